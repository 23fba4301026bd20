// Which operations a call that stores weights enqueues (tdmpc2_plan_refresh_weights / soft_update_target with a table,
// tdmpc2_plan_bind_weights / bind_encoder / bind_policy with one layer), as a pure function of what the jobs name and of the
// handle's arithmetic.  Compilable on the host, no HIP types: tests/test_refresh_route.py builds it with the host compiler.
// The host side (plan_weights.hip) walks the list; the kernels are in refresh_kernels.cuh.
//
// A call is at most REFRESH_MAX_OPS = 4 launches, whatever the model: every launch is GROUPED over a job table (one job per
// (net, layer), all ensemble members inside it), so the count depends on neither num_q nor the number of nets or layers.
//   RO_RESET   max|W| / max|g| / max|b| words of every named net back to zero                      (split arithmetic)
//   RO_SCAN    max over the finite |W|, |ln_g|, |ln_b| of every matrix (integer atomicMax on the float bits: order independent);
//              a soft update lerps the target tensors in place in this launch and scans what it wrote   (split, or any lerp)
//   RO_SCALES  kw / wscale / ka / ascale of the named layers, oscale of every layer of their (net, head): k_rf_scales        (split)
//   RO_PACK    operand slabs, padded biases, LayerNorm vectors, task-embedding columns, the transposed encoder and the policy
//              prior's fp32 copy
// The dependency max -> scale -> pack crosses launch boundaries: no workgroup waits for another, no float atomics.
#pragma once
#include "seed_route.h"  // <math.h>, <stdint.h> and the __host__ / __device__ shim for the host compiler of the test

enum { RO_RESET = 0, RO_SCAN = 1, RO_SCALES = 2, RO_PACK = 3, REFRESH_MAX_OPS = 4 };
enum { RF_NETS = 6, RF_MAX_ENC = 6, RF_THREADS = 256 };
enum { RF_TILE_K = 128 };        // packed contraction columns per pack workgroup (x 32 rows, staged through LDS)
enum { RF_SCAN_CHUNK = 4096 };   // elements per scan workgroup ...
enum { RF_SCAN_MAX_BLOCKS = 512 };  // ... up to this many per matrix, then the workgroups stride

struct RefreshIn {
    int split;          // 1: f16x2 split arithmetic (scales exist), 0: exact fp32
    unsigned nets;      // bit n: TDMPC2_NET_n is named (a table names all three layers, a per-layer bind one)
    int enc_layers;     // state-encoder layers named (0: none)
    int policy_copy;    // 1: the policy prior's fp32 copy is bound and TDMPC2_NET_PI is named
    int lerp;           // 1: soft update (the named net is the target ensemble, lerped in place first)
    int num_q, episodic;  // part of the input on purpose: the answer must not depend on them
    int policy_alone;   // 1: a layer of the policy prior's fp32 copy on its own, whatever `nets` says (tdmpc2_plan_bind_policy)
};
struct RefreshRoute {
    int nops;
    int op[REFRESH_MAX_OPS];
    unsigned nets;      // nets the launches touch (== in.nets: nothing is launched for an absent net)
    int enc_layers, policy_copy;
};

inline RefreshRoute refresh_route(const RefreshIn &in) {
    RefreshRoute r{};
    const unsigned nets = in.nets & ((1u << RF_NETS) - 1u);
    r.nets = nets;
    r.enc_layers = in.enc_layers > 0 ? in.enc_layers : 0;
    r.policy_copy = ((in.policy_copy && (nets & (1u << 2))) || in.policy_alone) ? 1 : 0;
    if (!nets && !r.enc_layers && !in.policy_alone) return r;  // an empty table: nothing to do
    if (in.split && nets) {
        r.op[r.nops++] = RO_RESET;
        r.op[r.nops++] = RO_SCAN;
        r.op[r.nops++] = RO_SCALES;
    } else if (in.lerp && nets) {
        r.op[r.nops++] = RO_SCAN;  // exact fp32: nothing to scan, the launch only lerps
    }
    r.op[r.nops++] = RO_PACK;
    return r;
}

// ---- workgroups per job (the grids grow with the model, the launch count does not)
// scan: per ensemble member `rf_scan_wblocks` workgroups over the matrix + one for the vectors (bias, ln_g, ln_b)
__host__ __device__ inline int rf_scan_wblocks(long n) {
    long b = (n + RF_SCAN_CHUNK - 1) / RF_SCAN_CHUNK;
    return (int)(b < 1 ? 1 : (b > RF_SCAN_MAX_BLOCKS ? RF_SCAN_MAX_BLOCKS : b));
}
// pack: per ensemble member one workgroup per (32-row tile, RF_TILE_K packed columns) + one for the vectors + one per row tile
// for the task-embedding columns
__host__ __device__ inline int rf_pack_kchunks(int kp) { return (kp + RF_TILE_K - 1) / RF_TILE_K; }
__host__ __device__ inline int rf_pack_blocks(int ct, int kp, int nt) { return ct * rf_pack_kchunks(kp) + 1 + (nt > 0 ? ct : 0); }
// transposes (encoder, policy copy): one workgroup per 32 x 32 tile; the first one also copies the vectors
__host__ __device__ inline int rf_transpose_blocks(int out, int in) { return ((out + 31) / 32) * ((in + 31) / 32); }
