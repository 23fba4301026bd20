// The arithmetic of the trainable layer (tdmpc2_layer_forward / tdmpc2_layer_backward): the three GEMMs as one strided
// description each, their tile grids, the maps from a lane's accumulator registers to output elements, the row split of the
// column reductions with the order of its partial sums, the workspace layout and 64-bit element offsets, as pure functions.
// Compilable on the host, no HIP types: tests/test_layer_grad_route.py builds it with the host compiler.  The host side
// (k_layer_grad.hip) walks what these return; the kernels (layer_grad_kernels.cuh) use the same functions to decode a workgroup.
//
// G = groups, R = rows, K = in_dim, N = out_dim.  Every GEMM is C[M x Nc] = sum_l A(m, l) B(l, n), one fmaf chain per element
// in the order l = 0 .. L - 1 (v_mfma_f32_32x32x2_f32 adds k = 0 then k = 1 of a step), chained over `gsum` groups g = 0 .. gsum - 1:
//   FWD  lin[g][r][n] = sum_k x[g][r][k]    w[g][n][k]     M = R, Nc = N, L = K   (both operands contiguous along l)
//   DX   dx [g][r][k] = sum_n dlin[g][r][n] w[g][n][k]     M = R, Nc = K, L = N   (A contiguous along l, B along n)
//   DW   dw [g][n][k] = sum_r dlin[g][r][n] x[g][r][k]     M = N, Nc = K, L = R   (A contiguous along m, B along n)
// With shared_x the x of FWD / DW has group stride 0, and DX is ONE output whose reduction runs over (g, n), g outermost, every
// group padded with zeros to whole trips.  A reduction is cut into partial chains of LG_SEG_TRIPS trips (256 elements); a partial
// chain starts from zero and the partials are added in rising order (lg_seg_end).  A serial chain of 4096 terms errs about
// 3.5 times more than a library GEMM's blocked sums; with the partials a long reduction stays beside one.  No reduction is split
// between workgroups: the order of an element's sum never depends on the grid or on the other rows of the call.
#pragma once
#include "seed_route.h"  // <math.h>, <stdint.h> and the __host__ / __device__ shim for the host compiler of the test

enum { LG_LINEAR = 0, LG_MISH = 1, LG_SIMNORM = 2 };
enum { LG_FWD = 0, LG_DX = 1, LG_DW = 2 };
enum { LG_THREADS = 256, LG_WAVES = 4 };
enum { LG_TILE = 32 };             // one MFMA accumulator: 32 x 32
enum { LG_BM = 64, LG_BN = 64 };   // a workgroup's output tile: 2 x 2 waves
enum { LG_KT = 32, LG_KSTEP = 2 }; // reduction elements staged per trip; per MFMA
enum { LG_SEG_TRIPS = 8 };         // trips per partial chain
enum { LG_LDS_LD = LG_BM + 1 };    // row stride of a staged tile [LG_KT][LG_LDS_LD] (odd: the transposing store spreads over the banks)
enum { LG_ROW_WAVES = 4 };         // row kernels: one wave per row, this many rows per workgroup
enum { LG_COLS = 32, LG_PARTS = 8 }; // column reductions: 32 columns x 8 row parts per workgroup
enum { LG_ALIGN = 256 };           // workspace regions start on this boundary

struct LgDesc {  // = tdmpc2_layer_desc
    int32_t kind, groups, rows, in_dim, out_dim, shared_x, simnorm_dim;
    float ln_eps;
};

// ---- 64-bit element offsets
__host__ __device__ inline uint64_t lg_off3(uint64_t g, uint64_t r, uint64_t c, uint64_t R, uint64_t C) { return (g * R + r) * C + c; }
__host__ __device__ inline uint64_t lg_off2(uint64_t g, uint64_t c, uint64_t C) { return g * C + c; }

// ---- one GEMM
struct LgGemm {
    int32_t M, Nc, L;        // output rows, output columns, chain length per group
    int32_t batch, gsum;     // outputs (grid), groups chained into each output
    int32_t tiles_m, tiles_n;
    uint64_t a_m, a_l, a_g;  // element strides of A(m, l) and per group
    uint64_t b_n, b_l, b_g;
    uint64_t ldc, c_g;
    uint64_t blocks;         // batch * tiles_m * tiles_n
};
__host__ __device__ inline LgGemm lg_gemm(int which, const LgDesc &d) {
    const uint64_t R = (uint64_t)d.rows, K = (uint64_t)d.in_dim, N = (uint64_t)d.out_dim;
    const uint64_t xg = d.shared_x ? 0 : R * K;
    LgGemm g{};
    g.batch = d.groups;
    g.gsum = 1;
    if (which == LG_FWD) {
        g.M = d.rows; g.Nc = d.out_dim; g.L = d.in_dim;
        g.a_m = K; g.a_l = 1; g.a_g = xg;
        g.b_n = K; g.b_l = 1; g.b_g = N * K;
        g.ldc = N; g.c_g = R * N;
    } else if (which == LG_DX) {
        g.M = d.rows; g.Nc = d.in_dim; g.L = d.out_dim;
        g.a_m = N; g.a_l = 1; g.a_g = R * N;
        g.b_n = 1; g.b_l = K; g.b_g = N * K;
        g.ldc = K; g.c_g = xg;
        if (d.shared_x) { g.batch = 1; g.gsum = d.groups; }
    } else {
        g.M = d.out_dim; g.Nc = d.in_dim; g.L = d.rows;
        g.a_m = 1; g.a_l = N; g.a_g = R * N;
        g.b_n = 1; g.b_l = K; g.b_g = xg;
        g.ldc = K; g.c_g = N * K;
    }
    g.tiles_m = (g.M + LG_BM - 1) / LG_BM;
    g.tiles_n = (g.Nc + LG_BN - 1) / LG_BN;
    g.blocks = (uint64_t)g.batch * (uint64_t)g.tiles_m * (uint64_t)g.tiles_n;
    return g;
}
__host__ __device__ inline uint64_t lg_a_off(const LgGemm &g, uint64_t grp, uint64_t m, uint64_t l) { return grp * g.a_g + m * g.a_m + l * g.a_l; }
__host__ __device__ inline uint64_t lg_b_off(const LgGemm &g, uint64_t grp, uint64_t l, uint64_t n) { return grp * g.b_g + l * g.b_l + n * g.b_n; }
__host__ __device__ inline uint64_t lg_c_off(const LgGemm &g, uint64_t out, uint64_t m, uint64_t n) { return out * g.c_g + m * g.ldc + n; }

// workgroup `blk` -> its output and the corner of its LG_BM x LG_BN tile (columns fastest: neighbours share the A rows)
struct LgTile {
    int32_t out, m0, n0;
};
__host__ __device__ inline LgTile lg_tile(const LgGemm &g, uint64_t blk) {
    LgTile t{};
    t.n0 = (int32_t)(blk % (uint64_t)g.tiles_n) * LG_BN;
    blk /= (uint64_t)g.tiles_n;
    t.m0 = (int32_t)(blk % (uint64_t)g.tiles_m) * LG_BM;
    t.out = (int32_t)(blk / (uint64_t)g.tiles_m);
    return t;
}
// wave w of a workgroup owns the 32 x 32 tile at (32 (w >> 1), 32 (w & 1)) of the workgroup's tile
__host__ __device__ inline int lg_wave_m(int wave) { return (wave >> 1) * LG_TILE; }
__host__ __device__ inline int lg_wave_n(int wave) { return (wave & 1) * LG_TILE; }
// accumulator register i (0 .. 15) of lane l holds element (row, col) of the wave's tile
__host__ __device__ inline int lg_acc_row(int lane, int i) { return (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5); }
__host__ __device__ inline int lg_acc_col(int lane) { return lane & 31; }
// MFMA step s of a staged trip: lane l supplies A(row l & 31, k) and B(k, col l & 31) with k = 2 s + (l >> 5)
__host__ __device__ inline int lg_step_k(int lane, int s) { return LG_KSTEP * s + (lane >> 5); }
__host__ __device__ inline int lg_trips(int L) { return (L + LG_KT - 1) / LG_KT; }
// after this trip (counted over all chained groups) the running chain is added to the element's total and restarts from zero
__host__ __device__ inline bool lg_seg_end(int trip) { return (trip + 1) % LG_SEG_TRIPS == 0; }

// ---- row kernels: one wave per row of [G R], lane l owns elements l, l + 64, ... (Mish) or SimNorm groups l, l + 64, ...;
// a row's sums are 64 per-lane serial sums folded by the butterfly xor 32, 16, 8, 4, 2, 1 (every lane ends with the same value)
__host__ __device__ inline uint64_t lg_row_blocks(const LgDesc &d) {
    return ((uint64_t)d.groups * (uint64_t)d.rows + LG_ROW_WAVES - 1) / LG_ROW_WAVES;
}

// ---- column reductions (db, dln_w, dln_b): a workgroup owns LG_COLS columns of one group; part p sums rows p, p + 8, ... in
// rising order, then the parts are added in the order p = 0 .. 7
__host__ __device__ inline int lg_col_part(int row) { return row % LG_PARTS; }
__host__ __device__ inline int lg_col_tiles(const LgDesc &d) { return (d.out_dim + LG_COLS - 1) / LG_COLS; }
__host__ __device__ inline uint64_t lg_col_blocks(const LgDesc &d) { return (uint64_t)d.groups * (uint64_t)lg_col_tiles(d); }

// ---- workspace of a backward call: dlin [G][R][N] (what the dX / dW GEMMs read), then for Mish / SimNorm du [G][R][N]
struct LgWs {
    uint64_t dlin_off, du_off, bytes;  // byte offsets
};
__host__ __device__ inline uint64_t lg_align_up(uint64_t x) { return (x + (LG_ALIGN - 1)) & ~(uint64_t)(LG_ALIGN - 1); }
__host__ __device__ inline LgWs lg_ws(const LgDesc &d) {
    const uint64_t act = lg_align_up((uint64_t)d.groups * (uint64_t)d.rows * (uint64_t)d.out_dim * sizeof(float));
    LgWs w{};
    w.dlin_off = 0;
    w.du_off = act;
    w.bytes = d.kind == LG_LINEAR ? act : 2 * act;
    return w;
}

// ---- what a call refuses before it touches the device: 0 = fine, else the index of the message in k_layer_grad.hip
enum { LG_OK = 0, LG_BAD_KIND, LG_BAD_DIMS, LG_BAD_SIMNORM, LG_BAD_SHARED, LG_TOO_LARGE };
__host__ __device__ inline int lg_check(const LgDesc &d) {
    if (d.kind != LG_LINEAR && d.kind != LG_MISH && d.kind != LG_SIMNORM) return LG_BAD_KIND;
    if (d.groups < 1 || d.rows < 1 || d.in_dim < 1 || d.out_dim < 1) return LG_BAD_DIMS;
    if (d.kind == LG_SIMNORM && (d.simnorm_dim < 1 || d.out_dim % d.simnorm_dim != 0)) return LG_BAD_SIMNORM;
    if (d.shared_x && d.groups == 1) return LG_BAD_SHARED;
    for (int which = LG_FWD; which <= LG_DW; ++which)
        if (lg_gemm(which, d).blocks > 0x7fffffffull) return LG_TOO_LARGE;
    if (lg_row_blocks(d) > 0x7fffffffull) return LG_TOO_LARGE;
    return LG_OK;
}
