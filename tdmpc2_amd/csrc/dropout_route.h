// The arithmetic of the dropout-mask unit (tdmpc2_dropout_*, include/tdmpc2_dropout.h): the drop threshold and the kept value, the
// grid and its walk, the quad / lane decode and one element restated serially (Philox rounds included), as pure functions.
// Compilable on the host, no HIP types: tests/test_dropout_route.py builds it with the host compiler.  The host side
// (k_dropout.hip) launches what drop_grid returns; the kernel (dropout_kernels.cuh) walks quads with drop_first_quad /
// drop_quad_stride and decodes them with the same functions.
//
// Element e of n: quad q = e >> 2, lane j = e & 3.  Words of a quad: philox4x32_10((q_lo, q_hi, call_lo, call_hi), (seed_lo,
// seed_hi)).  Dropped iff word_j < drop_thr(p); written +0.0f, else drop_keep(p).
// One thread per quad, DROP_THREADS per workgroup, at most DROP_MAX_BLOCKS workgroups: thread t of workgroup b takes quads
// b * DROP_THREADS + t, + grid * DROP_THREADS, ... below drop_quads(n).
#pragma once
#include "seed_route.h"  // <math.h>, <stdint.h> and the __host__ / __device__ shim for the host compiler of the test

// 2048 workgroups of 256 threads: 8 per compute unit of an MI355X, 2^21 elements (8 MiB) in one pass
enum { DROP_THREADS = 256, DROP_MAX_BLOCKS = 2048 };

struct DropDesc {  // tdmpc2_dropout_desc
    int64_t n;
    float p;
    uint32_t seed_lo, seed_hi, call_lo, call_hi, reserved;
};

// ---- what the entry point refuses on the descriptor alone: 0 = fine, else the index of the message in k_dropout.hip
enum { DROP_OK = 0, DROP_BAD_N, DROP_BAD_P, DROP_HUGE_N };
__host__ __device__ inline int drop_check(const DropDesc &d) {
    if (d.n < 1) return DROP_BAD_N;
    if (!(d.p >= 0.0f) || !(d.p < 1.0f)) return DROP_BAD_P;  // (NaN fails both comparisons)
    if (d.n >= ((int64_t)1 << 62)) return DROP_HUGE_N;
    return DROP_OK;
}

// ---- constants of a call (host): P(drop) = thr / 2^32 exactly; keep as torch's dropout forms it (fp32 one over fp32 (1 - p))
__host__ inline uint32_t drop_thr(float p) { return (uint32_t)floor((double)p * 4294967296.0); }
__host__ inline float drop_keep(float p) { return 1.0f / (float)(1.0 - (double)p); }

// ---- the grid and its walk
__host__ __device__ inline uint64_t drop_quads(uint64_t n) { return (n + 3) >> 2; }
__host__ __device__ inline uint64_t drop_grid(uint64_t n) {
    const uint64_t blocks = (drop_quads(n) + (DROP_THREADS - 1)) / DROP_THREADS;
    return blocks < DROP_MAX_BLOCKS ? blocks : (uint64_t)DROP_MAX_BLOCKS;
}
__host__ __device__ inline uint64_t drop_first_quad(uint64_t block, int thread) { return block * DROP_THREADS + (uint64_t)thread; }
__host__ __device__ inline uint64_t drop_quad_stride(uint64_t grid) { return grid * DROP_THREADS; }
__host__ __device__ inline uint64_t drop_quad_of(uint64_t e) { return e >> 2; }
__host__ __device__ inline int drop_lane_of(uint64_t e) { return (int)(e & 3); }
// elements of quad q that lie below n: 4 (one 16-byte store) or 1..3 (the last partial quad)
__host__ __device__ inline int drop_quad_elems(uint64_t q, uint64_t n) { return n - (q << 2) >= 4 ? 4 : (int)(n - (q << 2)); }

// ---- the call counter's increment (the one-thread launch): + 1 with carry
__host__ __device__ inline void drop_bump(uint32_t &lo, uint32_t &hi) {
    lo += 1u;
    if (lo == 0u) hi += 1u;
}

// ---- Philox4x32-10 restated for the host (the kernel uses common.cuh's philox4x32_10)
__host__ inline void drop_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t m0 = (uint64_t)0xD2511F53u * c0, m1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(m1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)m1, n2 = (uint32_t)(m0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)m0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// element e of the mask of descriptor d at call counter `call` (the descriptor's own, or what `state` held), serially
__host__ inline float drop_serial(const DropDesc &d, uint64_t call, uint64_t e) {
    const uint64_t q = drop_quad_of(e);
    const uint32_t ctr[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)call, (uint32_t)(call >> 32)};
    const uint32_t key[2] = {d.seed_lo, d.seed_hi};
    uint32_t w[4];
    drop_philox(ctr, key, w);
    return w[drop_lane_of(e)] < drop_thr(d.p) ? 0.0f : drop_keep(d.p);
}
