// The arithmetic of the draw unit (tdmpc2_draw_noise, include/tdmpc2_draw.h): the refusals on the descriptor, the grid and its walk,
// the quad / lane decode, the uniform of a word, the pair of heads and one element restated serially (Philox rounds included, the
// Box-Muller step in fp64), as pure functions.  Compilable on the host, no HIP types: tests/test_draw_route.py builds it with the
// host compiler.  The host side (k_draw.hip) launches what draw_grid returns; the kernel (draw_kernels.cuh) walks quads with
// draw_first_quad / draw_quad_stride, decodes them with the same functions and forms the pair with draw_pair.
//
// Element e of n: quad q = e >> 2, lane j = e & 3.  Words of a quad: w = philox4x32_10((q_lo, q_hi, call_lo, call_hi), (seed_lo,
// seed_hi)).  u(x) = draw_u01(x): the fp32 value of ((float)(x >> 8) + 0.5f) * 2^-24 (common.cuh's u01; 0 < u <= 1).  Lanes 0 / 1:
// r cos(2 pi u(w1)) / r sin(2 pi u(w1)), r = sqrt(-2 ln u(w0)); lanes 2 / 3 the same from (w2, w3).
// The pair: words of counter (0xFFFFFFFF, 0xFFFFFFFF, call_lo, call_hi), which no quad reaches (n < 2^62); i = (w0 * num_q) >> 32,
// k = (w1 * (num_q - 1)) >> 32, j = k + (k >= i).
// One thread per quad, DRAW_THREADS per workgroup, at most DRAW_MAX_BLOCKS workgroups: thread t of workgroup b takes quads
// b * DRAW_THREADS + t, + grid * DRAW_THREADS, ... below draw_quads(n); thread 0 of workgroup 0 also writes the pair.
#pragma once
#include "seed_route.h"  // <math.h>, <stdint.h> and the __host__ / __device__ shim for the host compiler of the test

// 2048 workgroups of 256 threads, as the dropout unit's grid: 2^21 elements in one pass
enum { DRAW_THREADS = 256, DRAW_MAX_BLOCKS = 2048, DRAW_MAXQ = 8 /* MAXQ of common.cuh */ };

struct DrawDesc {  // tdmpc2_draw_desc
    int64_t n;
    int32_t num_q;
    uint32_t seed_lo, seed_hi, call_lo, call_hi, reserved;
};

// ---- what the entry point refuses: 0 = fine, else the index of the message in k_draw.hip.  has_normal / has_pair: the output
// pointer is not null; normal_addr: the address of `normal` (alignment)
enum { DRAW_OK = 0, DRAW_NO_OUTPUT, DRAW_NEG_N, DRAW_ZERO_N, DRAW_NULL_NORMAL, DRAW_MISALIGNED, DRAW_BAD_Q, DRAW_HUGE_N };
__host__ __device__ inline int draw_check(const DrawDesc &d, bool has_normal, bool has_pair, uint64_t normal_addr) {
    if (!has_normal && !has_pair) return DRAW_NO_OUTPUT;
    if (d.n < 0) return DRAW_NEG_N;
    if (d.n == 0 && has_normal) return DRAW_ZERO_N;
    if (d.n > 0 && !has_normal) return DRAW_NULL_NORMAL;
    if (has_normal && (normal_addr & 15u)) return DRAW_MISALIGNED;
    if (has_pair && (d.num_q < 2 || d.num_q > DRAW_MAXQ)) return DRAW_BAD_Q;
    if (d.n >= ((int64_t)1 << 62)) return DRAW_HUGE_N;
    return DRAW_OK;
}

// ---- the grid and its walk (a call with the pair alone, n == 0, still launches one workgroup)
__host__ __device__ inline uint64_t draw_quads(uint64_t n) { return (n + 3) >> 2; }
__host__ __device__ inline uint64_t draw_grid(uint64_t n) {
    const uint64_t blocks = (draw_quads(n) + (DRAW_THREADS - 1)) / DRAW_THREADS;
    return blocks < 1 ? 1 : blocks < DRAW_MAX_BLOCKS ? blocks : (uint64_t)DRAW_MAX_BLOCKS;
}
__host__ __device__ inline uint64_t draw_first_quad(uint64_t block, int thread) { return block * DRAW_THREADS + (uint64_t)thread; }
__host__ __device__ inline uint64_t draw_quad_stride(uint64_t grid) { return grid * DRAW_THREADS; }
__host__ __device__ inline uint64_t draw_quad_of(uint64_t e) { return e >> 2; }
__host__ __device__ inline int draw_lane_of(uint64_t e) { return (int)(e & 3); }
// elements of quad q that lie below n: 4 (one 16-byte store) or 1..3 (the last partial quad)
__host__ __device__ inline int draw_quad_elems(uint64_t q, uint64_t n) { return n - (q << 2) >= 4 ? 4 : (int)(n - (q << 2)); }

// ---- the call counter's increment (the one-thread launch): + 1 with carry
__host__ __device__ inline void draw_bump(uint32_t &lo, uint32_t &hi) {
    lo += 1u;
    if (lo == 0u) hi += 1u;
}

// ---- the uniform of a word: the top 24 bits at the middle of their cell, formed in fp32 (above 2^23 the half rounds to even, so
// the largest word gives exactly 1 and a radius of 0; no word gives 0)
__host__ __device__ inline float draw_u01(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// ---- the pair of heads from the first two words of the pair counter: pure integer
__host__ __device__ inline void draw_pair(uint32_t w0, uint32_t w1, int32_t num_q, int32_t &i, int32_t &j) {
    i = (int32_t)(((uint64_t)w0 * (uint64_t)(uint32_t)num_q) >> 32);
    const int32_t k = (int32_t)(((uint64_t)w1 * (uint64_t)(uint32_t)(num_q - 1)) >> 32);
    j = k + (k >= i ? 1 : 0);
}

// ---- Philox4x32-10 restated for the host (the kernel uses common.cuh's philox4x32_10)
__host__ inline void draw_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
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
__host__ inline void draw_quad_words(const DrawDesc &d, uint64_t call, uint64_t q, uint32_t w[4]) {
    const uint32_t ctr[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)call, (uint32_t)(call >> 32)};
    const uint32_t key[2] = {d.seed_lo, d.seed_hi};
    draw_philox(ctr, key, w);
}

// lane j of a quad with words w, the Box-Muller step in fp64 on the fp32 uniforms: what the kernel's fp32 result is gated against
__host__ inline double draw_normal64(const uint32_t w[4], int lane) {
    const double u0 = (double)draw_u01(w[lane & 2]), u1 = (double)draw_u01(w[(lane & 2) + 1]);
    const double r = sqrt(-2.0 * log(u0)), a = 6.283185307179586476925286766559 * u1;
    return (lane & 1) ? r * sin(a) : r * cos(a);
}
// element e of the normals of descriptor d at call counter `call` (the descriptor's own, or what `state` held), serially
__host__ inline double draw_serial64(const DrawDesc &d, uint64_t call, uint64_t e) {
    uint32_t w[4];
    draw_quad_words(d, call, draw_quad_of(e), w);
    return draw_normal64(w, draw_lane_of(e));
}
// the pair of descriptor d at call counter `call`
__host__ inline void draw_pair_serial(const DrawDesc &d, uint64_t call, int32_t &i, int32_t &j) {
    uint32_t w[4];
    draw_quad_words(d, call, ~(uint64_t)0, w);
    draw_pair(w[0], w[1], d.num_q, i, j);
}
