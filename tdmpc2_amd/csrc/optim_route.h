// The arithmetic of the optimiser step (tdmpc2_optim_*): the layout of the flat arenas, their cut into workgroup chunks, the map
// from an arena quad to its segment, the summation order of the gradient norm and the grids, as pure functions.  Compilable on
// the host, no HIP types: tests/test_optim_route.py builds it with the host compiler.  The host side (k_optim.hip) walks what these
// return; the kernels (optim_kernels.cuh) use the same functions to decode a workgroup.
//
// Layout.  Segment i (one parameter tensor of count[i] floats) starts at offset[i] = sum over j < i of opt_pad(count[j]) in each of
// the three arenas (grad, exp_avg, exp_avg_sq): every segment is padded with zeros to whole quads (4 floats, 16 bytes), so a quad
// belongs to exactly one segment and every arena access is one aligned 16-byte access.  The kernels write zeros to the padding.
//
// Chunks.  The arena is cut into chunks of OPT_CHUNK floats, one workgroup of OPT_THREADS threads each, in the norm pass and in the
// update pass alike; thread t of chunk c owns the quads opt_quad(c, t, j), j = 0 .. OPT_QUADS_PER_THREAD - 1 (consecutive lanes,
// consecutive quads).  A chunk may hold many segments: chunk_seg[c] = the segment of its first quad bounds the binary search
// (opt_seg_of_quad) every quad makes.
//
// Norm: chunk -> partial -> total, no atomics, no waits between workgroups; the order depends on the arena length alone.
//   thread   acc = 0; for j, for i = 0 .. 3: acc = acc + g[i] * g[i]   (product and sum rounded separately; quads past the arena skipped)
//   wave     acc = acc + (acc of lane ^ w) for w = 32, 16, 8, 4, 2, 1    (every lane ends with the same value)
//   chunk    partial[c] = ((wave 0 + wave 1) + wave 2) + wave 3
//   total    one workgroup: thread t sums partial[t], partial[t + OPT_THREADS], ... in rising order from 0, then the wave and
//            chunk steps above; norm = sqrt(total), correctly rounded
// opt_norm_depth counts the longest chain of additions an element's square passes through (D of the a-priori bound: every term is
// non-negative, so |norm - norm64| <= (D + 2) 2^-24 norm64 -- D + 1 roundings on the sum of squares, halved by the root, one for it).
#pragma once
#include "seed_route.h"  // <math.h>, <stdint.h> and the __host__ / __device__ shim for the host compiler of the test

enum { OPT_THREADS = 256, OPT_WAVES = 4 };
enum { OPT_QUAD = 4 };                                           // floats per 16-byte access
enum { OPT_QUADS_PER_THREAD = 2 };
enum { OPT_CHUNK_QUADS = OPT_THREADS * OPT_QUADS_PER_THREAD };   // 512
enum { OPT_CHUNK = OPT_CHUNK_QUADS * OPT_QUAD };                 // 2048 floats: 8 KiB of each arena per workgroup
enum { OPT_ALIGN = 256 };                                        // regions of the handle's device block start on this boundary

struct OptSeg {  // device record of one segment
    float *param;
    uint64_t quad0;  // first arena quad
    uint64_t count;  // floats
    int32_t group, reserved;
};

// ---- layout
__host__ __device__ inline uint64_t opt_pad(uint64_t count) { return (count + (OPT_QUAD - 1)) & ~(uint64_t)(OPT_QUAD - 1); }
// offsets[i] of n segments (may be null); returns the arena length in floats (a multiple of 4).  stride: bytes between two counts
__host__ __device__ inline uint64_t opt_layout(int64_t n, const int64_t *count0, uint64_t stride, int64_t *offsets) {
    uint64_t at = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (offsets) offsets[i] = (int64_t)at;
        at += opt_pad((uint64_t)*(const int64_t *)((const unsigned char *)count0 + (uint64_t)i * stride));
    }
    return at;
}

// ---- chunks
__host__ __device__ inline uint64_t opt_chunks(uint64_t arena_floats) { return (arena_floats + (OPT_CHUNK - 1)) / OPT_CHUNK; }
__host__ __device__ inline uint64_t opt_quad(uint64_t chunk, int thread, int j) {
    return chunk * OPT_CHUNK_QUADS + (uint64_t)j * OPT_THREADS + (uint64_t)thread;
}
// the largest s in [lo, hi] with quad0[s] <= quad (quad0 rising, quad0[lo] <= quad); stride: bytes between two quad0 entries
__host__ __device__ inline int32_t opt_seg_of_quad(const void *quad0, uint64_t stride, int32_t lo, int32_t hi, uint64_t quad) {
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (*(const uint64_t *)((const unsigned char *)quad0 + (uint64_t)mid * stride) <= quad) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- norm
__host__ __device__ inline uint64_t opt_total_terms(uint64_t chunks) { return (chunks + (OPT_THREADS - 1)) / OPT_THREADS; }  // per thread of the total pass
__host__ __device__ inline uint64_t opt_norm_depth(uint64_t arena_floats) {
    const uint64_t wave = 6, waves = OPT_WAVES - 1;
    return (uint64_t)OPT_QUADS_PER_THREAD * OPT_QUAD + wave + waves + opt_total_terms(opt_chunks(arena_floats)) + wave + waves;
}

// ---- the handle's one device block: segment records | chunk_seg [chunks + 1] | lr [groups] | state | partial [chunks]
struct OptState {  // device scalars: a captured step advances them on replay
    int64_t step;
    double b1p, b2p;        // beta1^step, beta2^step as running products from 1
    float norm, clip, bc, reserved;
    // float ss[groups] follows: lr_g / (1 - b1p)
};
struct OptBlock {
    uint64_t segs_off, chunk_seg_off, lr_off, state_off, ss_off, partial_off, bytes;
};
__host__ __device__ inline uint64_t opt_align_up(uint64_t x) { return (x + (OPT_ALIGN - 1)) & ~(uint64_t)(OPT_ALIGN - 1); }
__host__ __device__ inline OptBlock opt_block(uint64_t n_segs, uint64_t n_groups, uint64_t chunks) {
    OptBlock b{};
    b.segs_off = 0;
    b.chunk_seg_off = opt_align_up(n_segs * sizeof(OptSeg));
    b.lr_off = b.chunk_seg_off + opt_align_up((chunks + 1) * sizeof(int32_t));
    b.state_off = b.lr_off + opt_align_up(n_groups * sizeof(float));
    b.ss_off = b.state_off + sizeof(OptState);
    b.partial_off = b.state_off + opt_align_up(sizeof(OptState) + n_groups * sizeof(float));
    b.bytes = b.partial_off + opt_align_up(chunks * sizeof(float));
    return b;
}

// ---- what create refuses before it touches the device: 0 = fine, else the index of the message in k_optim.hip
enum { OPT_OK = 0, OPT_BAD_SEG, OPT_BAD_GROUP, OPT_NULL_PARAM, OPT_BAD_HYPER };
__host__ __device__ inline int opt_check_hyper(float beta1, float beta2, float eps, float max_norm) {
    // (written so that a NaN fails every test)
    if (!(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(eps > 0.0f) || !(max_norm > 0.0f)) return OPT_BAD_HYPER;
    return OPT_OK;
}
__host__ __device__ inline int opt_check_seg(int64_t count, int32_t group, int32_t n_groups, const void *param) {
    if (count < 1 || count > ((int64_t)1 << 48)) return OPT_BAD_SEG;
    if (group < 0 || group >= n_groups) return OPT_BAD_GROUP;
    if (!param) return OPT_NULL_PARAM;
    return OPT_OK;
}
