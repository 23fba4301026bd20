// What the seed units (loss_grad_route.h, pi_grad_route.h) share, as pure functions: the grid of a launch whose workgroups are
// several kinds of work in a row and its decode, the step of a unit of [.., T, B] work, rho^t, and the order of the 256-thread sums.
// Compilable on the host, no HIP types.  Its first lines are the shim every *_route.h needs under the host compiler of its test.
#pragma once
#include <math.h>
#include <stdint.h>
#ifndef __host__  // the host compiler of the test
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

enum { SEED_THREADS = 256 };  // threads of a workgroup of both units, and of their sums

// ---- grids
template <int KINDS>
struct SeedGrid {
    uint64_t first[KINDS + 1];  // first workgroup of each kind; first[KINDS] = workgroups of the launch
};
// kind k takes ceil(units(k) / per(k)) workgroups if bit k of `want` is set, none otherwise
template <int KINDS, class Units, class Per>
__host__ __device__ inline SeedGrid<KINDS> seed_grid(int want, Units units, Per per) {
    SeedGrid<KINDS> g{};
    uint64_t at = 0;
    for (int k = 0; k < KINDS; ++k) {
        g.first[k] = at;
        if (!((want >> k) & 1)) continue;
        at += (units(k) + (per(k) - 1)) / per(k);
    }
    g.first[KINDS] = at;
    return g;
}
// workgroup `block` (< first[KINDS]) -> its kind and its index inside the kind; a kind with no workgroups is skipped
template <int KINDS>
__host__ __device__ inline void seed_decode(const SeedGrid<KINDS> &g, uint64_t block, int &kind, uint64_t &local) {
    kind = 0;
    for (int k = 1; k < KINDS; ++k)
        if (block >= g.first[k]) kind = k;
    local = block - g.first[kind];
}

// ---- a descriptor D with steps, batch and rho
template <class D>
__host__ __device__ inline uint64_t seed_tb(const D &d) { return (uint64_t)d.steps * (uint64_t)d.batch; }
// the step of unit (.. * T + t) * B + b
template <class D>
__host__ __device__ inline int seed_step_of(const D &d, uint64_t unit) { return (int)((unit / (uint64_t)d.batch) % (uint64_t)d.steps); }
template <class D>
__host__ inline float seed_rho_pow(const D &d, int t) { return (float)pow((double)d.rho, (double)t); }

// ---- the order of the sums, restated serially (the kernels run the same additions on SEED_THREADS threads): thread i adds
// term(i), term(i + SEED_THREADS), ... from 0 in rising order, then an in-place tree red[i] += red[i + w], w = 128, 64, .. 1
template <class Term>
__host__ inline float seed_ordered_sum(uint64_t n, Term term) {
    float red[SEED_THREADS];
    for (int i = 0; i < SEED_THREADS; ++i) {
        float s = 0.0f;
        for (uint64_t k = (uint64_t)i; k < n; k += SEED_THREADS) s = s + term(k);
        red[i] = s;
    }
    for (int w = SEED_THREADS / 2; w > 0; w >>= 1)
        for (int i = 0; i < w; ++i) red[i] = red[i] + red[i + w];
    return red[0];
}
__host__ inline float seed_ordered_sum(const float *src, uint64_t n) {
    return seed_ordered_sum(n, [=](uint64_t k) { return src[k]; });
}
