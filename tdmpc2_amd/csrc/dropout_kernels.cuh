// Kernels of the dropout-mask unit (tdmpc2_dropout_mask), included by k_dropout.hip alone.  Every decision (the walk over quads,
// the decode, the counter's increment) is dropout_route.h's; the Philox rounds are common.cuh's philox4x32_10.
#pragma once

struct DropParams {
    uint64_t n;                // elements
    uint32_t thr;              // drop_thr(p)
    float keep;                // drop_keep(p)
    uint32_t seed_lo, seed_hi;
    uint32_t call_lo, call_hi; // used when state is null
    const uint32_t *state;     // two words (lo, hi) or null; read only
    float *mask;               // [n], 16-byte aligned
};

// one thread per quad, grid-stride: a full quad leaves in one 16-byte store, the last partial quad in single-element stores
__global__ __launch_bounds__(DROP_THREADS) void k_drop_mask(DropParams p) {
    uint32_t call_lo = p.call_lo, call_hi = p.call_hi;
    if (p.state) {
        call_lo = p.state[0];
        call_hi = p.state[1];
    }
    const uint64_t quads = drop_quads(p.n), stride = drop_quad_stride(gridDim.x);
    for (uint64_t q = drop_first_quad(blockIdx.x, (int)threadIdx.x); q < quads; q += stride) {
        const uint4 w = philox4x32_10(make_uint4((uint32_t)q, (uint32_t)(q >> 32), call_lo, call_hi), make_uint2(p.seed_lo, p.seed_hi));
        const float v0 = w.x < p.thr ? 0.0f : p.keep, v1 = w.y < p.thr ? 0.0f : p.keep;
        const float v2 = w.z < p.thr ? 0.0f : p.keep, v3 = w.w < p.thr ? 0.0f : p.keep;
        float *dst = p.mask + (q << 2);
        const int live = drop_quad_elems(q, p.n);
        if (live == 4) {
            *reinterpret_cast<float4 *>(dst) = make_float4(v0, v1, v2, v3);
        } else {
            dst[0] = v0;
            if (live > 1) dst[1] = v1;
            if (live > 2) dst[2] = v2;
        }
    }
}

// the call counter + 1 with carry: one thread, after the mask kernel in the same stream
__global__ __launch_bounds__(64) void k_drop_bump(uint32_t *state) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t lo = state[0], hi = state[1];
    drop_bump(lo, hi);
    state[0] = lo;
    state[1] = hi;
}
