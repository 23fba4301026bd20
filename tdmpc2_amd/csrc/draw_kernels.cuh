// Kernels of the draw unit (tdmpc2_draw_noise), included by k_draw.hip alone.  Every decision (the walk over quads, the decode, the
// uniform of a word, the pair, the counter's increment) is draw_route.h's; the Philox rounds are common.cuh's philox4x32_10.  The
// Box-Muller step uses the precise logf / sqrtf / sincospif: the result is gated against an fp64 restatement of the same words.
#pragma once

struct DrawParams {
    uint64_t n;                // normals
    int32_t num_q;             // read when pair is not null
    uint32_t seed_lo, seed_hi;
    uint32_t call_lo, call_hi; // used when state is null
    const uint32_t *state;     // two words (lo, hi) or null; read only
    float *normal;             // [n], 16-byte aligned, or null (n == 0)
    int32_t *pair;             // [2] or null
};

// two normals from two words: r cos(2 pi u1), r sin(2 pi u1), r = sqrt(-2 ln u0)
__device__ __forceinline__ void draw_normal2(uint32_t w0, uint32_t w1, float &c, float &s) {
    const float r = sqrtf(-2.0f * logf(draw_u01(w0)));
    float sn, cs;
    sincospif(2.0f * draw_u01(w1), &sn, &cs);
    c = r * cs;
    s = r * sn;
}

// one thread per quad, grid-stride: a full quad leaves in one 16-byte store, the last partial quad in single-element stores; thread 0
// of workgroup 0 writes the pair from the counter no quad reaches
__global__ __launch_bounds__(DRAW_THREADS) void k_draw(DrawParams p) {
    uint32_t call_lo = p.call_lo, call_hi = p.call_hi;
    if (p.state) {
        call_lo = p.state[0];
        call_hi = p.state[1];
    }
    const uint2 key = make_uint2(p.seed_lo, p.seed_hi);
    if (p.pair && blockIdx.x == 0 && threadIdx.x == 0) {
        const uint4 w = philox4x32_10(make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, call_lo, call_hi), key);
        int32_t i, j;
        draw_pair(w.x, w.y, p.num_q, i, j);
        p.pair[0] = i;
        p.pair[1] = j;
    }
    const uint64_t quads = draw_quads(p.n), stride = draw_quad_stride(gridDim.x);
    for (uint64_t q = draw_first_quad(blockIdx.x, (int)threadIdx.x); q < quads; q += stride) {
        const uint4 w = philox4x32_10(make_uint4((uint32_t)q, (uint32_t)(q >> 32), call_lo, call_hi), key);
        float v0, v1, v2, v3;
        draw_normal2(w.x, w.y, v0, v1);
        draw_normal2(w.z, w.w, v2, v3);
        float *dst = p.normal + (q << 2);
        const int live = draw_quad_elems(q, p.n);
        if (live == 4) {
            *reinterpret_cast<float4 *>(dst) = make_float4(v0, v1, v2, v3);
        } else {
            dst[0] = v0;
            if (live > 1) dst[1] = v1;
            if (live > 2) dst[2] = v2;
        }
    }
}

// the call counter + 1 with carry: one thread, after the draw kernel in the same stream
__global__ __launch_bounds__(64) void k_draw_bump(uint32_t *state) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t lo = state[0], hi = state[1];
    draw_bump(lo, hi);
    state[0] = lo;
    state[1] = hi;
}
