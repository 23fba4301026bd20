// Pixel-observation encoder (tdmpc2/common/layers.py:36-71, 136-150, with the SimNorm of layers.py:74-91):
//   z = SimNorm(Flatten(conv4(ReLU(conv3(ReLU(conv2(ReLU(conv1(ShiftAug(obs) / 255 - 0.5)))))))))
// 16.7 M MACs per image at 32 channels: plain fp32 FMAs, no matrix pipe.  A thread computes one output pixel of PIX_CO channels;
// the weights are re-packed at bind to [cin][k][k][C] so that a tap's PIX_CO weights are one float4 (the same address across a
// wave).  ShiftAug and the preprocessing run inside the first convolution: every tap samples the uint8 / fp32 frames through the
// resampling table of pixel_route.h (source indices + bilinear weights), so the resampled stack is never stored.
// Routes, grids and work items: pixel_route.h.  Included by k_plan.hip inside its anonymous namespace.
#pragma once
#include "pixel_route.h"

struct PixParams : PixArgs {};  // the kernels' own name for the block of launch.h ("kernel parameter types" there)

template <bool U8>
__device__ __forceinline__ float pix_px(const void *plane, int off) {
    if (U8) return (float)static_cast<const uint8_t *>(plane)[off];
    return static_cast<const float *>(plane)[off];
}

// layer 0: ShiftAug + PixelPreprocess + conv 7x7/2 of output pixel (oy, ox), channels c0.. of image e
template <bool U8>
__device__ __forceinline__ void pix_conv0(const PixParams &p, int e, int c0, int oy, int ox, float acc[PIX_CO]) {
    constexpr int K = 7, S = 2;
    const int dx = pix_clamp_shift(p.shift[2 * e]), dy = pix_clamp_shift(p.shift[2 * e + 1]);
    const PixTap *tx = p.tab + dx * PIX_IN, *ty = p.tab + dy * PIX_IN;
    const size_t plane = (size_t)PIX_IN * PIX_IN;
    const char *img = static_cast<const char *>(p.obs) + (size_t)e * p.cin * plane * (U8 ? 1 : 4);
    for (int ky = 0; ky < K; ++ky) {
        const PixTap r = ty[S * oy + ky];
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const PixTap c = tx[S * ox + kx];
            // grid_sample's bilinear weights (nw, ne, sw, se) and source offsets
            const float wnw = c.w0 * r.w0, wne = c.w1 * r.w0, wsw = c.w0 * r.w1, wse = c.w1 * r.w1;
            const int onw = r.lo * PIX_IN + c.lo, one = r.lo * PIX_IN + c.hi, osw = r.hi * PIX_IN + c.lo, ose = r.hi * PIX_IN + c.hi;
            const float *w = p.wp[0] + (size_t)(ky * K + kx) * p.C + c0;
            for (int ci = 0; ci < p.cin; ++ci) {
                const void *pl = img + (size_t)ci * plane * (U8 ? 1 : 4);
                float v = 0.f;
                v += pix_px<U8>(pl, onw) * wnw;
                v += pix_px<U8>(pl, one) * wne;
                v += pix_px<U8>(pl, osw) * wsw;
                v += pix_px<U8>(pl, ose) * wse;
                v = v / 255.0f - 0.5f;
                const float4 wv = *reinterpret_cast<const float4 *>(w + (size_t)ci * K * K * p.C);
                acc[0] = fmaf(v, wv.x, acc[0]);
                acc[1] = fmaf(v, wv.y, acc[1]);
                acc[2] = fmaf(v, wv.z, acc[2]);
                acc[3] = fmaf(v, wv.w, acc[3]);
            }
        }
    }
}

// layers 1..3: conv KxK/S of output pixel (oy, ox) over the previous layer's [C][side][side] output `in`
template <int L>
__device__ __forceinline__ void pix_conv(const PixParams &p, const float *in, int c0, int oy, int ox, float acc[PIX_CO]) {
    constexpr int K = pix_kernel(L), S = pix_stride(L), side = pix_side(L);
    for (int ci = 0; ci < p.C; ++ci) {
        const float *src = in + (size_t)ci * side * side + (S * oy) * side + S * ox;
        const float *w = p.wp[L] + (size_t)ci * K * K * p.C + c0;
#pragma unroll
        for (int ky = 0; ky < K; ++ky)
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const float v = src[ky * side + kx];
                const float4 wv = *reinterpret_cast<const float4 *>(w + (size_t)(ky * K + kx) * p.C);
                acc[0] = fmaf(v, wv.x, acc[0]);
                acc[1] = fmaf(v, wv.y, acc[1]);
                acc[2] = fmaf(v, wv.z, acc[2]);
                acc[3] = fmaf(v, wv.w, acc[3]);
            }
    }
}

// One work item of layer L: `in` = the image's layer-(L-1) output (L > 0), `out` = its layer-L output [C][hw] (L < 3) or its
// latent row (L == 3: SimNorm over groups of 8 pixels of a channel).  Every lane of a wave calls this, valid or not: the last
// layer's SimNorm reduces across lanes.
template <int L>
__device__ __forceinline__ void pix_item(const PixParams &p, const PixItem it, const float *in, float *out) {
    float acc[PIX_CO] = {0.f, 0.f, 0.f, 0.f};
    const int oy = it.p / pix_out(L), ox = it.p % pix_out(L);
    if (it.valid) {
        if (L == 0) {
            if (p.obs_u8) pix_conv0<true>(p, it.e, it.c0, oy, ox, acc);
            else pix_conv0<false>(p, it.e, it.c0, oy, ox, acc);
        } else {
            pix_conv<L>(p, in, it.c0, oy, ox, acc);
        }
    }
#pragma unroll
    for (int u = 0; u < PIX_CO; ++u) {
        const int c = it.c0 + u;
        const float y = acc[u] + (it.valid ? p.bias[L][c] : 0.f);
        if (L < PIX_LAYERS - 1) {
            if (it.valid) out[(size_t)c * pix_hw(L) + it.p] = fmaxf(y, 0.f);
        } else {
            // Flatten: feature c * 16 + p; SimNorm groups = 8 consecutive pixels = 8 adjacent lanes (pixel blocks start at lane 0)
            float mx = it.valid ? y : -INFINITY;
            for (int o = 1; o < 8; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            const float ex = it.valid ? expf(y - mx) : 0.f;
            float s = ex;
            for (int o = 1; o < 8; o <<= 1) s += __shfl_xor(s, o);
            if (it.valid) out[(size_t)c * pix_hw(L) + it.p] = ex / s;
        }
    }
}

// spread route: one launch per layer, grid (pixel blocks, channel groups, images)
template <int L>
__global__ __launch_bounds__(PIX_SPREAD_WG) void k_pix_spread(PixParams p) {
    const PixItem it = pix_spread_item(L, blockIdx.x, blockIdx.y, blockIdx.z, threadIdx.x);
    const size_t img = (size_t)it.e * pix_ws_floats(p.C);
    const float *in = L > 0 ? p.ws + img + pix_ws_off(L - 1, p.C) : nullptr;
    float *out = L < PIX_LAYERS - 1 ? p.ws + img + pix_ws_off(L, p.C) : p.z + (size_t)it.e * 16 * p.C;
    pix_item<L>(p, it, in, out);
}

// per-image route: one workgroup per image, the whole stack, layer outputs 0..2 in LDS
template <int L>
__device__ __forceinline__ void pix_image_layer(const PixParams &p, float *lds, int e) {
    const float *in = L > 0 ? lds + pix_image_lds_off(L - 1, p.C) : nullptr;
    float *out = L < PIX_LAYERS - 1 ? lds + pix_image_lds_off(L, p.C) : p.z + (size_t)e * 16 * p.C;
    const int n = pix_image_items(L, p.C);  // a multiple of 64: the loop's trip count is uniform across a wave
    for (int i = threadIdx.x; i < n; i += PIX_IMAGE_WG) pix_item<L>(p, pix_image_item(L, p.C, e, i), in, out);
    __syncthreads();
}
__global__ __launch_bounds__(PIX_IMAGE_WG) void k_pix_image(PixParams p) {
    extern __shared__ float pix_lds[];
    const int e = blockIdx.x;
    pix_image_layer<0>(p, pix_lds, e);
    pix_image_layer<1>(p, pix_lds, e);
    pix_image_layer<2>(p, pix_lds, e);
    pix_image_layer<3>(p, pix_lds, e);
}

// Conv2d weight [C][cin][k][k] -> [cin][k][k][C]
__global__ void k_pix_pack(const float *__restrict__ w, float *__restrict__ wp, int C, int cin, int kk) {
    const int n = C * cin * kk;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int co = i % C, r = i / C;  // r = ci * kk + tap
        wp[i] = w[(size_t)co * cin * kk + r];
    }
}
