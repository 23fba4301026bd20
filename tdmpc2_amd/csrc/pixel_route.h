// The pixel encoder's geometry (tdmpc2/common/layers.py:36-71, 136-150: ShiftAug, PixelPreprocess, four Conv2d, Flatten,
// SimNorm) and its launch routes: which route encodes a call, the grids, the work item of every thread, the LDS of a workgroup,
// the workspace bind allocates, and ShiftAug's resampling table.  Pure functions; pixel_kernels.cuh, plan_obs.hip and plan_weights.hip call
// them, tests/test_pixel_route.py compiles this header with g++ and checks them on the CPU (tests/pixel_route_model.py).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

constexpr int PIX_IN = 64;          // observation side (the encoder is laid out for 64 x 64 frames only)
constexpr int PIX_PAD = 3;          // ShiftAug's replicate padding
constexpr int PIX_FULL = PIX_IN + 2 * PIX_PAD;  // 70
constexpr int PIX_SHIFTS = 2 * PIX_PAD + 1;     // integer shifts 0 .. 6 per axis
constexpr int PIX_LAYERS = 4;
constexpr int PIX_CO = 4;           // output channels per thread (one float4 of the re-packed weights per tap)
constexpr int PIX_SPREAD_WG = 64;   // threads of a spread-route workgroup: 64 output pixels of PIX_CO channels of one image
constexpr int PIX_IMAGE_WG = 1024;  // threads of a per-image workgroup
constexpr size_t PIX_LDS_MAX = 160 * 1024;
constexpr int PIX_MAX_CIN = 16;
constexpr int PIX_MIN_C = 8, PIX_MAX_C = 64;

// layer l: kernel, stride, input side, output side (64 -> 29 -> 13 -> 6 -> 4, no padding)
__host__ __device__ constexpr int pix_kernel(int l) { return l == 0 ? 7 : l == 1 ? 5 : 3; }
__host__ __device__ constexpr int pix_stride(int l) { return l < 3 ? 2 : 1; }
__host__ __device__ constexpr int pix_side(int l) { return l == 0 ? 64 : l == 1 ? 29 : l == 2 ? 13 : l == 3 ? 6 : 4; }  // input of layer l
__host__ __device__ constexpr int pix_out(int l) { return pix_side(l + 1); }
__host__ __device__ constexpr int pix_hw(int l) { return pix_out(l) * pix_out(l); }          // output pixels of layer l
__host__ __device__ constexpr int pix_hw_pad(int l) { return (pix_hw(l) + 63) / 64 * 64; }   // ... rounded to whole waves

// ---------------------------------------------------------------------------------------------------------------------------
// ShiftAug's resampling (layers.py:36-59): replicate-pad by 3, then grid_sample(bilinear, zeros, align_corners=False) on
// base_grid + shift * 2/70.  The source coordinate of output index j under integer shift s is j + s only up to fp32 round-off,
// so the bilinear weights are not exactly 0 / 1: the table reproduces torch's fp32 arithmetic (torch.linspace's two-sided rule,
// the fp32 shift product, grid_sample's unnormalisation) and stores, per (s, j), the two source indices of the UNPADDED image
// (the replicate padding folded in by clamping) with their weights; a neighbour outside the padded image weighs 0 (zeros
// padding).  Rows and columns share the table (square images).
struct PixTap {
    int32_t lo, hi;  // source index of the lower / upper neighbour, clamped to [0, 63]
    float w0, w1;    // their bilinear weights: (floor + 1) - ix and ix - floor, 0 where the neighbour is outside [0, 70)
};

inline void pix_shift_table(PixTap *tab /* [PIX_SHIFTS][PIX_IN] */) {
    // torch.linspace(-1 + 1/70, 1 - 1/70, 70) in fp32: start + step * i for the first half, end - step * (n - 1 - i) after
    const float start = (float)(-1.0 + 1.0 / PIX_FULL), end = (float)(1.0 - 1.0 / PIX_FULL);
    const float step = (end - start) / (float)(PIX_FULL - 1);
    const float unit = (float)(2.0 / PIX_FULL);
    for (int s = 0; s < PIX_SHIFTS; ++s) {
        const float shift = (float)s * unit;
        for (int j = 0; j < PIX_IN; ++j) {
            float lin;
            if (j < PIX_FULL / 2) {
                const float d = step * (float)j;
                lin = start + d;
            } else {
                const float d = step * (float)(PIX_FULL - 1 - j);
                lin = end - d;
            }
            const float g = lin + shift;
            const float g1 = g + 1.0f;
            const float gs = g1 * (float)PIX_FULL;
            const float ix = (gs - 1.0f) / 2.0f;
            const float f = std::floor(ix);
            const float w1 = ix - f;
            const float w0 = (f + 1.0f) - ix;
            const int i0 = (int)f;
            auto clampi = [](int v) { return v < 0 ? 0 : v > PIX_IN - 1 ? PIX_IN - 1 : v; };
            PixTap &t = tab[s * PIX_IN + j];
            t.lo = clampi(i0 - PIX_PAD);
            t.hi = clampi(i0 + 1 - PIX_PAD);
            t.w0 = (i0 >= 0 && i0 < PIX_FULL) ? w0 : 0.f;
            t.w1 = (i0 + 1 >= 0 && i0 + 1 < PIX_FULL) ? w1 : 0.f;
        }
    }
}
// shifts outside [0, 6] are clamped (tdmpc2_plan_encode_pix)
__host__ __device__ inline int pix_clamp_shift(int s) { return s < 0 ? 0 : s > PIX_SHIFTS - 1 ? PIX_SHIFTS - 1 : s; }

// ---------------------------------------------------------------------------------------------------------------------------
// Routes.
//   SPREAD     one launch per layer; grid (pixel blocks of 64, channel groups of PIX_CO, images); activations of layers 0..2 in
//              the bind-time workspace.  Workgroups never wait for each other: the stream orders the four launches.
//   PER_IMAGE  one launch, one workgroup per image; the outputs of layers 0 and 1 in LDS (layer 2 reuses layer 0's region), so
//              the workspace is not touched.  Takes C <= 40 (LDS) and enough images to occupy the chip.
enum PixRouteKind { PIX_SPREAD = 0, PIX_PER_IMAGE = 1 };

struct PixGrid {
    int x, y, z, threads;
    size_t lds;
};
struct PixRoute {
    int kind;
    int launches;
    PixGrid g[PIX_LAYERS];  // launch i (PER_IMAGE: g[0] only)
};

// LDS of a per-image workgroup: layer 0's output + layer 1's output (fp32)
__host__ __device__ inline size_t pix_image_lds(int C) { return (size_t)C * (pix_hw(0) + pix_hw(1)) * 4; }
// offset (floats) of layer l's output inside that LDS: 0 and 2 share the first region
__host__ __device__ inline int pix_image_lds_off(int l, int C) { return l == 1 ? C * pix_hw(0) : 0; }
// workspace floats per image of the spread route: outputs of layers 0..2; offset of layer l's output
__host__ __device__ inline size_t pix_ws_floats(int C) { return (size_t)C * (pix_hw(0) + pix_hw(1) + pix_hw(2)); }
__host__ __device__ inline size_t pix_ws_off(int l, int C) {
    return l == 0 ? 0 : l == 1 ? (size_t)C * pix_hw(0) : (size_t)C * (pix_hw(0) + pix_hw(1));
}
inline size_t pix_ws_bytes(int max_envs, int C) { return (size_t)max_envs * pix_ws_floats(C) * 4; }

// The per-image route pays one CU per image for the whole stack; it only beats the spread route's four launches once there are
// images for at least half of the compute units.
inline bool pix_image_fits(int C) { return pix_image_lds(C) <= PIX_LDS_MAX; }
inline int pix_image_min_envs(int cus) { return cus / 2 > 1 ? cus / 2 : 1; }

inline PixRoute pix_route(int E, int C, int cus) {
    PixRoute r{};
    if (pix_image_fits(C) && E >= pix_image_min_envs(cus)) {
        r.kind = PIX_PER_IMAGE;
        r.launches = 1;
        r.g[0] = PixGrid{E, 1, 1, PIX_IMAGE_WG, pix_image_lds(C)};
        return r;
    }
    r.kind = PIX_SPREAD;
    r.launches = PIX_LAYERS;
    for (int l = 0; l < PIX_LAYERS; ++l) r.g[l] = PixGrid{pix_hw_pad(l) / PIX_SPREAD_WG, C / PIX_CO, E, PIX_SPREAD_WG, 0};
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Work items: one thread computes output pixel p (row-major, p < pix_hw(l)) of channels c0 .. c0 + PIX_CO - 1 of image e.
// Threads whose p runs past the layer's pixels (the wave padding) compute nothing but take part in the SimNorm shuffles of the
// last layer: eight consecutive pixels of a channel's 4 x 4 map are one SimNorm group (Flatten order c * 16 + 4y + x).
struct PixItem {
    int e, c0, p;
    bool valid;
};
__host__ __device__ inline PixItem pix_spread_item(int l, int bx, int by, int bz, int t) {
    const int p = bx * PIX_SPREAD_WG + t;
    return PixItem{bz, by * PIX_CO, p, p < pix_hw(l)};
}
// per image: items i = 0 .. pix_image_items(l, C) - 1, thread t takes i = t, t + PIX_IMAGE_WG, ...; a wave's 64 items share c0
__host__ __device__ inline int pix_image_items(int l, int C) { return C / PIX_CO * pix_hw_pad(l); }
__host__ __device__ inline PixItem pix_image_item(int l, int C, int e, int i) {
    const int p = i % pix_hw_pad(l);
    return PixItem{e, i / pix_hw_pad(l) * PIX_CO, p, p < pix_hw(l)};
}
