// Pixel encoder, batch route: the four convolutions of pixel_kernels.cuh as exact-fp32 implicit GEMMs on
// v_mfma_f32_32x32x2_f32 (an fmaf chain per output element, as the scalar routes compute it), for training batches of any
// size.  The GEMM view, the tiles, the k order, layer 0's staging and the passes over the workspace: pixel_batch_route.h.
//   A   layer 0: ShiftAug + x / 255 - 0.5 evaluated once per input element of the workgroup's patch into LDS (the tap table and the
//       fp32 terms of pix_conv0, blended as one fmaf chain), fragments read from there; layers 1..3: the previous layer's output in the workspace
//       ([image][C][hw], the spread route's layout)
//   B   the bound weights [cin][ky][kx][C] where k_pix_pack left them: row k is one 128-byte line per column tile
//   D   bias add and ReLU into the workspace (layers 0..2); bias add and SimNorm(8) into z (layer 3): a group's eight pixels
//       are four registers of lanes c and c + 32, one exchange per group
// One launch per layer, ordered by the stream; no workgroup waits for another.  Included by k_pixel_batch.hip.
#pragma once
#include "pixel_batch_route.h"

typedef float pixb_f32x16 __attribute__((ext_vector_type(16)));

// layer 0: the workgroup's resampled, preprocessed patch[ci][slot][64]
template <bool U8>
__device__ __forceinline__ void pixb_stage0(const PixbParams &p, const PixbStage sg, float *patch) {
    const int nslots = sg.nA + sg.nB, total = nslots * p.cin * PIX_IN;
    const size_t plane = (size_t)PIX_IN * PIX_IN, esz = U8 ? 1 : 4;
    for (int i = threadIdx.x; i < total; i += PIXB_THREADS) {
        const int x = i % PIX_IN, t = i / PIX_IN, slot = t % nslots, ci = t / nslots;
        const int e = slot < sg.nA ? sg.eA : sg.eA + 1, y = slot < sg.nA ? sg.yA0 + slot : slot - sg.nA;
        const int dx = pix_clamp_shift(p.shift[2 * e]), dy = pix_clamp_shift(p.shift[2 * e + 1]);
        const PixTap r = p.tab[dy * PIX_IN + y], c = p.tab[dx * PIX_IN + x];
        // grid_sample's bilinear weights (nw, ne, sw, se) and source offsets: pix_conv0's expression
        const float wnw = c.w0 * r.w0, wne = c.w1 * r.w0, wsw = c.w0 * r.w1, wse = c.w1 * r.w1;
        const int onw = r.lo * PIX_IN + c.lo, one = r.lo * PIX_IN + c.hi, osw = r.hi * PIX_IN + c.lo, ose = r.hi * PIX_IN + c.hi;
        const char *pl = static_cast<const char *>(p.obs) + ((size_t)e * p.cin + ci) * plane * esz;
        // pix_conv0's terms in pix_conv0's order (nw, ne, sw, se), but as ONE explicit fmaf chain.  pix_conv0 writes `v += px * w` and
        // leaves the fusing to the compiler, which fuses all four terms in some copies of its unrolled kx loop and rounds two or four
        // products on their own in the others: there an element's value depends on the tap that reads it, which a patch
        // evaluated once per element cannot repeat.  Here the value is the same whichever trip stages it.
        float q[4];
        if (U8) {
            const uint8_t *s = reinterpret_cast<const uint8_t *>(pl);
            q[0] = (float)s[onw]; q[1] = (float)s[one]; q[2] = (float)s[osw]; q[3] = (float)s[ose];
        } else {
            const float *s = reinterpret_cast<const float *>(pl);
            q[0] = s[onw]; q[1] = s[one]; q[2] = s[osw]; q[3] = s[ose];
        }
        const float v = fmaf(q[3], wse, fmaf(q[2], wsw, fmaf(q[1], wne, fmaf(q[0], wnw, 0.f))));
        patch[pixb_l0_patch_off(ci, slot, x)] = v / 255.0f - 0.5f;
    }
}

template <int L, bool U8>
__global__ __launch_bounds__(PIXB_THREADS) void k_pixb(PixbParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pixb_smem[];
    constexpr int HW = pix_hw(L);
    const int C = p.C, cin_l = pixb_cin(L, p.cin, C);
    const int K = pixb_k(L, cin_l), KP = pixb_k_pad(L, cin_l), KG = KP / (PIXB_KSTEP * PIXB_KGROUP);
    int2 *ktab = reinterpret_cast<int2 *>(pixb_smem);  // per padded k: (A offset, B offset); B offset -1 = padding step
    float *patch = reinterpret_cast<float *>(pixb_smem + (size_t)KP * sizeof(int2));
    for (int k = threadIdx.x; k < KP; k += PIXB_THREADS)
        ktab[k] = k < K ? make_int2(pixb_a_off(L, cin_l, k), pixb_w_off(L, cin_l, C, k)) : make_int2(0, -1);

    const long nrows = pixb_rows(L, p.n);
    const long wg0 = (long)blockIdx.x * PIXB_WG_ROWS;
    const long wg1 = (wg0 + PIXB_WG_ROWS < nrows ? wg0 + PIXB_WG_ROWS : nrows) - 1;
    PixbStage sg{};
    if (L == 0) {
        sg = pixb_l0_stage(wg0, wg1);
        pixb_stage0<U8>(p, sg, patch);
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    const PixbItem it = pixb_item(L, p.n, blockIdx.x, wave);
    if (it.rows == 0) return;  // (no barrier and no cross-wave exchange below)
    // the row whose A elements this lane loads; lanes past the tile's valid rows load the last valid row (never stored)
    const int lr = (lane & 31) < it.rows ? (lane & 31) : it.rows - 1;
    const long r = it.row0 + lr;
    const int e = pixb_row_image(L, r), px = pixb_row_pixel(L, r);
    const float *A;
    if (L == 0) {
        const int oy = px / pix_out(0), ox = px % pix_out(0);
        A = patch + pixb_l0_patch_off(0, pixb_l0_slot(sg, e, pix_stride(0) * oy), pix_stride(0) * ox);
    } else {
        A = p.ws + (size_t)e * pix_ws_floats(C) + pix_ws_off(L - 1, C) + pixb_a_base(L, px);
    }
    const size_t wsf = pix_ws_floats(C), woff = L < PIX_LAYERS - 1 ? pix_ws_off(L, C) : 0;

    for (int ct = 0; ct < pixb_col_tiles(C); ++ct) {
        const int col = ct * PIXB_TILE + pixb_acc_col(lane);
        const bool cok = col < C;
        const float *wcol = p.wp[L] + (cok ? col : 0);
        pixb_f32x16 acc;
#pragma unroll
        for (int i = 0; i < PIXB_ACC; ++i) acc[i] = 0.f;
        // PIXB_KGROUP steps per trip, the next trip's operands loaded under this trip's MFMAs (the table is padded to whole trips)
        float av[PIXB_KGROUP], bv[PIXB_KGROUP];
        auto load = [&](int g, float *a, float *b) {
#pragma unroll
            for (int u = 0; u < PIXB_KGROUP; ++u) {
                const int2 t = ktab[PIXB_KSTEP * (PIXB_KGROUP * g + u) + half];
                const bool kok = t.y >= 0;
                const float x = A[t.x], w = wcol[kok ? t.y : 0];
                a[u] = kok ? x : 0.f;
                b[u] = kok && cok ? w : 0.f;
            }
        };
        load(0, av, bv);
        for (int g = 0; g < KG; ++g) {
            float an[PIXB_KGROUP], bn[PIXB_KGROUP];
            load(g + 1 < KG ? g + 1 : g, an, bn);
#pragma unroll
            for (int u = 0; u < PIXB_KGROUP; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
#pragma unroll
            for (int u = 0; u < PIXB_KGROUP; ++u) { av[u] = an[u]; bv[u] = bn[u]; }
        }
        const float bias = cok ? p.bias[L][col] : 0.f;
        if (L < PIX_LAYERS - 1) {
#pragma unroll
            for (int i = 0; i < PIXB_ACC; ++i) {
                const int tr = pixb_acc_row(lane, i);
                if (cok && tr < it.rows) {
                    const long rr = it.row0 + tr;
                    p.ws[(size_t)pixb_row_image(L, rr) * wsf + woff + (size_t)col * HW + pixb_row_pixel(L, rr)] = fmaxf(acc[i] + bias, 0.f);
                }
            }
        } else {
            // Flatten: feature c * 16 + pixel; SimNorm group g of the tile = rows 8 g .. 8 g + 7 = registers 4 g .. 4 g + 3 here
            // and in lane ^ 32.  Sums in k_pix_spread's order: pairs, quads, the two quads.
#pragma unroll
            for (int g = 0; g < PIXB_ACC / 4; ++g) {
                float y[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] = acc[4 * g + j] + bias;
                float mx = fmaxf(fmaxf(y[0], y[1]), fmaxf(y[2], y[3]));
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                float ex[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) ex[j] = expf(y[j] - mx);
                float sum = (ex[0] + ex[1]) + (ex[2] + ex[3]);
                sum += __shfl_xor(sum, 32);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int tr = pixb_acc_row(lane, 4 * g + j);
                    if (cok && tr < it.rows) {
                        const long rr = it.row0 + tr;
                        p.z[(size_t)pixb_row_image(L, rr) * HW * C + (size_t)col * HW + pixb_row_pixel(L, rr)] = ex[j] / sum;
                    }
                }
            }
        }
    }
}
