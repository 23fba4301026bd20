// Pixel encoder in training: the kernels of the backward (tdmpc2_pixgrad_backward) and the forward's re-pack.  Exact fp32 on
// v_mfma_f32_32x32x2_f32: every sum is an fmaf chain whose order pixel_grad_route.h states.  The views (DW, DA), tiles, chunks,
// folds and workspace offsets are that header's; layer 0's input is staged by the forward's own pixb_stage0.
//   k_pg_pack   W_l [C][cin_l][k][k] -> [cin_l][k][k][C] for the four layers, one launch
//   k_pg_seed   dy_3 = z (dz - sum_group dz z), or a copy of dz when the seed is layer 3's pre-activation gradient
//   k_pg_da     dy_{l-1} = (a_{l-1} > 0) * transposed convolution of dy_l with W_l
//   k_pg_dw     the partial [taps + 1][C] of one chunk of rows: dW_l and, from a row of ones, db_l
//   k_pg_fold   the partials of an element added in the fixed order, into the Conv2d layout
// No workgroup waits for another; the stream orders the launches.  Included by k_pixel_grad.hip.
#pragma once
#include "pixel_batch_kernels.cuh"
#include "pixel_grad_route.h"

struct PgParams {
    PixbParams fw;               // obs, cin, C, n, shift, tab: what layer 0's staging reads (wp, bias, ws, z unused here)
    const float *W[PIX_LAYERS];  // the Conv2d tensors [C][cin_l][k][k], read where they are
    const float *acts;           // [n][pix_ws_floats(C)]
    const float *z, *dz;         // [n][16 C]
    float *dy[PIX_LAYERS];       // [n][C][pix_hw(l)]
    float *part;
    float *dW[PIX_LAYERS], *db[PIX_LAYERS];
    int seed_is_preact;
};

struct PgPackParams {
    const float *W[PIX_LAYERS];
    float *wp[PIX_LAYERS];
    int cin, C;
};

__global__ __launch_bounds__(PG_ROW_THREADS) void k_pg_pack(PgPackParams p) {
    const int i0 = blockIdx.x * PG_ROW_THREADS + threadIdx.x, stride = gridDim.x * PG_ROW_THREADS;
    for (int l = 0; l < PIX_LAYERS; ++l) {
        const int rows = pixb_k(l, pixb_cin(l, p.cin, p.C)), total = rows * p.C;  // rows: ci k k + tap
        for (int i = i0; i < total; i += stride) {
            const int co = i % p.C, r = i / p.C;
            p.wp[l][i] = p.W[l][(size_t)co * rows + r];
        }
    }
}

__global__ __launch_bounds__(PG_ROW_THREADS) void k_pg_seed(PgParams p, size_t total) {
    const size_t i = (size_t)blockIdx.x * PG_ROW_THREADS + threadIdx.x;
    if (i >= total) return;
    if (p.seed_is_preact) {
        p.dy[3][i] = p.dz[i];
        return;
    }
    const size_t g = i & ~(size_t)7;  // a SimNorm group: eight consecutive features c 16 + 4 y + x
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s = fmaf(p.dz[g + j], p.z[g + j], s);
    p.dy[3][i] = p.z[i] * (p.dz[i] - s);
}

template <int L>
__global__ __launch_bounds__(PIXB_THREADS) void k_pg_da(PgParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pg_smem[];
    constexpr int KS = pix_kernel(L), KK = KS * KS, S = pix_stride(L), O = pix_out(L), HWO = pix_hw(L), SIDE = pix_side(L), HWI = SIDE * SIDE;
    const int C = p.fw.C, K = pg_da_k(L, C);
    int4 *ktab = reinterpret_cast<int4 *>(pg_smem);  // per kk <= K: (A offset of co, B offset at ci = 0 or -1: padding, ky, kx)
    for (int k = threadIdx.x; k <= K; k += PIXB_THREADS) {
        const PgDaK t = pg_da_decode(L, k);
        ktab[k] = k < K ? make_int4(t.co * HWO, pg_da_w_off(L, C, k, 0), t.ky, t.kx) : make_int4(0, -1, 0, 0);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    const PixbItem it = pg_da_item(L, p.fw.n, blockIdx.x, wave);
    if (it.rows == 0) return;
    const int lr = (lane & 31) < it.rows ? (lane & 31) : it.rows - 1;
    const long q = it.row0 + lr;
    const int e = (int)(q / HWI), px = (int)(q % HWI), y = px / SIDE, x = px % SIDE;
    const float *dyb = p.dy[L] + (size_t)e * C * HWO;
    const int steps = pg_da_steps(L, C);
    const size_t wsf = pix_ws_floats(C), aoff = pix_ws_off(L - 1, C);

    for (int ct = 0; ct < pixb_col_tiles(C); ++ct) {
        const int col = ct * PIXB_TILE + pixb_acc_col(lane);
        const bool cok = col < C;
        const float *wcol = p.W[L] + (cok ? col * KK : 0);
        pixb_f32x16 acc, tot;
#pragma unroll
        for (int i = 0; i < PIXB_ACC; ++i) acc[i] = tot[i] = 0.f;
        for (int s = 0; s < steps; ++s) {
            const int4 t = ktab[PIXB_KSTEP * s + half];
            const bool kok = t.y >= 0;
            const int ty = y - t.z, tx = x - t.w;
            const bool ok = kok && ty >= 0 && tx >= 0 && ty % S == 0 && tx % S == 0 && ty / S < O && tx / S < O;
            const float g = dyb[ok ? t.x + (ty / S) * O + tx / S : 0], w = wcol[kok ? t.y : 0];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ok ? g : 0.f, kok && cok ? w : 0.f, acc, 0, 0, 0);
            if ((s + 1) % PG_DA_SEG == 0) {
                tot += acc;
#pragma unroll
                for (int i = 0; i < PIXB_ACC; ++i) acc[i] = 0.f;
            }
        }
        if (steps % PG_DA_SEG != 0) tot += acc;
#pragma unroll
        for (int i = 0; i < PIXB_ACC; ++i) {
            const int tr = pixb_acc_row(lane, i);
            if (cok && tr < it.rows) {
                const long qq = it.row0 + tr;
                const size_t img = (size_t)(qq / HWI);
                const int pp = (int)(qq % HWI);
                const float a = p.acts[img * wsf + aoff + (size_t)col * HWI + pp];
                p.dy[L - 1][pg_dy_elem(L - 1, C, img, col, pp)] = a > 0.f ? tot[i] : 0.f;
            }
        }
    }
}

template <int L, bool U8>
__global__ __launch_bounds__(PIXB_THREADS) void k_pg_dw(PgParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pg_smem[];
    constexpr int HW = pix_hw(L);
    int2 *rowtab = reinterpret_cast<int2 *>(pg_smem);  // per row of the chunk: (A offset, B offset) relative to the chunk's first image
    float *patch = reinterpret_cast<float *>(pg_smem + (size_t)PG_CHUNK * sizeof(int2));
    const int C = p.fw.C, M = pg_dw_m(L, p.fw.cin, C), K = M - 1;
    const long chunk = blockIdx.x, r0 = chunk * PG_CHUNK;
    const int rows = pg_chunk_rows(L, p.fw.n, chunk);
    const int e0 = pixb_row_image(L, r0);
    PixbStage sg{};
    if (L == 0) {
        sg = pixb_l0_stage(r0, r0 + rows - 1);
        pixb_stage0<U8>(p.fw, sg, patch);
    }
    for (int i = threadIdx.x; i < PG_CHUNK; i += PIXB_THREADS) {
        const long r = r0 + (i < rows ? i : rows - 1);  // rows past the chunk's end name its last row; their terms are zeroed below
        rowtab[i] = make_int2(pg_row_a(L, C, sg, e0, r), pg_row_b(L, C, e0, r));
    }
    __syncthreads();
    const float *A = L == 0 ? patch : p.acts + (size_t)e0 * pix_ws_floats(C);
    const float *B = p.dy[L] + (size_t)e0 * C * HW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    const int ctiles = pixb_col_tiles(C), tiles = pg_dw_tap_tiles(M) * ctiles, steps = (rows + 1) / 2;

    for (int t = blockIdx.y * PIXB_WAVES + wave; t < tiles; t += PIXB_WAVES * gridDim.y) {
        const int tt = t / ctiles, ct = t % ctiles;
        const int m = tt * PIXB_TILE + (lane & 31);
        const bool tok = m < K, one = m == K;
        const int toff = tok ? pg_a_off(L, pg_tap(L, m)) : 0;
        const int col = ct * PIXB_TILE + pixb_acc_col(lane);
        const bool cok = col < C;
        const int boff = cok ? col * HW : 0;
        pixb_f32x16 acc, tot;
#pragma unroll
        for (int i = 0; i < PIXB_ACC; ++i) acc[i] = tot[i] = 0.f;
        for (int s = 0; s < steps; ++s) {
            const int i = PIXB_KSTEP * s + half;
            const bool v = i < rows;
            const int2 rt = rowtab[i];
            const float x = A[rt.x + toff], g = B[rt.y + boff];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v ? (tok ? x : one ? 1.f : 0.f) : 0.f, v && cok ? g : 0.f, acc, 0, 0, 0);
            if ((s + 1) % (PG_SUB / PIXB_KSTEP) == 0) {  // a sub-chain ends: into the chunk's partial
                tot += acc;
#pragma unroll
                for (int i = 0; i < PIXB_ACC; ++i) acc[i] = 0.f;
            }
        }
        if (steps % (PG_SUB / PIXB_KSTEP) != 0) tot += acc;
#pragma unroll
        for (int i = 0; i < PIXB_ACC; ++i) {
            const int mr = tt * PIXB_TILE + pixb_acc_row(lane, i);
            if (cok && mr < M) p.part[pg_part_off(M, C, chunk, mr, col)] = tot[i];
        }
    }
}

__global__ __launch_bounds__(PG_FOLD_THREADS) void k_pg_fold(const float *part, long chunks, int M, int C, float *dW, float *db) {
    const int i = blockIdx.x * PG_FOLD_THREADS + threadIdx.x, MC = M * C;
    if (i >= MC) return;
    const int m = i / C, co = i % C, K = M - 1;
    float total = 0.f;
    for (long g0 = 0; g0 < chunks; g0 += PG_FOLD) {
        const long g1 = g0 + PG_FOLD < chunks ? g0 + PG_FOLD : chunks;
        float s = 0.f;
        for (long j = g0; j < g1; ++j) s += part[(size_t)j * MC + i];
        total += s;
    }
    if (m < K) dW[(size_t)co * K + m] = total;
    else db[co] = total;
}
