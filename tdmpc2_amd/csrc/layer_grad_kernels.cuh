// Kernels of the trainable layer (tdmpc2_layer_forward / tdmpc2_layer_backward): Linear -> (dropout mask) -> LayerNorm -> Mish or
// SimNorm, forward and backward, exact fp32.  Grids, tiles, offsets and summation orders: layer_grad_route.h.
//   k_lg_gemm   the three contractions on v_mfma_f32_32x32x2_f32.  Both operands of a trip (LG_KT reduction elements) are read from
//               global memory along their contiguous dimension, held in registers under the previous trip's MFMAs, and stored
//               to LDS as [l][row or column]; a lane's MFMA operand is then one bank-conflict-free LDS word.  Per output element fmaf chains
//               of LG_SEG_TRIPS trips in rising l, added in rising order, whatever the grid.
//   k_lg_row_fwd / k_lg_row_bwd   LayerNorm, activation and their backward, one wave per row; F.layer_norm's biased variance,
//               F.mish's softplus threshold 20, softmax with the group's max subtracted.
//   k_lg_cols   db, dln_w, dln_b: sums over rows in the fixed order of lg_col_part.
// No workgroup waits for another, nothing is atomic.  Included by k_layer_grad.hip.
#pragma once
#include "layer_grad_route.h"

typedef float lg_f32x16 __attribute__((ext_vector_type(16)));

struct LgGemmParams {
    LgGemm g;
    const float *A, *B;
    float *C;
    const float *bias;  // FWD: [G][N]; else null
    const float *mask;  // FWD: laid out as C, or null
};

// a trip's [LG_KT][64] tile of one operand: element (i, l) of the tile is base[i s_i + l s_l], zero outside (I, L).  LCONT: the
// operand is contiguous along l, so consecutive threads take consecutive l; otherwise consecutive i.  8 elements per thread.
template <bool LCONT>
__device__ __forceinline__ void lg_gload(const float *base, uint64_t s_i, uint64_t s_l, int i0, int I, int l0, int L, float (&reg)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int e = threadIdx.x + LG_THREADS * u;
        const int l = LCONT ? e % LG_KT : e / LG_BM, i = LCONT ? e / LG_KT : e % LG_BM;
        const bool ok = i0 + i < I && l0 + l < L;
        reg[u] = ok ? base[(uint64_t)(i0 + i) * s_i + (uint64_t)(l0 + l) * s_l] : 0.f;
    }
}
template <bool LCONT>
__device__ __forceinline__ void lg_sstore(float *tile, const float (&reg)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int e = threadIdx.x + LG_THREADS * u;
        const int l = LCONT ? e % LG_KT : e / LG_BM, i = LCONT ? e / LG_KT : e % LG_BM;
        tile[l * LG_LDS_LD + i] = reg[u];
    }
}

template <bool A_LCONT, bool B_LCONT>
__global__ __launch_bounds__(LG_THREADS) void k_lg_gemm(LgGemmParams p) {
    __shared__ float As[LG_KT * LG_LDS_LD], Bs[LG_KT * LG_LDS_LD];
    const LgGemm &g = p.g;
    const LgTile t = lg_tile(g, blockIdx.x);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = lg_wave_m(wave), wn = lg_wave_n(wave);
    const int tr = lg_trips(g.L), total = tr * g.gsum;

    lg_f32x16 acc, tot;  // the running partial chain; the partials added so far
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = tot[i] = 0.f;
    float ra[8], rb[8];
    auto gload = [&](int trip) {
        const uint64_t grp = g.gsum == 1 ? (uint64_t)t.out : (uint64_t)(trip / tr);
        const int l0 = (trip % tr) * LG_KT;
        lg_gload<A_LCONT>(p.A + grp * g.a_g, g.a_m, g.a_l, t.m0, g.M, l0, g.L, ra);
        lg_gload<B_LCONT>(p.B + grp * g.b_g, g.b_n, g.b_l, t.n0, g.Nc, l0, g.L, rb);
    };
    gload(0);
    for (int trip = 0; trip < total; ++trip) {
        __syncthreads();  // the previous trip's MFMA operands have been read
        lg_sstore<A_LCONT>(As, ra);
        lg_sstore<B_LCONT>(Bs, rb);
        __syncthreads();
        if (trip + 1 < total) gload(trip + 1);
#pragma unroll
        for (int s = 0; s < LG_KT / LG_KSTEP; ++s) {
            const int k = lg_step_k(lane, s);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[k * LG_LDS_LD + wm + (lane & 31)], Bs[k * LG_LDS_LD + wn + (lane & 31)], acc, 0, 0, 0);
        }
        if (lg_seg_end(trip) || trip + 1 == total) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                tot[i] += acc[i];
                acc[i] = 0.f;
            }
        }
    }

    const int n = t.n0 + wn + lg_acc_col(lane);
    if (n >= g.Nc) return;
    const float bias = p.bias ? p.bias[lg_off2((uint64_t)t.out, (uint64_t)n, (uint64_t)g.Nc)] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int m = t.m0 + wm + lg_acc_row(lane, i);
        if (m < g.M) {
            const uint64_t off = lg_c_off(g, (uint64_t)t.out, (uint64_t)m, (uint64_t)n);
            float v = tot[i] + bias;
            if (p.mask) v *= p.mask[off];
            p.C[off] = v;
        }
    }
}

__device__ __forceinline__ float lg_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// t = tanh(softplus(u)) (F.mish: softplus threshold 20), 1 - t^2 and sigmoid(u).  With e = exp(u), n = e (e + 2): t = n / (n + 2) and
// 1 - t = 2 / (n + 2): the same functions without tanh(log1p(.)) and without the cancellation of 1 - t * t near t = 1, which
// costs several ulp of the derivative once u passes 5.  Past the threshold softplus(u) = u and tanh(u) rounds to 1.
__device__ __forceinline__ void lg_mish_terms(float u, float &t, float &omt2, float &sg) {
    if (u > 20.f) {
        t = 1.f; omt2 = 0.f; sg = 1.f;
        return;
    }
    const float e = expf(u), n = e * (e + 2.f);
    t = n / (n + 2.f);
    omt2 = (2.f / (n + 2.f)) * (1.f + t);
    sg = e / (1.f + e);
}

struct LgRowParams {
    LgDesc d;
    const float *pre, *ln_w, *ln_b, *mask, *dy;
    const float *stat_in;  // backward
    float *stat, *y;       // forward
    float *du, *dlin;      // backward (workspace)
};

// lane l owns units l, l + 64, ... of its row; a unit is one element (Linear, Mish) or one SimNorm group
#define LG_FOR_OWNED(unit, units) for (int unit = lane; unit < (units); unit += 64)

__global__ __launch_bounds__(64 * LG_ROW_WAVES) void k_lg_row_fwd(LgRowParams p) {
    const LgDesc &d = p.d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, N = d.out_dim;
    const uint64_t row = (uint64_t)blockIdx.x * LG_ROW_WAVES + wave;
    if (row >= (uint64_t)d.groups * (uint64_t)d.rows) return;  // (no barrier below)
    const uint64_t grp = row / (uint64_t)d.rows;
    const float *pre = p.pre + row * (uint64_t)N, *lw = p.ln_w + grp * (uint64_t)N, *lb = p.ln_b + grp * (uint64_t)N;
    float *y = p.y + row * (uint64_t)N;
    const int sd = d.kind == LG_SIMNORM ? d.simnorm_dim : 1, units = N / sd;

    float s = 0.f;
    LG_FOR_OWNED(unit, units)
        for (int j = 0; j < sd; ++j) s += pre[unit * sd + j];
    const float mean = lg_wave_sum(s) / (float)N;
    s = 0.f;
    LG_FOR_OWNED(unit, units)
        for (int j = 0; j < sd; ++j) {
            const float c = pre[unit * sd + j] - mean;
            s += c * c;
        }
    const float rstd = 1.0f / sqrtf(lg_wave_sum(s) / (float)N + d.ln_eps);
    if (lane == 0) {
        p.stat[2 * row] = mean;
        p.stat[2 * row + 1] = rstd;
    }
    auto u_of = [&](int n) { return (pre[n] - mean) * rstd * lw[n] + lb[n]; };
    if (d.kind == LG_MISH) {
        LG_FOR_OWNED(n, units) {
            float t, omt2, sg;
            const float u = u_of(n);
            lg_mish_terms(u, t, omt2, sg);
            y[n] = u * t;
        }
    } else {
        LG_FOR_OWNED(unit, units) {
            const int n0 = unit * sd;
            float mx = -INFINITY, sum = 0.f;
            for (int j = 0; j < sd; ++j) mx = fmaxf(mx, u_of(n0 + j));
            for (int j = 0; j < sd; ++j) sum += expf(u_of(n0 + j) - mx);
            for (int j = 0; j < sd; ++j) y[n0 + j] = expf(u_of(n0 + j) - mx) / sum;
        }
    }
}

// dy -> du (kept in the workspace for the column sums) -> dlin = dpre * mask.  Linear with a mask: dlin = dy * mask only.
__global__ __launch_bounds__(64 * LG_ROW_WAVES) void k_lg_row_bwd(LgRowParams p) {
    const LgDesc &d = p.d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, N = d.out_dim;
    const uint64_t row = (uint64_t)blockIdx.x * LG_ROW_WAVES + wave;
    if (row >= (uint64_t)d.groups * (uint64_t)d.rows) return;  // (no barrier below)
    const uint64_t grp = row / (uint64_t)d.rows, base = row * (uint64_t)N;
    const float *dy = p.dy + base, *mask = p.mask ? p.mask + base : nullptr;
    float *dlin = p.dlin + base;
    if (d.kind == LG_LINEAR) {
        LG_FOR_OWNED(n, N) dlin[n] = dy[n] * mask[n];
        return;
    }
    const float *pre = p.pre + base, *lw = p.ln_w + grp * (uint64_t)N, *lb = p.ln_b + grp * (uint64_t)N;
    float *du = p.du + base;
    const float mean = p.stat_in[2 * row], rstd = p.stat_in[2 * row + 1];
    const int sd = d.kind == LG_SIMNORM ? d.simnorm_dim : 1, units = N / sd;
    auto xh_of = [&](int n) { return (pre[n] - mean) * rstd; };
    auto u_of = [&](int n) { return xh_of(n) * lw[n] + lb[n]; };

    float s1 = 0.f, s2 = 0.f;  // sum dxh, sum dxh xh
    if (d.kind == LG_MISH) {
        LG_FOR_OWNED(n, units) {
            float t, omt2, sg;
            const float u = u_of(n);
            lg_mish_terms(u, t, omt2, sg);
            const float g = dy[n] * (t + u * sg * omt2);
            du[n] = g;
            const float dxh = g * lw[n];
            s1 += dxh;
            s2 += dxh * xh_of(n);
        }
    } else {
        LG_FOR_OWNED(unit, units) {
            const int n0 = unit * sd;
            float mx = -INFINITY, sum = 0.f, dot = 0.f;
            for (int j = 0; j < sd; ++j) mx = fmaxf(mx, u_of(n0 + j));
            for (int j = 0; j < sd; ++j) sum += expf(u_of(n0 + j) - mx);
            for (int j = 0; j < sd; ++j) dot += dy[n0 + j] * (expf(u_of(n0 + j) - mx) / sum);
            for (int j = 0; j < sd; ++j) {
                const int n = n0 + j;
                const float yv = expf(u_of(n) - mx) / sum, g = yv * (dy[n] - dot);
                du[n] = g;
                const float dxh = g * lw[n];
                s1 += dxh;
                s2 += dxh * xh_of(n);
            }
        }
    }
    s1 = lg_wave_sum(s1) / (float)N;
    s2 = lg_wave_sum(s2) / (float)N;
    // every lane reads back only the du it wrote itself
    LG_FOR_OWNED(unit, units)
        for (int j = 0; j < sd; ++j) {
            const int n = unit * sd + j;
            const float dpre = rstd * (du[n] * lw[n] - s1 - xh_of(n) * s2);
            dlin[n] = mask ? dpre * mask[n] : dpre;
        }
}

struct LgColParams {
    LgDesc d;
    const float *dlin, *du, *pre, *stat;  // du / pre / stat: null for Linear
    float *db, *dln_w, *dln_b;
};

__global__ __launch_bounds__(LG_COLS * LG_PARTS) void k_lg_cols(LgColParams p) {
    __shared__ float part[3][LG_PARTS][LG_COLS];
    const LgDesc &d = p.d;
    const int c = threadIdx.x % LG_COLS, pt = threadIdx.x / LG_COLS;
    const int tiles = lg_col_tiles(d);
    const uint64_t grp = blockIdx.x / tiles, R = (uint64_t)d.rows, N = (uint64_t)d.out_dim;
    const int n = (blockIdx.x % tiles) * LG_COLS + c;
    const bool ok = n < d.out_dim, ln = d.kind != LG_LINEAR;
    float sb = 0.f, sw = 0.f, sbeta = 0.f;
    if (ok)
        for (int r = pt; r < d.rows; r += LG_PARTS) {  // lg_col_part(r) == pt
            const uint64_t off = lg_off3(grp, (uint64_t)r, (uint64_t)n, R, N), srow = 2 * (grp * R + (uint64_t)r);
            sb += p.dlin[off];
            if (ln) {
                const float g = p.du[off], xh = (p.pre[off] - p.stat[srow]) * p.stat[srow + 1];
                sw += g * xh;
                sbeta += g;
            }
        }
    part[0][pt][c] = sb;
    part[1][pt][c] = sw;
    part[2][pt][c] = sbeta;
    __syncthreads();
    if (pt == 0 && ok) {
        float a = 0.f, b = 0.f, e = 0.f;
        for (int q = 0; q < LG_PARTS; ++q) {
            a += part[0][q][c];
            b += part[1][q][c];
            e += part[2][q][c];
        }
        const uint64_t o = lg_off2(grp, (uint64_t)n, N);
        p.db[o] = a;
        if (ln) {
            p.dln_w[o] = b;
            p.dln_b[o] = e;
        }
    }
}
