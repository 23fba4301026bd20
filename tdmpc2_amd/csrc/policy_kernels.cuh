// Policy prior (WorldModel.pi, tdmpc2/common/world_model.py:144-184; common/math.py:12-29) row by row, plain fp32 FMAs like
// encoder_kernels.cuh: _pi = NormedLinear(Mish) -> NormedLinear(Mish) -> Linear(2A), mean, log_std = chunk(2), then the Gaussian
// head (log_std squash, masking, log-probability, reparameterised sample, tanh squash, entropies).  Weights are the fp32 [in][out]
// copies of tdmpc2_plan_bind_policy (and, when acting, the encoder's transposed copies of tdmpc2_plan_bind_encoder).
// Routes and work items: policy_route.h.  No workgroup waits for another one.
// Included by k_policy.hip inside its anonymous namespace.
#pragma once

__device__ __forceinline__ float pol_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float pol_block_sum(float v, float *red) {
    // all threads get the sum over the workgroup (the encoder's enc_block_sum)
    v = pol_wave_sum(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();  // `red` may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < POL_THREADS / 64; ++w) s += red[w];
    return s;
}

// The Gaussian head of one row on one wave (lane = action dimension), in the reference's order of operations:
//   log_std = min + 0.5 dif (tanh(x) + 1); masked mean / log_std / eps; log_prob = sum(-0.5 eps^2 - log_std - log(2 pi)/2);
//   scaled = log_prob * (A | action_dims); action = mean + eps exp(log_std); tanh; log_prob -= sum log(relu(1 - a^2) + 1e-6);
//   entropy = -log_prob; scaled_entropy = -log_prob * scaled / (log_prob + 1e-8).
// __fmul_rn / __fadd_rn keep the products and sums the reference rounds separately from being contracted into FMAs.
__device__ __forceinline__ void pol_head(const float *y /* [2A] */, int e, const PolHeadArgs &p) {
    const int lane = threadIdx.x & 63, A = p.A;
    const PolItem it = pol_head_item(e, lane, A);
    const bool on = it.valid;
    const size_t ra = (size_t)e * A + lane;
    float mu = on ? y[lane] : 0.f;
    const float lr = on ? y[A + lane] : 0.f;
    float ls = __fadd_rn(p.lmin, __fmul_rn(__fmul_rn(0.5f, p.ldif), __fadd_rn(tanhf(lr), 1.f)));
    float eps = 0.f;
    if (on) eps = p.eps ? p.eps[ra] : rng_normal(p.seed, p.call, SITE_POLICY, 0, p.row0 + e, (unsigned)lane);
    if (on && p.eps_out) p.eps_out[ra] = eps;
    float size = (float)A;
    if (p.mask) {
        const float m = on ? p.mask[ra] : 0.f;
        mu = __fmul_rn(mu, m);
        ls = __fmul_rn(ls, m);
        eps = __fmul_rn(eps, m);
        size = pol_wave_sum(m);
    }
    const float res = __fsub_rn(__fmul_rn(-0.5f, __fmul_rn(eps, eps)), ls);
    float lp = pol_wave_sum(on ? __fsub_rn(res, 0.9189385175704956f) : 0.f);
    const float slp = __fmul_rn(lp, size);
    const float act = tanhf(__fadd_rn(mu, __fmul_rn(eps, expf(ls))));
    const float mt = tanhf(mu);
    const float sq = on ? logf(__fadd_rn(fmaxf(__fsub_rn(1.f, __fmul_rn(act, act)), 0.f), 1e-6f)) : 0.f;
    lp = __fsub_rn(lp, pol_wave_sum(sq));
    if (on) {
        p.action[ra] = p.eval_mode ? mt : act;
        if (p.mean) p.mean[ra] = mt;
        if (p.log_std) p.log_std[ra] = ls;
    }
    if (lane == 0) {
        if (p.entropy) p.entropy[e] = -lp;
        if (p.scaled_entropy) p.scaled_entropy[e] = __fmul_rn(-lp, __fdiv_rn(slp, __fadd_rn(lp, 1e-8f)));
    }
}

// One dense layer of a row held in LDS (x -> y), thread = output feature(s).  kind 0: LayerNorm + Mish; 1: LayerNorm + SimNorm
// (the encoder's last layer); 2: plain Linear (the policy's output layer).
__device__ __forceinline__ void pol_layer(const PolLayerDev &ly, const float *xa, float *xb, float *red, int kind, int simnorm_dim) {
    const int tid = threadIdx.x;
    float y[POL_MAX_PER_THREAD];
    float part = 0.f;
#pragma unroll
    for (int u = 0; u < POL_MAX_PER_THREAD; ++u) {
        const PolItem it = pol_row_item(blockIdx.x, tid, u, ly.out);
        y[u] = 0.f;
        if (it.valid) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;  // four chains: the loads of different k are independent
            const float *w = ly.wt + it.f;
            int k = 0;
            for (; k + 16 <= ly.in; k += 16) {  // sixteen loads in flight per wave (one CU streams the whole chain), then the FMAs
                float wk[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) wk[j] = w[(size_t)(k + j) * ly.out];
#pragma unroll
                for (int j = 0; j < 16; j += 4) {
                    a0 = fmaf(xa[k + j], wk[j], a0);
                    a1 = fmaf(xa[k + j + 1], wk[j + 1], a1);
                    a2 = fmaf(xa[k + j + 2], wk[j + 2], a2);
                    a3 = fmaf(xa[k + j + 3], wk[j + 3], a3);
                }
            }
            for (; k + 4 <= ly.in; k += 4) {
                a0 = fmaf(xa[k], w[(size_t)k * ly.out], a0);
                a1 = fmaf(xa[k + 1], w[(size_t)(k + 1) * ly.out], a1);
                a2 = fmaf(xa[k + 2], w[(size_t)(k + 2) * ly.out], a2);
                a3 = fmaf(xa[k + 3], w[(size_t)(k + 3) * ly.out], a3);
            }
            for (; k < ly.in; ++k) a0 = fmaf(xa[k], w[(size_t)k * ly.out], a0);
            y[u] = ((a0 + a1) + (a2 + a3)) + ly.bias[it.f];
            part += y[u];
        }
    }
    if (kind == 2) {
#pragma unroll
        for (int u = 0; u < POL_MAX_PER_THREAD; ++u) {
            const PolItem it = pol_row_item(blockIdx.x, tid, u, ly.out);
            if (it.valid) xb[it.f] = y[u];
        }
        return;
    }
    const float mean = pol_block_sum(part, red) / (float)ly.out;
    part = 0.f;
#pragma unroll
    for (int u = 0; u < POL_MAX_PER_THREAD; ++u) {
        if (pol_row_item(blockIdx.x, tid, u, ly.out).valid) {
            const float d = y[u] - mean;
            part = fmaf(d, d, part);
        }
    }
    const float rstd = 1.0f / sqrtf(pol_block_sum(part, red) / (float)ly.out + LN_EPS);
#pragma unroll
    for (int u = 0; u < POL_MAX_PER_THREAD; ++u) {
        const PolItem it = pol_row_item(blockIdx.x, tid, u, ly.out);
        const float v = it.valid ? (y[u] - mean) * rstd * ly.g[it.f] + ly.b[it.f] : -INFINITY;
        if (kind == 0) {
            if (it.valid) {  // Mish (layers.py:103)
                const float ex = expf(fminf(v, 20.f));
                const float n = ex * (ex + 2.f);
                xb[it.f] = v * (n / (n + 2.f));
            }
        } else {
            // SimNorm (layers.py:74-91): softmax over groups of simnorm_dim consecutive features = adjacent lanes
            float mx = v;
            for (int o = 1; o < simnorm_dim; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            const float ex = it.valid ? expf(v - mx) : 0.f;
            float s = ex;
            for (int o = 1; o < simnorm_dim; o <<= 1) s += __shfl_xor(s, o);
            if (it.valid) xb[it.f] = ex / s;
        }
    }
}

// Row route: one workgroup per row, one launch for the whole chain -- [encoder layers ->] z | task_emb -> _pi -> head.
__global__ __launch_bounds__(POL_THREADS) void k_pol_row(PolRowParams p) {
    extern __shared__ float pol_lds[];
    float *xa = pol_lds, *xb = pol_lds + p.maxw, *red = pol_lds + 2 * p.maxw;
    const int e = blockIdx.x, tid = threadIdx.x;
    if (p.enc_nl > 0) {
        for (int i = tid; i < p.obs_dim; i += POL_THREADS) xa[i] = p.obs[(size_t)e * p.obs_dim + i];
        for (int i = tid; i < p.T; i += POL_THREADS) xa[p.obs_dim + i] = p.task_emb[(size_t)e * p.T + i];
        __syncthreads();
        for (int l = 0; l < p.enc_nl; ++l) {
            pol_layer(p.enc[l], xa, xb, red, l == p.enc_nl - 1 ? 1 : 0, p.simnorm_dim);
            __syncthreads();
            float *t = xa; xa = xb; xb = t;
        }
    } else {
        for (int i = tid; i < p.L; i += POL_THREADS) xa[i] = p.z[(size_t)e * p.L + i];
    }
    for (int i = tid; i < p.T; i += POL_THREADS) xa[p.L + i] = p.task_emb[(size_t)e * p.T + i];
    __syncthreads();
    for (int l = 0; l < 3; ++l) {
        pol_layer(p.pi[l], xa, xb, red, l < 2 ? 0 : 2, p.simnorm_dim);
        __syncthreads();
        float *t = xa; xa = xb; xb = t;
    }
    if (tid < 64) pol_head(xa, e, p.head);
}

// Spread route, one layer: workgroup (bx, by) computes features bx * 64 .. + 63 of rows by * R .. + R - 1; the eight waves split
// the contraction, every weight element is read once per R rows.  Layer 0 assembles z | task_emb itself.
template <int R>
__global__ __launch_bounds__(POL_GEMV_THREADS) void k_pol_gemv(PolGemvParams p) {
    extern __shared__ float pol_lds[];
    float *xs = pol_lds, *part = pol_lds + R * p.in;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.y * R, f = blockIdx.x * POL_GEMV_COLS + lane;
    for (int i = tid; i < R * p.in; i += POL_GEMV_THREADS) {
        const int r = i / p.in, k = i - r * p.in, row = r0 + r;
        float v = 0.f;
        if (row < p.n) v = p.x ? p.x[(size_t)row * p.ldx + k] : k < p.L ? p.z[(size_t)row * p.L + k] : p.emb[(size_t)row * p.T + (k - p.L)];
        xs[i] = v;
    }
    __syncthreads();
    const int kq = (p.in + POL_GEMV_WAVES - 1) / POL_GEMV_WAVES, k0 = min(p.in, wave * kq), k1 = min(p.in, k0 + kq);
    float a[R], b[R];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = b[r] = 0.f;
    if (f < p.out) {
        const float *w = p.wt + f;
        int k = k0;
        for (; k + 8 <= k1; k += 8) {  // eight loads in flight per wave, then the FMAs (same chains as below)
            float wk[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) wk[j] = w[(size_t)(k + j) * p.out];
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    a[r] = fmaf(xs[r * p.in + k + j], wk[j], a[r]);
                    b[r] = fmaf(xs[r * p.in + k + j + 1], wk[j + 1], b[r]);
                }
            }
        }
        for (; k + 2 <= k1; k += 2) {
            const float w0 = w[(size_t)k * p.out], w1 = w[(size_t)(k + 1) * p.out];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                a[r] = fmaf(xs[r * p.in + k], w0, a[r]);
                b[r] = fmaf(xs[r * p.in + k + 1], w1, b[r]);
            }
        }
        if (k < k1) {
            const float w0 = w[(size_t)k * p.out];
#pragma unroll
            for (int r = 0; r < R; ++r) a[r] = fmaf(xs[r * p.in + k], w0, a[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) part[(wave * R + r) * POL_GEMV_COLS + lane] = a[r] + b[r];
    __syncthreads();
    const PolItem it = pol_gemv_item(blockIdx.x, blockIdx.y, R, tid, p.n, p.out);
    if (it.valid) {
        const int r = tid / POL_GEMV_COLS;
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < POL_GEMV_WAVES; ++w) s += part[(w * R + r) * POL_GEMV_COLS + lane];
        p.y[(size_t)it.row * p.out + it.f] = s + p.bias[it.f];
    }
}

// Spread route, head: one wave per row on the output layer's pre-activations [n, 2A].
__global__ __launch_bounds__(POL_HEAD_THREADS) void k_pol_head(PolHeadParams p) {
    pol_head(p.y + (size_t)blockIdx.x * 2 * p.head.A, blockIdx.x, p.head);
}
