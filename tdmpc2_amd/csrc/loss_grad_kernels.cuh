// Kernels of the loss unit (included by k_loss_grad.hip inside its namespace, after model_rows.cuh): the per-row terms of the four
// losses of TDMPC2._update (tdmpc2/tdmpc2.py:272-304), their fixed-order final add, and the gradient seeds of the total in one
// launch.  Every decision (grids, decode, workspace slots, the order of the sums, the per-step constants) is loss_grad_route.h's.
// The row math is model_rows.cuh's: symlog_f through an fp64 log, model_soft_ce with the two bins picked by index, model_bce.

struct LsFwdParams {
    LsDesc d;
    LsGrid g;
    const float *z_pred, *next_z, *reward_logits, *reward, *q_logits, *td_target, *term_logit, *terminated;
    float *ws;
};

struct LsTailParams {
    LsDesc d;
    const float *ws;
    float rho_pow[LS_MAXT];
    float *losses;      // [5]
    float *step_means;  // [4, steps] or null
};

struct LsBwdParams {
    LsDesc d;
    LsGrid g;
    const float *z_pred, *next_z, *reward_logits, *reward, *q_logits, *td_target, *term_logit, *terminated;
    const float *grad_total;  // device float[1] or null (= 1)
    float coef[LS_KINDS][LS_MAXT];
    float *d_z_pred, *d_reward_logits, *d_q_logits, *d_term_logit;
};

__device__ __forceinline__ ModelLossArgs ls_loss_args(const LsDesc &d) {
    ModelLossArgs a{};
    a.num_bins = d.num_bins;
    a.vmin = d.vmin;
    a.vmax = d.vmax;
    a.bin_size = d.bin_size;
    return a;
}

// launch 1 of the forward: the per-row terms
__global__ __launch_bounds__(LS_THREADS) void k_ls_rows(const LsFwdParams p) {
    int kind;
    uint64_t local;
    ls_decode(p.g, blockIdx.x, kind, local);
    const uint64_t TB = ls_tb(p.d);
    if (kind == LS_K_TERM) {
        const uint64_t e = ls_term_elem(local, (int)threadIdx.x);
        if (e < TB) p.ws[ls_ws_index(p.d, LS_TERM, e)] = model_bce(p.term_logit[e], p.terminated[e]);
        return;
    }
    const int lane = threadIdx.x & 63;
    const uint64_t row = ls_row(local, (int)threadIdx.x);
    if (row >= ls_units(p.d, kind, false)) return;
    if (kind == LS_K_CONS) {
        const int L = p.d.latent_dim;
        const float *a = p.z_pred + row * (uint64_t)L, *b = p.next_z + row * (uint64_t)L;
        float s = 0.f;
        for (int c = lane; c < L; c += 64) {
            const float df = a[c] - b[c];
            s = fmaf(df, df, s);
        }
        s = group_sum<64>(s);
        if (lane == 0) p.ws[ls_ws_index(p.d, LS_CONS, row)] = s;
        return;
    }
    const bool q = kind == LS_K_Q;
    const float *rp = (q ? p.q_logits : p.reward_logits) + row * (uint64_t)p.d.num_bins;
    float m, es;
    row_max_sum(rp, lane, p.d.num_bins, m, es);
    if (lane != 0) return;
    const float lse = m + logf(es);
    const float target = (q ? p.td_target : p.reward)[ls_target_of(p.d, row)];
    // (slot LS_Q0 + head of row (head * T + t) * B + b is LS_Q0 * TB + row)
    p.ws[ls_ws_index(p.d, q ? LS_Q0 : LS_REW, row)] = model_soft_ce(rp, lse, target, ls_loss_args(p.d));
}

// launch 2 of the forward: tdmpc2/tdmpc2.py:285-304 from the per-row terms.  One workgroup; block_sum is ls_ordered_sum.
__global__ __launch_bounds__(LS_THREADS) void k_ls_tail(const LsTailParams p) {
    __shared__ float red[LS_THREADS];
    const int T = p.d.steps, Q = p.d.num_q;
    const uint64_t B = (uint64_t)p.d.batch;
    const float fB = (float)p.d.batch;
    float cons = 0.f, rew = 0.f, val = 0.f, term = 0.f;
    for (int t = 0; t < T; ++t) {
        const uint64_t r0 = (uint64_t)t * B;
        const float c_t = block_sum(p.ws + ls_ws_index(p.d, LS_CONS, r0), B, red) / (fB * (float)p.d.latent_dim);
        const float r_t = block_sum(p.ws + ls_ws_index(p.d, LS_REW, r0), B, red) / fB;
        float v_t = 0.f;
        for (int i = 0; i < Q; ++i) v_t += block_sum(p.ws + ls_ws_index(p.d, LS_Q0 + i, r0), B, red) / fB;
        const float e_t = p.d.episodic ? block_sum(p.ws + ls_ws_index(p.d, LS_TERM, r0), B, red) / fB : 0.f;
        cons += c_t * p.rho_pow[t];
        rew += r_t * p.rho_pow[t];
        val += v_t * p.rho_pow[t];
        term += e_t;
        if (p.step_means && threadIdx.x == 0) {
            p.step_means[0 * T + t] = c_t;
            p.step_means[1 * T + t] = r_t;
            p.step_means[2 * T + t] = v_t / (float)Q;
            p.step_means[3 * T + t] = e_t;
        }
    }
    if (threadIdx.x != 0) return;
    cons /= (float)T;
    rew /= (float)T;
    val /= (float)(T * Q);
    term /= (float)T;
    p.losses[0] = cons;
    p.losses[1] = rew;
    p.losses[2] = val;
    p.losses[3] = term;
    p.losses[4] = p.d.consistency_coef * cons + p.d.reward_coef * rew + p.d.termination_coef * term + p.d.value_coef * val;
}

// the one launch of the backward: the seeds of `total` over every kind whose output was asked for.  Nothing was saved by the
// forward: a row's max and sum are computed again.
__global__ __launch_bounds__(LS_THREADS) void k_ls_bwd(const LsBwdParams p) {
    int kind;
    uint64_t local;
    ls_decode(p.g, blockIdx.x, kind, local);
    const float g = p.grad_total ? *p.grad_total : 1.f;
    const uint64_t n = ls_units(p.d, kind, true);
    if (kind == LS_K_CONS) {
#pragma unroll
        for (int j = 0; j < LS_ELEMS / LS_THREADS; ++j) {
            const uint64_t e = ls_elem(local, (int)threadIdx.x, j);
            if (e >= n) continue;
            const float c = g * p.coef[LS_K_CONS][ls_step_of(p.d, LS_K_CONS, true, e)];
            p.d_z_pred[e] = c * (p.z_pred[e] - p.next_z[e]);
        }
        return;
    }
    if (kind == LS_K_TERM) {
        const uint64_t e = ls_term_elem(local, (int)threadIdx.x);
        if (e >= n) return;
        const float c = g * p.coef[LS_K_TERM][0];
        const float sig = 1.f / (1.f + expf(-p.term_logit[e]));
        p.d_term_logit[e] = c * (sig - p.terminated[e]);
        return;
    }
    const int lane = threadIdx.x & 63;
    const uint64_t row = ls_row(local, (int)threadIdx.x);
    if (row >= n) return;
    const bool q = kind == LS_K_Q;
    const int NB = p.d.num_bins;
    const float *rp = (q ? p.q_logits : p.reward_logits) + row * (uint64_t)NB;
    float *out = (q ? p.d_q_logits : p.d_reward_logits) + row * (uint64_t)NB;
    float m, es;
    row_max_sum(rp, lane, NB, m, es);
    // the two-hot row of math.py:58-71, as model_soft_ce picks it: weights 1 - off at i0 and off at i1
    const float target = (q ? p.td_target : p.reward)[ls_target_of(p.d, row)];
    const float s = symlog_f(target);
    const float x = s != s ? s : fminf(fmaxf(s, p.d.vmin), p.d.vmax);
    const float u = (x - p.d.vmin) / p.d.bin_size;
    const float fl = floorf(u);
    const float off = u - fl, w0 = 1.f - off;
    int i0 = fl == fl ? (int)fl : 0;
    i0 = i0 < 0 ? 0 : (i0 > NB - 1 ? NB - 1 : i0);
    const int i1 = (i0 + 1) % NB;
    const float S = w0 + off;  // what log_softmax's backward sums of its incoming gradient
    const float c = g * p.coef[kind][ls_step_of(p.d, kind, true, row)];
    for (int k = lane; k < NB; k += 64) {
        const float pk = expf(rp[k] - m) / es;
        const float th = k == i0 ? w0 : (k == i1 ? off : 0.f);
        out[k] = c * (pk * S - th);
    }
}
