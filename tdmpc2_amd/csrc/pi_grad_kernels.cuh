// Kernels of the policy-loss unit (included by k_pi_grad.hip inside its namespace, after model_rows.cuh): the Gaussian head of
// WorldModel.pi after its MLP (tdmpc2/common/math.py:12-39, world_model.py:160-184) forward and backward, two_hot_inv of the two
// drawn Q heads and their average, the rho-weighted loss of update_pi (tdmpc2/tdmpc2.py:221-226) and its gradient seeds.  Every
// decision (grids, decode, bins, the order of the sums, the per-step constants) is pi_grad_route.h's.  The row statistics of a
// logit row are model_rows.cuh's model_row_stats over the bins of pg_bin, held in LDS by each workgroup.

struct PgHeadParams {
    PgDesc d;
    const float *pi_out, *eps, *mask;
    const float *d_action, *d_se;  // backward: either may be null (= zero)
    float *action, *entropy, *se;  // forward
    float *d_pi_out;               // backward
};

struct PgValueParams {
    PgDesc d;
    const float *q_logits;
    float *q;
};

struct PgLossParams {
    PgDesc d;
    const float *q, *entropy, *se, *scale;
    float rho_pow[PG_MAXT];
    float *losses;      // [3]
    float *step_means;  // [steps] or null
};

struct PgBwdParams {
    PgDesc d;
    PgGrid g;
    const float *q_logits, *scale, *grad_total;
    float coef_q[PG_MAXT], coef_se[PG_MAXT];
    float *d_q_logits, *d_se;
};

// ---------------------------------------------------------------- the Gaussian head
// One column of a row, every product and sum rounded on its own as the reference's tensor operations round them.
struct PgCol {
    float th;   // tanh(raw log_std)
    float ls;   // masked log_std
    float e;    // masked eps
    float sd;   // exp(log_std)
    float a;    // tanh(mean + eps * sd)
    float om;   // 1 - a * a
    float lp;   // -0.5 eps^2 - log_std - log(2 pi) / 2
    float sq;   // log(relu(1 - a^2) + 1e-6)
};
__device__ __forceinline__ PgCol pg_col(const PgDesc &d, float mean, float raw, float eps, float m, bool masked) {
#pragma clang fp contract(off)
    PgCol c;
    c.th = tanhf(raw);
    c.ls = d.log_std_min + (0.5f * d.log_std_dif) * (c.th + 1.f);
    c.e = eps;
    if (masked) {
        mean = mean * m;
        c.ls = c.ls * m;
        c.e = eps * m;
    }
    c.sd = expf(c.ls);
    c.a = tanhf(mean + c.e * c.sd);
    c.om = 1.f - c.a * c.a;
    c.lp = (-0.5f * (c.e * c.e) - c.ls) - 0.9189385175704956f;
    c.sq = logf(fmaxf(c.om, 0.f) + 1e-6f);
    return c;
}

// the row sums of a head row on its 8 lanes: log_prob before the squash, the squash term, the mask row's sum
__device__ __forceinline__ void pg_head_sums(const PgHeadParams &p, uint64_t row, int part, float *action, float &lp0, float &K,
                                             float &size) {
    const int A = p.d.action_dim;
    const float *y = p.pi_out + row * (uint64_t)(2 * A), *ep = p.eps + row * (uint64_t)A;
    const float *mk = p.mask ? p.mask + pg_mask_row(p.d, row) * (uint64_t)A : nullptr;
    lp0 = 0.f;
    K = 0.f;
    size = 0.f;
    for (int j = part; j < A; j += PG_HEAD_LANES) {
        const float m = mk ? mk[j] : 1.f;
        const PgCol c = pg_col(p.d, y[j], y[A + j], ep[j], m, mk != nullptr);
        lp0 += c.lp;
        K += c.sq;
        size += m;
        if (action) action[row * (uint64_t)A + j] = c.a;
    }
    lp0 = group_sum<PG_HEAD_LANES>(lp0);
    K = group_sum<PG_HEAD_LANES>(K);
    size = mk ? group_sum<PG_HEAD_LANES>(size) : (float)A;
}

__global__ __launch_bounds__(PG_THREADS) void k_pg_head_fwd(const PgHeadParams p) {
#pragma clang fp contract(off)
    const uint64_t row = pg_head_row(blockIdx.x, (int)threadIdx.x);
    const int part = pg_head_part((int)threadIdx.x);
    if (row >= pg_tb(p.d)) return;  // (a whole group of 8 lanes leaves: the shuffles of the others stay inside their groups)
    float lp0, K, size;
    pg_head_sums(p, row, part, p.action, lp0, K, size);
    if (part != 0) return;
    const float slp = lp0 * size;
    const float lp = lp0 - K;
    p.entropy[row] = -lp;
    p.se[row] = (-lp) * (slp / (lp + 1e-8f));
}

// d_pi_out of one row: the row sums again, then per column
//   se = -lp S / den, S = lp0 size, lp = lp0 - K, den = lp + 1e-8:  d se / d S = -lp / den,  d se / d lp = -S 1e-8 / den^2
//   (the two terms of autograd's -S / den + lp S / den^2, which cancel to that, taken together)
__global__ __launch_bounds__(PG_THREADS) void k_pg_head_bwd(const PgHeadParams p) {
#pragma clang fp contract(off)
    const uint64_t row = pg_head_row(blockIdx.x, (int)threadIdx.x);
    const int part = pg_head_part((int)threadIdx.x);
    if (row >= pg_tb(p.d)) return;
    const int A = p.d.action_dim;
    float lp0, K, size;
    pg_head_sums(p, row, part, nullptr, lp0, K, size);
    const float lp = lp0 - K, den = lp + 1e-8f, S = lp0 * size;
    const float gs = p.d_se ? p.d_se[row] : 0.f;
    const float g_S = gs * (-(lp / den));
    const float g_lp = gs * (-((S * 1e-8f) / (den * den)));
    const float g_lp0 = g_lp + g_S * size;
    const float g_K = -g_lp;
    const float *y = p.pi_out + row * (uint64_t)(2 * A), *ep = p.eps + row * (uint64_t)A;
    const float *mk = p.mask ? p.mask + pg_mask_row(p.d, row) * (uint64_t)A : nullptr;
    const float *ga = p.d_action ? p.d_action + row * (uint64_t)A : nullptr;
    float *out = p.d_pi_out + row * (uint64_t)(2 * A);
    for (int j = part; j < A; j += PG_HEAD_LANES) {
        const float m = mk ? mk[j] : 1.f;
        const PgCol c = pg_col(p.d, y[j], y[A + j], ep[j], m, mk != nullptr);
        const float dK = c.om > 0.f ? (-2.f * c.a) / (c.om + 1e-6f) : 0.f;  // relu' = 0 where 1 - a^2 <= 0
        const float g_a = (ga ? ga[j] : 0.f) + g_K * dK;
        const float g_u = g_a * c.om;  // tanh' = 1 - y^2
        const float g_ls = g_u * (c.e * c.sd) - g_lp0;
        const float th1 = 1.f - c.th * c.th;
        out[j] = g_u * m;
        out[A + j] = ((g_ls * m) * (0.5f * p.d.log_std_dif)) * th1;
    }
}

// ---------------------------------------------------------------- two_hot_inv of the two heads
// the bins of the descriptor into LDS, by the whole workgroup (before any thread leaves)
__device__ __forceinline__ void pg_fill_bins(const PgDesc &d, float *bins) {
    for (int k = threadIdx.x; k < d.num_bins; k += PG_THREADS) bins[k] = pg_bin(d, k);
    __syncthreads();
}

__global__ __launch_bounds__(PG_THREADS) void k_pg_value(const PgValueParams p) {
    __shared__ float bins[PG_MAXBINS];
    pg_fill_bins(p.d, bins);
    const int lane = threadIdx.x & 63, NB = p.d.num_bins;
    const uint64_t TB = pg_tb(p.d), row = pg_row(blockIdx.x, (int)threadIdx.x);
    if (row >= TB) return;
    float lse0, lse1, q0, q1;
    model_row_stats<64>(p.q_logits + row * (uint64_t)NB, lane, NB, bins, lse0, q0);
    model_row_stats<64>(p.q_logits + (TB + row) * (uint64_t)NB, lane, NB, bins, lse1, q1);
    // a NaN logit makes the row's sum of exponentials NaN, which symexp_f's comparisons turn into 0: the row's q is NaN here, as
    // every torch op of the reference propagates it
    if (lse0 != lse0) q0 = lse0;
    if (lse1 != lse1) q1 = lse1;
    if (lane == 0) p.q[row] = (q0 + q1) / 2.f;
}

// ---------------------------------------------------------------- the loss
// pg_step_sum / pg_ordered_sum of pi_grad_route.h on the workgroup's PG_THREADS threads: block_tree / block_sum of model_rows.cuh
__global__ __launch_bounds__(PG_THREADS) void k_pg_loss(const PgLossParams p) {
    __shared__ float red[PG_THREADS];
    const uint64_t B = (uint64_t)p.d.batch;
    const float scale = *p.scale;
    float loss = 0.f;
    for (int t = 0; t < p.d.steps; ++t) {
        const float *q = p.q + (uint64_t)t * B, *se = p.se + (uint64_t)t * B;
        float s = 0.f;
        for (uint64_t i = threadIdx.x; i < B; i += PG_THREADS) s = s + pg_term(q[i], se[i], p.d.entropy_coef, scale);
        const float m = block_tree(s, red) / (float)p.d.batch;
        loss = pg_loss_step(loss, m, p.rho_pow[t]);
        if (p.step_means && threadIdx.x == 0) p.step_means[t] = m;
    }
    const float ent = block_sum(p.entropy, pg_tb(p.d), red);
    const float sent = block_sum(p.se, pg_tb(p.d), red);
    if (threadIdx.x != 0) return;
    const float rows = (float)p.d.steps * (float)p.d.batch;
    p.losses[0] = loss / (float)p.d.steps;
    p.losses[1] = ent / rows;
    p.losses[2] = sent / rows;
}

// the one launch of the loss's backward.  Nothing was saved by the forward: a row's statistics are computed again.
__global__ __launch_bounds__(PG_THREADS) void k_pg_loss_bwd(const PgBwdParams p) {
    __shared__ float bins[PG_MAXBINS];
    int kind;
    uint64_t local;
    pg_decode(p.g, blockIdx.x, kind, local);
    const float g = p.grad_total ? *p.grad_total : 1.f;
    if (kind == PG_K_SE) {
        const uint64_t e = pg_se_elem(local, (int)threadIdx.x);
        if (e < pg_tb(p.d)) p.d_se[e] = g * p.coef_se[pg_step_of(p.d, e)];
        return;
    }
    pg_fill_bins(p.d, bins);
    const int lane = threadIdx.x & 63, NB = p.d.num_bins;
    const uint64_t row = pg_row(local, (int)threadIdx.x);
    if (row >= pg_units(p.d, PG_K_Q)) return;
    const float *rp = p.q_logits + row * (uint64_t)NB;
    float *out = p.d_q_logits + row * (uint64_t)NB;
    const float m = row_max(rp, lane, NB);
    // The sums of exp and of exp * bin in fp64, rounded once into x: symexp'(x) = exp|x| turns an ulp of x (1e-6 at |x| = 8) into a
    // relative error of the whole row's seeds, and the fp32 sums of model_row_stats are good to about an ulp -- restated on the
    // CPU in that order against the fixture: 1.2e-6 of the tensor's maximum where the gate of tests/test_gpu_pi_grad.py is 1.3e-6.
    double es = 0.0, xs = 0.0;
    for (int j = lane; j < NB; j += 64) {
        const double ev = (double)expf(rp[j] - m);
        es += ev;
        xs += ev * (double)bins[j];
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        es += __shfl_xor(es, o);
        xs += __shfl_xor(xs, o);
    }
    const float x = (float)(xs / es), esf = (float)es;
    // symexp'(x) = exp|x|, exactly 0 at x == 0 (torch: sign(x) * (exp(|x|) - 1) through sign' = 0 and abs' = sign)
    const float ds = x != 0.f ? expf(fabsf(x)) : 0.f;
    const float c = ((g * p.coef_q[pg_step_of(p.d, row)]) / *p.scale) * ds;
    for (int k = lane; k < NB; k += 64) {
        const float pk = expf(rp[k] - m) / esf;
        out[k] = c * (pk * (bins[k] - x));
    }
}
