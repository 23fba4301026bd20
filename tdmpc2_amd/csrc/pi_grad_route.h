// The arithmetic of the policy-loss unit (tdmpc2_pigrad_*): the grids of its five launches and their decode, the bin values, the
// per-step constants of the seeds and the order of every sum of the loss, as pure functions.  Compilable on the host, no HIP types:
// tests/test_pi_grad_route.py builds it with the host compiler.  The host side (k_pi_grad.hip) walks what these return; the kernels
// (pi_grad_kernels.cuh) use the same functions to decode a workgroup.
//
// Rows.  T = steps, B = batch, A = action_dim, NB = num_bins, TB = T * B.
//   head (forward and backward)   TB rows, PG_HEAD_LANES lanes per row, PG_HEAD_ROWS rows per workgroup; lane l of a row takes
//                                 columns l, l + 8, ... of its A; the mask row of row r is r % B
//   value_forward                 TB row pairs, one wavefront per pair (row r of head 0, then row TB + r of head 1), PG_ROWS per
//                                 workgroup
//   loss_backward                 two kinds of work, in this order in the grid:
//     PG_K_Q    2 TB rows of NB logits, one wavefront per row, row = (head * T + t) * B + b
//     PG_K_SE   TB elements of d_scaled_entropy, one thread each (PG_THREADS per workgroup)
//   A kind whose output is NULL takes no workgroups: pg_decode skips it.
//
// Sums of the loss, all fp32, none atomic, one workgroup:
//   step     pg_step_sum over the B rows of step t: thread i of PG_THREADS adds pg_term(q[i], se[i]), pg_term(q[i + PG_THREADS], ..)
//            ... from 0 in rising order, then an in-place tree red[i] += red[i + w], w = 128, 64, .. 1
//            pg_term = fl(fl(entropy_coef * se) + fl(q / scale)), no contraction
//   loss     per step t = 0 .. T - 1 in rising order: m_t = sum / float(B), loss += (-m_t) * rho_pow[t]; then loss / float(T)
//   means    pg_ordered_sum over all TB elements of entropy (of scaled_entropy), / (float(T) * float(B))
// rho_pow[t] = fp32(pow(double(rho), t)).
//
// Seeds.  Per step, computed in fp64 from the widened fp32 hyperparameters and rounded once (pg_coef_q, pg_coef_se, both negative);
// the kernel multiplies the one fp32 factor g = *grad_total in front: c = g * coef.
#pragma once
#include "seed_route.h"

enum { PG_THREADS = SEED_THREADS, PG_ROWS = 4, PG_HEAD_LANES = 8, PG_HEAD_ROWS = 32, PG_MAXT = 16, PG_MAXA = 64, PG_MAXBINS = 4096 };
enum { PG_K_Q = 0, PG_K_SE = 1, PG_KINDS = 2 };  // kinds of work of loss_backward, in grid order
enum { PG_WANT_Q = 1, PG_WANT_SE = 2 };          // its outputs that are not NULL

struct PgDesc {  // tdmpc2_pigrad_desc
    int32_t steps, batch, action_dim, num_bins, multitask;
    float vmin, vmax, rho, entropy_coef, log_std_min, log_std_dif;
};

// ---- what every entry point refuses on the descriptor alone: 0 = fine, else the index of the message in k_pi_grad.hip
enum { PG_OK = 0, PG_BAD_STEPS, PG_BAD_BATCH, PG_BAD_ACTION, PG_BAD_BINS };
__host__ __device__ inline int pg_check(const PgDesc &d) {
    if (d.steps < 1 || d.steps > PG_MAXT) return PG_BAD_STEPS;
    if (d.batch < 1) return PG_BAD_BATCH;
    if (d.action_dim < 1 || d.action_dim > PG_MAXA) return PG_BAD_ACTION;
    if (d.num_bins < 2 || d.num_bins > PG_MAXBINS) return PG_BAD_BINS;
    return PG_OK;
}

// ---- sizes and grids
__host__ __device__ inline uint64_t pg_tb(const PgDesc &d) { return seed_tb(d); }
__host__ __device__ inline uint64_t pg_head_grid(const PgDesc &d) { return (pg_tb(d) + (PG_HEAD_ROWS - 1)) / PG_HEAD_ROWS; }
__host__ __device__ inline uint64_t pg_value_grid(const PgDesc &d) { return (pg_tb(d) + (PG_ROWS - 1)) / PG_ROWS; }
// the row of a thread of the head kernels and its first column; both may lie past the rows / the row's A
__host__ __device__ inline uint64_t pg_head_row(uint64_t block, int thread) {
    return block * PG_HEAD_ROWS + (uint64_t)(thread / PG_HEAD_LANES);
}
__host__ __device__ inline int pg_head_part(int thread) { return thread % PG_HEAD_LANES; }
__host__ __device__ inline uint64_t pg_mask_row(const PgDesc &d, uint64_t row) { return row % (uint64_t)d.batch; }
// the row (pair) of a thread's wavefront and the element of a thread (PG_K_SE); both may lie past the kind's units
__host__ __device__ inline uint64_t pg_row(uint64_t local, int thread) { return local * PG_ROWS + (uint64_t)(thread >> 6); }
__host__ __device__ inline uint64_t pg_se_elem(uint64_t local, int thread) { return local * PG_THREADS + (uint64_t)thread; }

__host__ __device__ inline uint64_t pg_units(const PgDesc &d, int kind) { return kind == PG_K_Q ? 2 * pg_tb(d) : pg_tb(d); }
__host__ __device__ inline uint64_t pg_units_per_block(int kind) { return kind == PG_K_Q ? PG_ROWS : PG_THREADS; }
using PgGrid = SeedGrid<PG_KINDS>;
__host__ __device__ inline PgGrid pg_bwd_grid(const PgDesc &d, int want) {
    return seed_grid<PG_KINDS>(want, [&](int k) { return pg_units(d, k); }, [](int k) { return pg_units_per_block(k); });
}
__host__ __device__ inline void pg_decode(const PgGrid &g, uint64_t block, int &kind, uint64_t &local) {
    seed_decode(g, block, kind, local);
}
// the step of a row of PG_K_Q or an element of PG_K_SE
__host__ __device__ inline int pg_step_of(const PgDesc &d, uint64_t unit) { return seed_step_of(d, unit); }

// ---- bin k of torch.linspace(vmin, vmax, num_bins) in fp32, as the planner's handle forms its table (plan_core.hip): the float
// step, the product and the sum in fp64, rounded once; the upper half counted down from vmax
__host__ __device__ inline float pg_bin(const PgDesc &d, int k) {
    const float step = (d.vmax - d.vmin) / (float)(d.num_bins - 1);
    return k < d.num_bins / 2 ? (float)((double)d.vmin + (double)step * k)
                              : (float)((double)d.vmax - (double)step * (d.num_bins - 1 - k));
}

// ---- constants of a call
__host__ inline float pg_rho_pow(const PgDesc &d, int t) { return seed_rho_pow(d, t); }
// the per-step factors of the seeds without g
__host__ inline float pg_coef_q(const PgDesc &d, int t) {
    return (float)(-pow((double)d.rho, (double)t) / (2.0 * (double)d.steps * (double)d.batch));
}
__host__ inline float pg_coef_se(const PgDesc &d, int t) {
    return (float)(-(double)d.entropy_coef * pow((double)d.rho, (double)t) / ((double)d.steps * (double)d.batch));
}

// ---- one term of a step's sum: every operation rounded on its own
__host__ __device__ inline float pg_term(float q, float se, float entropy_coef, float scale) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float a = entropy_coef * se;
    const float b = q / scale;
    return a + b;
}

// one step's share of the loss: loss + fl((-m) * w), no contraction
__host__ __device__ inline float pg_loss_step(float loss, float m, float w) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float p = (-m) * w;
    return loss + p;
}

// ---- the order of the sums, restated serially (the kernel runs the same additions on PG_THREADS threads)
__host__ inline float pg_ordered_sum(const float *src, uint64_t n) { return seed_ordered_sum(src, n); }
__host__ inline float pg_step_sum(const float *q, const float *se, uint64_t n, float entropy_coef, float scale) {
    return seed_ordered_sum(n, [=](uint64_t k) { return pg_term(q[k], se[k], entropy_coef, scale); });
}
// losses [3] and step_means [T] (or null) of tdmpc2_pigrad_loss_forward, serially
__host__ inline void pg_loss_serial(const PgDesc &d, const float *q, const float *entropy, const float *se, float scale, float *losses,
                                    float *step_means) {
    const uint64_t B = (uint64_t)d.batch;
    float loss = 0.0f;
    for (int t = 0; t < d.steps; ++t) {
        const float m = pg_step_sum(q + (uint64_t)t * B, se + (uint64_t)t * B, B, d.entropy_coef, scale) / (float)d.batch;
        loss = pg_loss_step(loss, m, pg_rho_pow(d, t));
        if (step_means) step_means[t] = m;
    }
    const float rows = (float)d.steps * (float)d.batch;
    losses[0] = loss / (float)d.steps;
    losses[1] = pg_ordered_sum(entropy, pg_tb(d)) / rows;
    losses[2] = pg_ordered_sum(se, pg_tb(d)) / rows;
}
