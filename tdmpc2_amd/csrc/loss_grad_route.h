// The arithmetic of the loss unit (tdmpc2_loss_*): sizes, the workspace of per-row terms, the grids of its three launches and their
// decode, the per-step constants of the seeds and the order of every sum, as pure functions.  Compilable on the host, no HIP types:
// tests/test_loss_grad_route.py builds it with the host compiler.  The host side (k_loss_grad.hip) walks what these return; the
// kernels (loss_grad_kernels.cuh) use the same functions to decode a workgroup.
//
// Rows.  T = steps, B = batch, L = latent_dim, NB = num_bins, Q = num_q, TB = T * B.  Four kinds of work, in this order in a grid:
//   LS_K_CONS   forward: TB rows of L (one wavefront per row, LS_ROWS rows per workgroup)
//               backward: TB * L elements of d_z_pred (LS_ELEMS per workgroup; thread t owns first + j * LS_THREADS + t, j = 0 .. 3)
//   LS_K_REW    TB rows of NB logits, one wavefront per row
//   LS_K_Q      Q * TB rows of NB logits, row = (q * T + t) * B + b, its target is element row % TB of td_target
//   LS_K_TERM   TB elements, one thread each (LS_THREADS per workgroup); only when episodic
// A kind with no work (termination of a plain model, a backward output that is NULL) takes no workgroups: ls_decode skips it.
//
// Workspace of the forward: float ws[(LS_Q0 + Q) * TB], slot s of row r at s * TB + r: LS_CONS the row's sum of squared differences,
// LS_REW its soft cross-entropy, LS_TERM its binary cross-entropy (never read when not episodic), LS_Q0 + q head q's.
//
// Sums, all fp32, none atomic, none waiting for another workgroup:
//   row      lane l of a wavefront takes columns l, l + 64, ... in rising order (consistency: s = fma(d, d, s); log-sum-exp: the
//            maximum, then s = s + exp(x - max)), then s = s + (s of lane ^ m) for m = 1, 2, 4, 8, 16, 32
//   step     one workgroup (the second launch): ls_ordered_sum over the B terms of a slot at step t -- thread i of LS_THREADS adds
//            src[i], src[i + LS_THREADS], ... from 0 in rising order, then an in-place tree red[i] += red[i + w], w = 128, 64, .. 1
//   loss     per step t = 0 .. T - 1 in rising order: c_t = sum / (float(B) * float(L)), r_t = sum / float(B), v_t = the sum over
//            q = 0 .. Q - 1 of (sum_q / float(B)), e_t = sum / float(B); consistency += c_t * rho_pow[t], reward and value likewise,
//            termination += e_t; then consistency / float(T), reward / float(T), value / float(T * Q), termination / float(T);
//            total = ((cc * consistency + rc * reward) + tc * termination) + vc * value
// rho_pow[t] = fp32(pow(double(rho), t)).
//
// Seeds.  Per step, computed in fp64 from the widened fp32 hyperparameters and rounded once (ls_coef); the kernel multiplies the
// one fp32 factor g = *grad_total in front: c = g * coef.
#pragma once
#include "seed_route.h"

enum { LS_THREADS = SEED_THREADS, LS_WAVES = 4, LS_ROWS = 4, LS_ELEMS = 1024, LS_MAXT = 8 };
enum { LS_CONS = 0, LS_REW = 1, LS_TERM = 2, LS_Q0 = 3 };                     // workspace slots
enum { LS_K_CONS = 0, LS_K_REW = 1, LS_K_Q = 2, LS_K_TERM = 3, LS_KINDS = 4 };  // kinds of work, in grid order
enum { LS_WANT_Z = 1, LS_WANT_REW = 2, LS_WANT_Q = 4, LS_WANT_TERM = 8 };       // backward outputs that are not NULL

struct LsDesc {  // tdmpc2_loss_desc
    int32_t steps, batch, latent_dim, num_q, num_bins, episodic;
    float vmin, vmax, bin_size;
    float rho, consistency_coef, reward_coef, value_coef, termination_coef;
};

// ---- what every entry point refuses on the descriptor alone: 0 = fine, else the index of the message in k_loss_grad.hip
enum { LS_OK = 0, LS_BAD_STEPS, LS_BAD_DIMS, LS_BAD_BINS };
__host__ __device__ inline int ls_check(const LsDesc &d) {
    if (d.steps < 1 || d.steps > LS_MAXT) return LS_BAD_STEPS;
    if (d.batch < 1 || d.latent_dim < 1 || d.num_q < 1) return LS_BAD_DIMS;
    if (d.num_bins < 2) return LS_BAD_BINS;
    return LS_OK;
}

// ---- sizes
__host__ __device__ inline uint64_t ls_tb(const LsDesc &d) { return seed_tb(d); }
__host__ __device__ inline uint64_t ls_ws_floats(const LsDesc &d) { return (uint64_t)(LS_Q0 + d.num_q) * ls_tb(d); }
__host__ __device__ inline uint64_t ls_ws_bytes(const LsDesc &d) { return ls_ws_floats(d) * sizeof(float); }
__host__ __device__ inline uint64_t ls_ws_index(const LsDesc &d, int slot, uint64_t row) { return (uint64_t)slot * ls_tb(d) + row; }
// units of work of a kind: rows, or elements (backward LS_K_CONS, LS_K_TERM)
__host__ __device__ inline uint64_t ls_units(const LsDesc &d, int kind, bool backward) {
    switch (kind) {
    case LS_K_CONS: return backward ? ls_tb(d) * (uint64_t)d.latent_dim : ls_tb(d);
    case LS_K_REW: return ls_tb(d);
    case LS_K_Q: return ls_tb(d) * (uint64_t)d.num_q;
    default: return d.episodic ? ls_tb(d) : 0;
    }
}
__host__ __device__ inline uint64_t ls_units_per_block(int kind, bool backward) {
    if (kind == LS_K_TERM) return LS_THREADS;
    if (kind == LS_K_CONS && backward) return LS_ELEMS;
    return LS_ROWS;
}

// ---- grids
using LsGrid = SeedGrid<LS_KINDS>;
// forward: every kind (want ignored); backward: the kinds in `want` (LS_WANT_*)
__host__ __device__ inline LsGrid ls_grid(const LsDesc &d, bool backward, int want) {
    return seed_grid<LS_KINDS>(backward ? want : ~0, [&](int k) { return ls_units(d, k, backward); },
                               [&](int k) { return ls_units_per_block(k, backward); });
}
__host__ __device__ inline void ls_decode(const LsGrid &g, uint64_t block, int &kind, uint64_t &local) {
    seed_decode(g, block, kind, local);
}
// the step of a row (LS_K_REW, LS_K_Q, forward LS_K_CONS) or element (LS_K_TERM, backward LS_K_CONS: of d_z_pred)
__host__ __device__ inline int ls_step_of(const LsDesc &d, int kind, bool backward, uint64_t unit) {
    if (kind == LS_K_CONS && backward) return (int)(unit / ((uint64_t)d.batch * (uint64_t)d.latent_dim));
    return seed_step_of(d, unit);
}
// the element of reward / td_target / terminated a row reads
__host__ __device__ inline uint64_t ls_target_of(const LsDesc &d, uint64_t row) { return row % ls_tb(d); }
// element j of thread t of workgroup `local` in the backward of LS_K_CONS
__host__ __device__ inline uint64_t ls_elem(uint64_t local, int thread, int j) {
    return local * LS_ELEMS + (uint64_t)j * LS_THREADS + (uint64_t)thread;
}
// the row of a thread's wavefront (row kinds) and the element of a thread (LS_K_TERM); both may lie past the kind's units
__host__ __device__ inline uint64_t ls_row(uint64_t local, int thread) { return local * LS_ROWS + (uint64_t)(thread >> 6); }
__host__ __device__ inline uint64_t ls_term_elem(uint64_t local, int thread) { return local * LS_THREADS + (uint64_t)thread; }

// ---- constants of a call
__host__ inline float ls_rho_pow(const LsDesc &d, int t) { return seed_rho_pow(d, t); }
// the per-step factor of a kind's seeds without g
__host__ inline float ls_coef(const LsDesc &d, int kind, int t) {
    const double w = pow((double)d.rho, (double)t), T = d.steps, B = d.batch;
    switch (kind) {
    case LS_K_CONS: return (float)((double)d.consistency_coef * 2.0 * w / (T * B * (double)d.latent_dim));
    case LS_K_REW: return (float)((double)d.reward_coef * w / (T * B));
    case LS_K_Q: return (float)((double)d.value_coef * w / (T * (double)d.num_q * B));
    default: return (float)((double)d.termination_coef / (T * B));
    }
}

// ---- the order of the step sums, restated serially (the kernel runs the same additions on LS_THREADS threads)
__host__ inline float ls_ordered_sum(const float *src, uint64_t n) { return seed_ordered_sum(src, n); }
