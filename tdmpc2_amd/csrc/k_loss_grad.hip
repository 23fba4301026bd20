// Translation unit of the loss unit (tdmpc2_loss_*): the kernels of loss_grad_kernels.cuh and their host side.  It shares nothing
// with a planner handle and keeps no state: a call is its descriptor, its pointers and, for the forward, a caller-owned workspace.
// Every decision (sizes, grids, decode, the order of the sums, the per-step constants, refusals on the descriptor) is
// loss_grad_route.h's; this file checks arguments, then launches.  Nothing is allocated, nothing synchronises the host: forward
// and backward can be captured in a hipGraph.
#include "launch.h"
#include "loss_grad_route.h"

namespace {
using namespace tdk;
#include "model_rows.cuh"
#include "loss_grad_kernels.cuh"

static_assert(sizeof(LsDesc) == sizeof(tdmpc2_loss_desc) && sizeof(LsDesc) == 56, "tdmpc2_loss_desc is 56 bytes, no padding");

int ls_desc(const tdmpc2_loss_desc *desc, LsDesc &d, const char *what) {
    if (!desc) return fail(TDMPC2_ERR_INVALID, "%s: null descriptor", what);
    d = LsDesc{desc->steps, desc->batch, desc->latent_dim, desc->num_q, desc->num_bins, desc->episodic, desc->vmin, desc->vmax,
               desc->bin_size, desc->rho, desc->consistency_coef, desc->reward_coef, desc->value_coef, desc->termination_coef};
    switch (ls_check(d)) {
    case LS_OK: return 0;
    case LS_BAD_STEPS: return fail(TDMPC2_ERR_INVALID, "%s: steps %d outside [1, %d]", what, d.steps, (int)LS_MAXT);
    case LS_BAD_DIMS:
        return fail(TDMPC2_ERR_INVALID, "%s: batch %d, latent_dim %d, num_q %d: each must be at least 1", what, d.batch, d.latent_dim,
                    d.num_q);
    default:
        return fail(TDMPC2_ERR_UNSUPPORTED, "%s: num_bins %d: the two-hot losses need at least 2 bins (regression heads are not covered)",
                    what, d.num_bins);
    }
}

// the termination pointers are both NULL exactly when the model is not episodic
int ls_term_ptrs(const LsDesc &d, const void *term_logit, const void *terminated, const char *what) {
    if (d.episodic ? (!term_logit || !terminated) : (term_logit || terminated))
        return fail(TDMPC2_ERR_INVALID, "%s: term_logit and terminated are both %s (episodic = %d)", what,
                    d.episodic ? "required" : "NULL on a model without a termination head", d.episodic);
    return 0;
}
}  // namespace

extern "C" {

int tdmpc2_loss_workspace_bytes(const tdmpc2_loss_desc *desc, size_t *ws_bytes) {
    LsDesc d;
    if (int rc = ls_desc(desc, d, "loss_workspace_bytes")) return rc;
    if (!ws_bytes) return fail(TDMPC2_ERR_INVALID, "loss_workspace_bytes: null argument");
    *ws_bytes = (size_t)ls_ws_bytes(d);
    return 0;
}

int tdmpc2_loss_forward(const tdmpc2_loss_desc *desc, const float *z_pred, const float *next_z, const float *reward_logits,
                        const float *reward, const float *q_logits, const float *td_target, const float *term_logit,
                        const float *terminated, float *losses, float *step_means, void *ws, size_t ws_bytes, void *stream) {
    LsDesc d;
    if (int rc = ls_desc(desc, d, "loss_forward")) return rc;
    if (!z_pred || !next_z || !reward_logits || !reward || !q_logits || !td_target || !losses)
        return fail(TDMPC2_ERR_INVALID, "loss_forward: null z_pred, next_z, reward_logits, reward, q_logits, td_target or losses");
    if (int rc = ls_term_ptrs(d, term_logit, terminated, "loss_forward")) return rc;
    LsFwdParams fp{};
    fp.d = d;
    fp.g = ls_grid(d, false, 0);
    if (int rc = grid_fits(fp.g.first[LS_KINDS], "loss_forward")) return rc;
    if (!ws) return fail(TDMPC2_ERR_INVALID, "loss_forward: null workspace");
    if (ws_bytes < ls_ws_bytes(d))
        return fail(TDMPC2_ERR_INVALID, "loss_forward: workspace of %llu bytes is too small, %llu needed (tdmpc2_loss_workspace_bytes)",
                    (unsigned long long)ws_bytes, (unsigned long long)ls_ws_bytes(d));
    fp.z_pred = z_pred; fp.next_z = next_z; fp.reward_logits = reward_logits; fp.reward = reward; fp.q_logits = q_logits;
    fp.td_target = td_target; fp.term_logit = term_logit; fp.terminated = terminated; fp.ws = (float *)ws;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ls_rows, dim3((uint32_t)fp.g.first[LS_KINDS]), dim3(LS_THREADS), 0, st, fp);
    LAUNCH_CHECK();
    LsTailParams tp{};
    tp.d = d;
    tp.ws = (const float *)ws;
    for (int t = 0; t < d.steps; ++t) tp.rho_pow[t] = ls_rho_pow(d, t);
    tp.losses = losses;
    tp.step_means = step_means;
    hipLaunchKernelGGL(k_ls_tail, dim3(1), dim3(LS_THREADS), 0, st, tp);
    LAUNCH_CHECK();
    return 0;
}

int tdmpc2_loss_backward(const tdmpc2_loss_desc *desc, const float *z_pred, const float *next_z, const float *reward_logits,
                         const float *reward, const float *q_logits, const float *td_target, const float *term_logit,
                         const float *terminated, const float *grad_total, float *d_z_pred, float *d_reward_logits,
                         float *d_q_logits, float *d_term_logit, void *stream) {
    LsDesc d;
    if (int rc = ls_desc(desc, d, "loss_backward")) return rc;
    if (!z_pred || !next_z || !reward_logits || !reward || !q_logits || !td_target)
        return fail(TDMPC2_ERR_INVALID, "loss_backward: null z_pred, next_z, reward_logits, reward, q_logits or td_target");
    if (int rc = ls_term_ptrs(d, term_logit, terminated, "loss_backward")) return rc;
    if (d_term_logit && !d.episodic) return fail(TDMPC2_ERR_INVALID, "loss_backward: d_term_logit on a model without a termination head");
    const int want = (d_z_pred ? LS_WANT_Z : 0) | (d_reward_logits ? LS_WANT_REW : 0) | (d_q_logits ? LS_WANT_Q : 0) |
                     (d_term_logit ? LS_WANT_TERM : 0);
    if (!want) return fail(TDMPC2_ERR_INVALID, "loss_backward: every output is null: nothing to compute");
    LsBwdParams bp{};
    bp.d = d;
    bp.g = ls_grid(d, true, want);
    if (int rc = grid_fits(bp.g.first[LS_KINDS], "loss_backward")) return rc;
    bp.z_pred = z_pred; bp.next_z = next_z; bp.reward_logits = reward_logits; bp.reward = reward; bp.q_logits = q_logits;
    bp.td_target = td_target; bp.term_logit = term_logit; bp.terminated = terminated; bp.grad_total = grad_total;
    for (int k = 0; k < LS_KINDS; ++k)
        for (int t = 0; t < d.steps; ++t) bp.coef[k][t] = ls_coef(d, k, t);
    bp.d_z_pred = d_z_pred; bp.d_reward_logits = d_reward_logits; bp.d_q_logits = d_q_logits; bp.d_term_logit = d_term_logit;
    hipLaunchKernelGGL(k_ls_bwd, dim3((uint32_t)bp.g.first[LS_KINDS]), dim3(LS_THREADS), 0, (hipStream_t)stream, bp);
    LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
