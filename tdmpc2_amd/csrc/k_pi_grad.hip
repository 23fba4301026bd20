// Translation unit of the policy-loss unit (tdmpc2_pigrad_*, include/tdmpc2_pi_grad.h): the kernels of pi_grad_kernels.cuh and
// their host side.  It shares nothing with a planner handle and keeps no state: a call is its descriptor and its pointers.  Every
// decision (grids, decode, bins, the order of the sums, the per-step constants, refusals on the descriptor) is pi_grad_route.h's;
// this file checks arguments, then launches.  Nothing is allocated, nothing synchronises the host: every call can be captured in
// a hipGraph.
#include "../../include/tdmpc2_pi_grad.h"
#include "launch.h"
#include "pi_grad_route.h"

namespace {
using namespace tdk;
#include "model_rows.cuh"
#include "pi_grad_kernels.cuh"

static_assert(sizeof(PgDesc) == sizeof(tdmpc2_pigrad_desc) && sizeof(PgDesc) == 44, "tdmpc2_pigrad_desc is 44 bytes, no padding");

int pg_desc(const tdmpc2_pigrad_desc *desc, PgDesc &d, const char *what) {
    if (!desc) return fail(TDMPC2_ERR_INVALID, "%s: null descriptor", what);
    d = PgDesc{desc->steps, desc->batch, desc->action_dim, desc->num_bins, desc->multitask, desc->vmin, desc->vmax, desc->rho,
               desc->entropy_coef, desc->log_std_min, desc->log_std_dif};
    switch (pg_check(d)) {
    case PG_OK: return 0;
    case PG_BAD_STEPS: return fail(TDMPC2_ERR_INVALID, "%s: steps %d outside [1, %d]", what, d.steps, (int)PG_MAXT);
    case PG_BAD_BATCH: return fail(TDMPC2_ERR_INVALID, "%s: batch %d: must be at least 1", what, d.batch);
    case PG_BAD_ACTION: return fail(TDMPC2_ERR_INVALID, "%s: action_dim %d outside [1, %d]", what, d.action_dim, (int)PG_MAXA);
    default:
        return fail(TDMPC2_ERR_UNSUPPORTED, "%s: num_bins %d outside [2, %d] (regression heads are not covered; the bins live in LDS)",
                    what, d.num_bins, (int)PG_MAXBINS);
    }
}

// the mask is non-NULL exactly when the descriptor says multitask
int pg_mask(const PgDesc &d, const void *mask, const char *what) {
    if (d.multitask ? !mask : mask != nullptr)
        return fail(TDMPC2_ERR_INVALID, "%s: action_mask is %s (multitask = %d)", what,
                    d.multitask ? "required" : "NULL on a single-task model", d.multitask);
    return 0;
}
}  // namespace

extern "C" {

int tdmpc2_pigrad_head_forward(const tdmpc2_pigrad_desc *desc, const float *pi_out, const float *eps, const float *action_mask,
                               float *action, float *entropy, float *scaled_entropy, void *stream) {
    PgDesc d;
    if (int rc = pg_desc(desc, d, "pigrad_head_forward")) return rc;
    if (!pi_out || !eps || !action || !entropy || !scaled_entropy)
        return fail(TDMPC2_ERR_INVALID, "pigrad_head_forward: null pi_out, eps, action, entropy or scaled_entropy");
    if (int rc = pg_mask(d, action_mask, "pigrad_head_forward")) return rc;
    if (int rc = grid_fits(pg_head_grid(d), "pigrad_head_forward")) return rc;
    PgHeadParams hp{};
    hp.d = d;
    hp.pi_out = pi_out; hp.eps = eps; hp.mask = action_mask; hp.action = action; hp.entropy = entropy; hp.se = scaled_entropy;
    hipLaunchKernelGGL(k_pg_head_fwd, dim3((uint32_t)pg_head_grid(d)), dim3(PG_THREADS), 0, (hipStream_t)stream, hp);
    LAUNCH_CHECK();
    return 0;
}

int tdmpc2_pigrad_head_backward(const tdmpc2_pigrad_desc *desc, const float *pi_out, const float *eps, const float *action_mask,
                                const float *d_action, const float *d_scaled_entropy, float *d_pi_out, void *stream) {
    PgDesc d;
    if (int rc = pg_desc(desc, d, "pigrad_head_backward")) return rc;
    if (!pi_out || !eps) return fail(TDMPC2_ERR_INVALID, "pigrad_head_backward: null pi_out or eps");
    if (int rc = pg_mask(d, action_mask, "pigrad_head_backward")) return rc;
    if (!d_action && !d_scaled_entropy)
        return fail(TDMPC2_ERR_INVALID, "pigrad_head_backward: d_action and d_scaled_entropy are both null: no incoming gradient");
    if (!d_pi_out) return fail(TDMPC2_ERR_INVALID, "pigrad_head_backward: d_pi_out is null: nothing to compute");
    if (int rc = grid_fits(pg_head_grid(d), "pigrad_head_backward")) return rc;
    PgHeadParams hp{};
    hp.d = d;
    hp.pi_out = pi_out; hp.eps = eps; hp.mask = action_mask; hp.d_action = d_action; hp.d_se = d_scaled_entropy; hp.d_pi_out = d_pi_out;
    hipLaunchKernelGGL(k_pg_head_bwd, dim3((uint32_t)pg_head_grid(d)), dim3(PG_THREADS), 0, (hipStream_t)stream, hp);
    LAUNCH_CHECK();
    return 0;
}

int tdmpc2_pigrad_value_forward(const tdmpc2_pigrad_desc *desc, const float *q_logits, float *q, void *stream) {
    PgDesc d;
    if (int rc = pg_desc(desc, d, "pigrad_value_forward")) return rc;
    if (!q_logits || !q) return fail(TDMPC2_ERR_INVALID, "pigrad_value_forward: null q_logits or q");
    if (int rc = grid_fits(pg_value_grid(d), "pigrad_value_forward")) return rc;
    PgValueParams vp{};
    vp.d = d;
    vp.q_logits = q_logits; vp.q = q;
    hipLaunchKernelGGL(k_pg_value, dim3((uint32_t)pg_value_grid(d)), dim3(PG_THREADS), 0, (hipStream_t)stream, vp);
    LAUNCH_CHECK();
    return 0;
}

int tdmpc2_pigrad_loss_forward(const tdmpc2_pigrad_desc *desc, const float *q, const float *entropy, const float *scaled_entropy,
                               const float *scale, float *losses, float *step_means, void *stream) {
    PgDesc d;
    if (int rc = pg_desc(desc, d, "pigrad_loss_forward")) return rc;
    if (!q || !entropy || !scaled_entropy || !scale || !losses)
        return fail(TDMPC2_ERR_INVALID, "pigrad_loss_forward: null q, entropy, scaled_entropy, scale or losses");
    PgLossParams lp{};
    lp.d = d;
    lp.q = q; lp.entropy = entropy; lp.se = scaled_entropy; lp.scale = scale; lp.losses = losses; lp.step_means = step_means;
    for (int t = 0; t < d.steps; ++t) lp.rho_pow[t] = pg_rho_pow(d, t);
    hipLaunchKernelGGL(k_pg_loss, dim3(1), dim3(PG_THREADS), 0, (hipStream_t)stream, lp);
    LAUNCH_CHECK();
    return 0;
}

int tdmpc2_pigrad_loss_backward(const tdmpc2_pigrad_desc *desc, const float *q_logits, const float *scale, const float *grad_total,
                                float *d_q_logits, float *d_scaled_entropy, void *stream) {
    PgDesc d;
    if (int rc = pg_desc(desc, d, "pigrad_loss_backward")) return rc;
    if (!q_logits || !scale) return fail(TDMPC2_ERR_INVALID, "pigrad_loss_backward: null q_logits or scale");
    const int want = (d_q_logits ? PG_WANT_Q : 0) | (d_scaled_entropy ? PG_WANT_SE : 0);
    if (!want) return fail(TDMPC2_ERR_INVALID, "pigrad_loss_backward: every output is null: nothing to compute");
    PgBwdParams bp{};
    bp.d = d;
    bp.g = pg_bwd_grid(d, want);
    if (int rc = grid_fits(bp.g.first[PG_KINDS], "pigrad_loss_backward")) return rc;
    bp.q_logits = q_logits; bp.scale = scale; bp.grad_total = grad_total; bp.d_q_logits = d_q_logits; bp.d_se = d_scaled_entropy;
    for (int t = 0; t < d.steps; ++t) {
        bp.coef_q[t] = pg_coef_q(d, t);
        bp.coef_se[t] = pg_coef_se(d, t);
    }
    hipLaunchKernelGGL(k_pg_loss_bwd, dim3((uint32_t)bp.g.first[PG_KINDS]), dim3(PG_THREADS), 0, (hipStream_t)stream, bp);
    LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
