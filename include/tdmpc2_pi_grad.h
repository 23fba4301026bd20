/* Policy loss seeds (tdmpc2_pigrad_*): the arithmetic of TDMPC2.update_pi between its layers (reference tdmpc2/tdmpc2.py:208-239),
 * forward and backward.  A stateless unit beside the planner's ABI (tdmpc2_plan.h, whose version and symbols it leaves as they
 * are), linked into the same libtdmpc2_plan.so: no handle, no allocation, no host synchronisation, no atomics, no wait between
 * workgroups, no environment variable.  Every call is its descriptor and its pointers, ordered by `stream`, and can be captured
 * in a hipGraph.  The MLPs on either side (the policy prior, the two drawn Q heads) are tdmpc2_layer_*; the running scale between
 * value_forward and loss_forward is tdmpc2_plan_running_scale: this unit only reads *scale.
 *
 * T = steps (horizon + 1, 1..16), B = batch, A = action_dim (1..64), NB = num_bins (2..4096).  Every data pointer is contiguous
 * fp32 on the device; the hyperparameters are the fp32 values the caller's doubles round to, widened once on the host.
 *
 *   head_forward    pi_out [T,B,2A] (mean | raw log_std), eps [T,B,A], action_mask [B,A] (non-NULL exactly when multitask)
 *                   -> action [T,B,A], entropy [T,B], scaled_entropy [T,B]: log_std = log_std_min + 0.5 log_std_dif (tanh(raw) + 1);
 *                   mean, log_std, eps times the mask row; log_prob = sum(-0.5 eps^2 - log_std - log(2 pi)/2); scaled = log_prob *
 *                   (A | the mask row's sum); action = tanh(mean + eps exp(log_std)); log_prob -= sum log(relu(1 - action^2) + 1e-6);
 *                   entropy = -log_prob; scaled_entropy = -log_prob * scaled / (log_prob + 1e-8).  One launch, 8 lanes per row.
 *   head_backward   d_action [T,B,A] | NULL, d_scaled_entropy [T,B] | NULL (NULL = zero, not both) -> d_pi_out [T,B,2A]: the
 *                   gradient of that expression (through scaled / (log_prob + 1e-8) too; relu' = 0 where 1 - action^2 <= 0; tanh' =
 *                   1 - y^2).  Nothing is saved by the forward: the row is computed again.  Masked columns get +-0.  One launch.
 *   value_forward   q_logits [2,T,B,NB] -> q [T,B] = (two_hot_inv(head 0) + two_hot_inv(head 1)) / 2.  One launch, one wavefront per
 *                   row pair.
 *   loss_forward    q, entropy, scaled_entropy [T,B], scale (device float[1]) -> losses [3] = pi_loss, mean(entropy),
 *                   mean(scaled_entropy); step_means [T] | NULL = mean_b(entropy_coef scaled_entropy + q / scale).
 *                   pi_loss = mean_t(-step_means[t] rho^t), rho^t = fp32(pow(double(rho), t)).  One workgroup, a fixed order
 *                   of sums (tdmpc2_amd/csrc/pi_grad_route.h).
 *   loss_backward   q_logits, scale, grad_total (device float[1] | NULL = 1) -> d_q_logits [2,T,B,NB] | NULL, d_scaled_entropy [T,B]
 *                   | NULL (not both NULL): d_scaled_entropy = -g fp32(entropy_coef rho^t / (T B)); d_q_logits[i,t,b,k] =
 *                   -g fp32(rho^t / (2 T B)) / scale * symexp'(x_i) * p_k (bin_k - x_i), x_i = sum p_k bin_k, symexp'(x) = exp|x|,
 *                   exactly 0 at x == 0.  The constants are computed in fp64 and rounded once; g is one fp32 factor.  One launch.
 *
 * Non-finite inputs: a NaN in a row of q_logits, pi_out or eps makes NaN that row's outputs and seeds and the scalar losses that
 * sum it; every other row keeps its bits.  A NaN *scale poisons everything that divides by it.  +-Inf logits are not covered.
 *
 * Return codes are tdmpc2_plan.h's (the message: tdmpc2_last_error).  TDMPC2_ERR_INVALID before the device is touched: NULL
 * descriptor or required pointer; steps outside [1,16]; batch < 1; action_dim outside [1,64]; a mask that does not match multitask;
 * a backward with no output or (head) no incoming gradient.  TDMPC2_ERR_UNSUPPORTED, also before the device is touched: num_bins
 * < 2 (regression heads) or > 4096 (the bins of a workgroup live in LDS); a grid past 2^31 workgroups. */
#ifndef TDMPC2_PI_GRAD_H
#define TDMPC2_PI_GRAD_H
#include <stdint.h>

#include "tdmpc2_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tdmpc2_pigrad_desc {
    int32_t steps, batch, action_dim, num_bins, multitask;
    float vmin, vmax, rho, entropy_coef, log_std_min, log_std_dif;
} tdmpc2_pigrad_desc;   /* 44 bytes, no padding */

int tdmpc2_pigrad_head_forward(const tdmpc2_pigrad_desc *d, const float *pi_out, const float *eps, const float *action_mask,
                               float *action, float *entropy, float *scaled_entropy, void *stream);
int tdmpc2_pigrad_head_backward(const tdmpc2_pigrad_desc *d, const float *pi_out, const float *eps, const float *action_mask,
                                const float *d_action, const float *d_scaled_entropy, float *d_pi_out, void *stream);
int tdmpc2_pigrad_value_forward(const tdmpc2_pigrad_desc *d, const float *q_logits, float *q, void *stream);
int tdmpc2_pigrad_loss_forward(const tdmpc2_pigrad_desc *d, const float *q, const float *entropy, const float *scaled_entropy,
                               const float *scale, float *losses, float *step_means, void *stream);
int tdmpc2_pigrad_loss_backward(const tdmpc2_pigrad_desc *d, const float *q_logits, const float *scale, const float *grad_total,
                                float *d_q_logits, float *d_scaled_entropy, void *stream);

#ifdef __cplusplus
}
#endif
#endif
