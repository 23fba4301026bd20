// Host unit of the training forward passes.  Reference (nicklashansen/tdmpc2, paths relative to its root):
//   TDMPC2._td_target                      tdmpc2/tdmpc2.py:242-257
//   TDMPC2._update, forward half           tdmpc2/tdmpc2.py:259-304
//   TDMPC2.update_pi, forward              tdmpc2/tdmpc2.py:208-239 (RunningScale: tdmpc2/common/scale.py)
//
// This unit: the opening and the per-task tables the training calls share (begin_value_call, build_task_tables),
// tdmpc2_plan_policy_value / td_target, tdmpc2_plan_model_rollout / model_losses (model_route.h decides the stages),
// tdmpc2_plan_policy_loss, tdmpc2_plan_running_scale and tdmpc2_plan_termination_stats, each with its multitask twin.  The fused
// family's kernels are k_fused.hip (ks_value), k_model.hip and k_policy_loss.hip; the layered family's stages are k_layered.hip's
// (lay_value, lay_model); ks_task_bias is k_plan.hip's.  Shared services: plan_host.h.
#include "plan_host.h"

namespace {

// The opening the training calls share (policy_value / td_target, model_rollout / model_losses, policy_loss), in this order: the
// task tables against the handle's kind (then `own`: the call's own refusals that sit there), bound weights, the sticky fault word,
// a fresh verdict word, the target ensemble, the call-counter tick.  `needs`: the call's name(s) and verb as the refusal words them.
template <class Own>
int begin_value_call(tdmpc2_plan *h, const char *needs, const tdmpc2_task_tables *tk, bool target, hipStream_t st, unsigned *call,
                     Own own) {
    const tdmpc2_plan_cfg &c = h->cfg;
    if (c.multitask) {
        if (!tk || !tk->task_ids || !tk->task_emb || !tk->act_mask || tk->n_tasks < 1)
            return fail(TDMPC2_ERR_INVALID, "multitask %s the row -> task map and the per-task tables", needs);
    } else if (tk) {
        return fail(TDMPC2_ERR_INVALID, "task tables given to a single-task handle");
    }
    int rc = own();
    if (rc) return rc;
    if ((rc = check_ready(h))) return rc;
    (void)fault_poll(h);  // (a wait that gave up in an earlier call: this one already runs on the paths without waits)
    // between the calls of a sharded plan word 0 is that plan's verdict (its final pick reads it): keep it
    if (!h->in_shard && (rc = fault_fresh(h, st))) return rc;
    if (target)
        for (int i = 0; i < 3; ++i)
            for (int qh = 0; qh < c.num_q; ++qh)
                if (!h->tq[qh].l[i].bound)
                    return fail(TDMPC2_ERR_STATE, "layer %d of target Q head %d is not bound (net TDMPC2_NET_TARGET_Q)", i, qh);
    *call = h->call++;  // (model_rollout / model_losses draw nothing: their tick keeps the siblings' numbering uniform)
    return 0;
}

// per-task tables of a multitask value call: effective first-layer biases of pi and of the chosen Q ensemble, action
// masks, discounts; (re)built on every call (the weights may have been re-bound), storage grown on demand
int build_task_tables(tdmpc2_plan *h, const tdmpc2_task_tables *tk, bool target, size_t rows_p, hipStream_t st, bool all_nets = false) {
    const tdmpc2_plan_cfg &c = h->cfg;
    const int nt = tk->n_tasks;
    const size_t width = h->lay.on ? (size_t)h->lay.Mp : (size_t)WIDTH;
    int rc;
    // (grow_ws: the old tables are released stream-ordered -- earlier calls on `st` are done with them)
    if ((rc = grow_ws(h, &h->tab_tasks, (size_t)nt, {{(void **)&h->beff_tab, (size_t)nt * h->nnets * width * 4},
                                                      {(void **)&h->mask_tab, (size_t)nt * c.action_dim * 4},
                                                      {(void **)&h->disc_tab, (size_t)nt * 4}}, st))) return rc;
    if ((rc = grow_ws(h, &h->task_rows_cap, rows_p, {{(void **)&h->task_rows, rows_p * 4}}, st))) return rc;
    HIP_TRY(hipMemcpyAsync(h->mask_tab, tk->act_mask, (size_t)nt * c.action_dim * 4, hipMemcpyDeviceToDevice, st));
    if (tk->discount) HIP_TRY(hipMemcpyAsync(h->disc_tab, tk->discount, (size_t)nt * 4, hipMemcpyDeviceToDevice, st));
    const HostNet *qarr = target ? h->tq : h->q;
    if (h->lay.on) return lay_setup(h, st, nt, tk->task_emb, nullptr, nullptr, false, h->beff_tab, qarr);
    TaskBiasParams p{};
    p.T = c.task_dim; p.nq = c.num_q; p.nnets = h->nnets; p.task_emb = tk->task_emb; p.beff_tab = h->beff_tab;
    p.wemb[BE_PI] = h->pi.l[0].wemb; p.bias[BE_PI] = h->pi.l[0].bias;
    if (all_nets) {  // model rollout: the dynamics and reward first layers take the row's task as well
        p.wemb[BE_DYN] = h->dyn.l[0].wemb; p.bias[BE_DYN] = h->dyn.l[0].bias;
        p.wemb[BE_REW] = h->rew.l[0].wemb; p.bias[BE_REW] = h->rew.l[0].bias;
    }
    for (int i = 0; i < c.num_q; ++i) { p.wemb[BE_Q0 + i] = qarr[i].l[0].wemb; p.bias[BE_Q0 + i] = qarr[i].l[0].bias; }
    launch_task_bias(p, nt, st);
    HIP_TRY(hipGetLastError());
    return 0;
}

// What ks_value (policy_value / td_target) and ks_value_ent (policy_loss) read alike: the shapes, pi and the Q ensemble, the
// rows, the draws, the outputs and -- after build_task_tables -- the per-task tables.
void fill_value(tdmpc2_plan *h, ValueParams &p, int rows, const float *z, bool target, bool reduce_min, const float *pi_eps,
                const int32_t *qidx, uint64_t seed, unsigned call, const tdmpc2_task_tables *tk, float *action, float *out) {
    const tdmpc2_plan_cfg &c = h->cfg;
    p.rows = rows; p.A = c.action_dim; p.Apad = h->Apad; p.nq = c.num_q; p.num_bins = c.num_bins; p.reduce_min = reduce_min ? 1 : 0;
    p.log_std_min = c.log_std_min; p.log_std_dif = c.log_std_dif;
    p.pi = to_dev(h->pi);
    for (int i = 0; i < c.num_q; ++i) p.q[i] = to_dev(target ? h->tq[i] : h->q[i]);
    p.bins = h->bins; p.z = z; p.pi_eps = pi_eps; p.qidx = qidx; p.seed = seed; p.call = call;
    p.action = action; p.out = out;
    p.nnets = h->nnets;
    if (c.multitask) { p.task_ids = tk->task_ids; p.beff_tab = h->beff_tab; p.mask_tab = h->mask_tab; }
}

int launch_value(tdmpc2_plan *h, int rows, const float *z, bool target, bool reduce_min, const float *pi_eps, const int32_t *qidx,
                 uint64_t seed, const float *reward, const float *terminated, float discount, const tdmpc2_task_tables *tk,
                 float *action, float *out, hipStream_t st) {
    const tdmpc2_plan_cfg &c = h->cfg;
    unsigned call;
    int rc = begin_value_call(h, "policy_value / td_target need", tk, target, st, &call, [&] {
        return c.multitask && reward && !tk->discount ? fail(TDMPC2_ERR_INVALID, "multitask td_target needs the per-task discounts") : 0;
    });
    if (rc) return rc;
    if (h->lay.on) {
        const size_t rows_p = round_up((size_t)rows, GBM), cap = round_up((size_t)c.max_envs * c.num_samples, GBM);
        if (rows_p > cap)
            return fail(TDMPC2_ERR_INVALID, "the layered workspace holds %zu rows (max_envs x num_samples); got %d", cap, rows);
        if (c.multitask) {
            if ((rc = build_task_tables(h, tk, target, rows_p, st))) return rc;
            HIP_TRY(hipMemsetAsync(h->task_rows, 0, rows_p * 4, st));
            HIP_TRY(hipMemcpyAsync(h->task_rows, tk->task_ids, (size_t)rows * 4, hipMemcpyDeviceToDevice, st));
        }
        // the two heads: given, or randperm(num_q)[:2] once per call (world_model.py:212)
        if ((rc = lay_set_qidx(h, st, 1, qidx, 2L, c.num_q, 0, seed, call, h->lay.qidx))) return rc;
        return lay_value(h, st, rows, z, target, reduce_min, pi_eps, h->lay.qidx, seed, call, reward, terminated, discount,
                         c.multitask ? h->task_rows : nullptr, action, out);
    }
    if (c.multitask && (rc = build_task_tables(h, tk, target, 0, st))) return rc;
    ValueParams p{};
    fill_value(h, p, rows, z, target, reduce_min, pi_eps, qidx, seed, call, tk, action, out);
    p.discount = discount; p.reward = reward; p.terminated = terminated;
    if (c.multitask) p.disc_tab = reward ? h->disc_tab : nullptr;
    const int grid = (rows + ROWS - 1) / ROWS;
    const size_t lds = h->lds_bytes;
    const int ar = h->split ? 0 : 1;
    fused_ops(h->Apad).value(ar, p, grid, lds, st);
    HIP_TRY(hipGetLastError());
    return 0;
}
}  // namespace

extern "C" {

int tdmpc2_plan_policy_value_mt(tdmpc2_plan_t *h, int n_rows, const float *z, const tdmpc2_task_tables *tasks, int use_target,
                                int reduce_min, const float *pi_eps, const int32_t *qidx, uint64_t seed, float *action, float *q,
                                void *stream) {
    if (!h || !z || !q) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n_rows < 1) return fail(TDMPC2_ERR_INVALID, "n_rows %d < 1", n_rows);
    ENTER_ON(h, stream);
    return launch_value(h, n_rows, z, use_target != 0, reduce_min != 0, pi_eps, qidx, seed, nullptr, nullptr, 0.f, tasks, action, q,
                        (hipStream_t)stream);
}

int tdmpc2_plan_policy_value(tdmpc2_plan_t *h, int n_rows, const float *z, int use_target, int reduce_min, const float *pi_eps,
                             const int32_t *qidx, uint64_t seed, float *action, float *q, void *stream) {
    return tdmpc2_plan_policy_value_mt(h, n_rows, z, nullptr, use_target, reduce_min, pi_eps, qidx, seed, action, q, stream);
}

int tdmpc2_plan_td_target_mt(tdmpc2_plan_t *h, int n_rows, const float *next_z, const float *reward, const float *terminated,
                             float discount, const tdmpc2_task_tables *tasks, const float *pi_eps, const int32_t *qidx,
                             uint64_t seed, float *td, void *stream) {
    if (!h || !next_z || !reward || !terminated || !td) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n_rows < 1) return fail(TDMPC2_ERR_INVALID, "n_rows %d < 1", n_rows);
    ENTER_ON(h, stream);
    return launch_value(h, n_rows, next_z, true, true, pi_eps, qidx, seed, reward, terminated, discount, tasks, nullptr, td,
                        (hipStream_t)stream);
}

int tdmpc2_plan_td_target(tdmpc2_plan_t *h, int n_rows, const float *next_z, const float *reward, const float *terminated,
                          float discount, const float *pi_eps, const int32_t *qidx, uint64_t seed, float *td, void *stream) {
    return tdmpc2_plan_td_target_mt(h, n_rows, next_z, reward, terminated, discount, nullptr, pi_eps, qidx, seed, td, stream);
}

// ---------------------------------------------------------------- model rollout + losses: the forward half of TDMPC2._update
// (tdmpc2/tdmpc2.py:259-304).  model_route.h decides the stages; the fused family launches ks_value_roll / ks_value_chain
// (k_model.hip), the layered family its GEMM chains (lay_model); the loss rows and the fixed-order tail are shared.
namespace {
int launch_model(tdmpc2_plan *h, int B, int H, const float *z0, const float *actions, bool target, const tdmpc2_task_tables *tk,
                 const tdmpc2_model_targets *tg, const tdmpc2_model_out *out, float *losses, float *step_means, hipStream_t st) {
    const tdmpc2_plan_cfg &c = h->cfg;
    static const tdmpc2_model_out none{};
    if (!out) out = &none;
    unsigned want = 0;
    if (out->zs) want |= MW_ZS;
    if (out->reward_logits) want |= MW_REW_LOGITS;
    if (out->reward) want |= MW_REW;
    if (out->q_logits) want |= MW_Q_LOGITS;
    if (out->q) want |= MW_Q;
    if (out->term_logit) want |= MW_TERM;
    if (tg) want |= MW_LOSSES;
    if (tg && c.num_bins < 2) return fail(TDMPC2_ERR_UNSUPPORTED, "model_losses needs two-hot heads (num_bins %d: the reference's soft_ce is identically 0)", c.num_bins);
    if (tg && tg->terminated && !c.episodic) return fail(TDMPC2_ERR_INVALID, "`terminated` given to a non-episodic handle");
    const size_t cap = round_up((size_t)c.max_envs * c.num_samples, GBM);
    const ModelRoute r = model_route(ModelIn{h->lay.on ? MODEL_LAYERED : MODEL_FUSED, B, H, c.num_q, c.num_bins, c.episodic, want, (long)cap,
                                                 (h->split && h->lay.fuse_ln) ? 0 : 1});
    switch (r.refuse) {
        case MR_OK: break;
        case MR_BAD_H: return fail(TDMPC2_ERR_INVALID, "steps %d outside [0, %d]", H, MAXH);
        case MR_BAD_B: return fail(TDMPC2_ERR_INVALID, "batch %d < 1", B);
        case MR_LOSSES_H0: return fail(TDMPC2_ERR_INVALID, "model_losses needs at least one step");
        case MR_NOT_EPISODIC: return fail(TDMPC2_ERR_INVALID, "term_logit asked of a non-episodic handle");
        case MR_ROWS: return fail(TDMPC2_ERR_INVALID, "the layered workspace holds %zu rows (max_envs x num_samples); got batch x steps = %d x %d", cap, B, H);
        default: return fail(TDMPC2_ERR_UNSUPPORTED, "model_losses needs two-hot heads (num_bins %d)", c.num_bins);
    }
    if (H > 0 && !actions) return fail(TDMPC2_ERR_INVALID, "null actions");
    if (tg) {
        if (!tg->next_z || !tg->reward || !tg->td_target || !losses) return fail(TDMPC2_ERR_INVALID, "null target / losses argument");
        if (c.episodic && !tg->terminated) return fail(TDMPC2_ERR_INVALID, "episodic handle: `terminated` is required");
    }
    unsigned call;
    int rc = begin_value_call(h, "model_rollout / model_losses need", tk, target, st, &call, [] { return 0; });
    if (rc) return rc;
    const size_t Ld = (size_t)c.latent_dim, HB = (size_t)H * B;
    if (r.launches == 0) {  // H = 0 and no termination logit: zs[0] = z0 is all there is
        if (out->zs && out->zs != z0) HIP_TRY(hipMemcpyAsync(out->zs, z0, (size_t)B * Ld * 4, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    float *zs = out->zs;
    if (!zs) {
        if ((rc = grow_ws(h, &h->model_zs, &h->model_zs_cap, (size_t)(H + 1) * B * Ld, st))) return rc;
        zs = h->model_zs;
    }
    if (tg && (rc = grow_ws(h, &h->model_rowloss, &h->model_rowloss_cap, (size_t)model_rowloss_floats(B, H, c.num_q), st))) return rc;
    const size_t trows = (size_t)(H + 1) * B, trows_p = round_up(trows, GBM);
    if (c.multitask) {
        if ((rc = build_task_tables(h, tk, target, h->lay.on ? trows_p : 0, st, true))) return rc;
        if (h->lay.on && (rc = model_launch_tile_tasks(tk->task_ids, B, (int)trows, (int)trows_p, h->task_rows, st))) return rc;
    }
    if (zs != z0) HIP_TRY(hipMemcpyAsync(zs, z0, (size_t)B * Ld * 4, hipMemcpyDeviceToDevice, st));
    ModelLossArgs ls{};
    ls.num_bins = c.num_bins; ls.vmin = c.vmin; ls.vmax = c.vmax;
    ls.bin_size = c.num_bins > 1 ? (float)(((double)c.vmax - (double)c.vmin) / (c.num_bins - 1)) : 1.f;  // parser.py: cfg.bin_size
    ls.bins = h->bins; ls.HB = (long)HB;
    if (tg) { ls.t_reward = tg->reward; ls.t_td = tg->td_target; ls.t_term = tg->terminated; ls.rowloss = h->model_rowloss; }
    const ModelOutArgs oa{out->reward_logits, out->reward, out->q_logits, out->q, out->term_logit};
    if (h->lay.on) {
        if ((rc = lay_model(h, st, r, B, H, actions, zs, target, c.multitask ? h->task_rows : nullptr, oa, ls))) return rc;
    } else {
        ModelParams p{};
        p.B = B; p.H = H; p.A = c.action_dim; p.Apad = h->Apad; p.nq = c.num_q; p.nnets = h->nnets; p.steps = r.st[MS_DYN].steps;
        p.dyn = to_dev(h->dyn); p.rew = to_dev(h->rew);
        if (c.episodic) p.term = to_dev(h->term);
        for (int i = 0; i < c.num_q; ++i) p.q[i] = to_dev(target ? h->tq[i] : h->q[i]);
        p.z0 = z0; p.actions = actions; p.zs = zs; p.out = oa; p.ls = ls;
        if (c.multitask) { p.task_ids = tk->task_ids; p.beff_tab = h->beff_tab; }
        const int ar = h->split ? 0 : 1;
        const ModelOps &ops = model_ops(h->Apad);
        if (r.st[MS_DYN].run) {
            ops.dyn(ar, p, r.st[MS_DYN].gx, h->lds_bytes, st);
            HIP_TRY(hipGetLastError());
        }
        if (r.st[MS_HEADS].run) {
            for (int k = 0; k < r.nchain; ++k) p.chain[k] = r.chain[k];
            ops.chain(ar, p, r.st[MS_HEADS].gx, r.st[MS_HEADS].gy, r.st[MS_HEADS].gz, h->lds_bytes, st);
            HIP_TRY(hipGetLastError());
        }
        if (r.st[MS_TERM].run) {
            p.chain[0] = MC_TERM;
            ops.chain(ar, p, r.st[MS_TERM].gx, r.st[MS_TERM].gy, 1, h->lds_bytes, st);
            HIP_TRY(hipGetLastError());
        }
    }
    if (!tg) return 0;
    const unsigned int *err = (h->lay.on && h->split && h->lay.fuse_ln) ? h->cl_err_dev : nullptr;
    ModelConsParams cp{zs + (size_t)B * Ld, tg->next_z, (int)HB, c.latent_dim, h->model_rowloss};
    if ((rc = model_launch_cons(cp, r.st[MS_CONS].gx, st))) return rc;
    ModelTailParams tp{};
    tp.rowloss = h->model_rowloss; tp.B = B; tp.H = H; tp.L = c.latent_dim; tp.nq = c.num_q; tp.episodic = c.episodic;
    for (int t = 0; t < H; ++t) tp.rho_pow[t] = (float)std::pow((double)tg->rho, t);
    tp.coef[0] = tg->consistency_coef; tp.coef[1] = tg->reward_coef; tp.coef[2] = tg->value_coef; tp.coef[3] = tg->termination_coef;
    tp.losses = losses; tp.step_means = step_means; tp.err = err;
    return model_launch_tail(tp, st);
}
}  // namespace

int tdmpc2_plan_model_rollout_mt(tdmpc2_plan_t *h, int batch, int steps, const float *z0, const float *actions,
                                 const tdmpc2_task_tables *tasks, int use_target, const tdmpc2_model_out *out, void *stream) {
    if (!h || !z0 || !out) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    return launch_model(h, batch, steps, z0, actions, use_target != 0, tasks, nullptr, out, nullptr, nullptr, (hipStream_t)stream);
}
int tdmpc2_plan_model_rollout(tdmpc2_plan_t *h, int batch, int steps, const float *z0, const float *actions, int use_target,
                              const tdmpc2_model_out *out, void *stream) {
    return tdmpc2_plan_model_rollout_mt(h, batch, steps, z0, actions, nullptr, use_target, out, stream);
}
int tdmpc2_plan_model_losses_mt(tdmpc2_plan_t *h, int batch, int steps, const float *z0, const float *actions,
                                const tdmpc2_task_tables *tasks, int use_target, const tdmpc2_model_targets *targets,
                                const tdmpc2_model_out *out, float *losses, float *step_means, void *stream) {
    if (!h || !z0 || !targets || !losses) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    return launch_model(h, batch, steps, z0, actions, use_target != 0, tasks, targets, out, losses, step_means, (hipStream_t)stream);
}
int tdmpc2_plan_model_losses(tdmpc2_plan_t *h, int batch, int steps, const float *z0, const float *actions, int use_target,
                             const tdmpc2_model_targets *targets, const tdmpc2_model_out *out, float *losses, float *step_means,
                             void *stream) {
    return tdmpc2_plan_model_losses_mt(h, batch, steps, z0, actions, nullptr, use_target, targets, out, losses, step_means, stream);
}

// ---------------------------------------------------------------- policy loss: the forward of TDMPC2.update_pi (tdmpc2/tdmpc2.py:208-239)
// ks_value_ent (pi + two online Q heads + the entropy terms, per row into the handle's workspace), then one workgroup each for
// RunningScale.update on q[0] and for the fixed-order tail.
namespace {
int launch_policy_loss(tdmpc2_plan *h, int B, int steps, const float *zs, const tdmpc2_task_tables *tk, const float *pi_eps,
                       const int32_t *qidx, uint64_t seed, const tdmpc2_policy_loss_in *in, float *scale,
                       const tdmpc2_policy_loss_out *out, float *loss, hipStream_t st) {
    const tdmpc2_plan_cfg &c = h->cfg;
    static const tdmpc2_policy_loss_out none{};
    if (!out) out = &none;
    if (B < 1) return fail(TDMPC2_ERR_INVALID, "batch %d < 1", B);
    if (steps < 0 || steps > PL_MAX_STEPS) return fail(TDMPC2_ERR_INVALID, "steps %d outside [0, %d]", steps, (int)PL_MAX_STEPS);
    unsigned call;
    int rc = begin_value_call(h, "policy_loss needs", tk, false, st, &call, [&] {
        return in->update_scale && B > PL_SCALE_MAX_N
                   ? fail(TDMPC2_ERR_UNSUPPORTED, "the running scale takes at most %d values; got batch %d", (int)PL_SCALE_MAX_N, B) : 0;
    });
    if (rc) return rc;
    const int T = steps + 1;
    const size_t rows = (size_t)T * B;
    if ((rc = grow_ws(h, &h->ploss_rows, &h->ploss_rows_cap, 3 * rows, st))) return rc;
    float *wq = h->ploss_rows, *went = wq + rows, *wsent = went + rows;
    const unsigned int *err = nullptr;
    if (h->lay.on) {
        // LAYERED: pi, then the two heads, as lay_value runs them -- in pieces of the workspace's rows (max_envs x num_samples) when
        // the call has more; the two heads are drawn once, and a row's noise index is its row in the call, whatever the pieces
        const size_t cap = round_up((size_t)c.max_envs * c.num_samples, GBM), rows_p = round_up(rows, GBM);
        if (c.multitask) {
            if ((rc = build_task_tables(h, tk, false, rows_p, st))) return rc;
            if ((rc = model_launch_tile_tasks(tk->task_ids, B, (int)rows, (int)rows_p, h->task_rows, st))) return rc;
        }
        if ((rc = lay_set_qidx(h, st, 1, qidx, 2L, c.num_q, 0, seed, call, h->lay.qidx))) return rc;
        for (size_t r0 = 0; r0 < rows; r0 += cap) {
            const int n = (int)std::min(cap, rows - r0);
            if ((rc = lay_value(h, st, n, zs + r0 * c.latent_dim, false, false, pi_eps, h->lay.qidx, seed, call, nullptr, nullptr, 0.f,
                                c.multitask ? h->task_rows + r0 : nullptr, out->action ? out->action + r0 * c.action_dim : nullptr,
                                wq + r0, (int)r0, went + r0, wsent + r0))) return rc;
        }
        err = (h->split && h->lay.fuse_ln) ? h->cl_err_dev : nullptr;
    } else {
        if (c.multitask && (rc = build_task_tables(h, tk, false, 0, st))) return rc;
        ValueEntParams p{};
        fill_value(h, p, (int)rows, zs, false, false, pi_eps, qidx, seed, call, tk, out->action, wq);
        p.entropy = went; p.scaled_entropy = wsent;
        if (c.multitask) p.task_mod = B;
        policy_loss_ops(h->Apad).value_ent(h->split ? 0 : 1, p, (int)((rows + ROWS - 1) / ROWS), h->lds_bytes, st);
        HIP_TRY(hipGetLastError());
    }
    if (in->update_scale && (rc = pl_launch_scale(RunningScaleParams{wq, B, in->tau, scale, out->percentiles, err}, st))) return rc;
    PolicyLossTailParams tp{};
    tp.q = wq; tp.entropy = went; tp.scaled_entropy = wsent; tp.scale = scale; tp.B = B; tp.T = T; tp.entropy_coef = in->entropy_coef;
    for (int t = 0; t < T; ++t) tp.rho_pow[t] = std::pow(in->rho, (float)t);  // torch.pow(rho, arange) in fp32 (tdmpc2.py:227)
    tp.step_means = out->step_means; tp.loss = loss; tp.err = err;
    tp.action = out->action; tp.A = c.action_dim;
    if ((rc = pl_launch_tail(tp, st))) return rc;
    if (out->q) HIP_TRY(hipMemcpyAsync(out->q, wq, rows * 4, hipMemcpyDeviceToDevice, st));
    if (out->entropy) HIP_TRY(hipMemcpyAsync(out->entropy, went, rows * 4, hipMemcpyDeviceToDevice, st));
    if (out->scaled_entropy) HIP_TRY(hipMemcpyAsync(out->scaled_entropy, wsent, rows * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}
}  // namespace

int tdmpc2_plan_policy_loss_mt(tdmpc2_plan_t *h, int batch, int steps, const float *zs, const tdmpc2_task_tables *tasks,
                               const float *pi_eps, const int32_t *qidx, uint64_t seed, const tdmpc2_policy_loss_in *in,
                               float *scale, const tdmpc2_policy_loss_out *out, float *loss, void *stream) {
    if (!h || !zs || !in || !scale || !loss) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    return launch_policy_loss(h, batch, steps, zs, tasks, pi_eps, qidx, seed, in, scale, out, loss, (hipStream_t)stream);
}
int tdmpc2_plan_policy_loss(tdmpc2_plan_t *h, int batch, int steps, const float *zs, const float *pi_eps, const int32_t *qidx,
                            uint64_t seed, const tdmpc2_policy_loss_in *in, float *scale, const tdmpc2_policy_loss_out *out,
                            float *loss, void *stream) {
    return tdmpc2_plan_policy_loss_mt(h, batch, steps, zs, nullptr, pi_eps, qidx, seed, in, scale, out, loss, stream);
}
int tdmpc2_plan_running_scale(tdmpc2_plan_t *h, int n, const float *x, float tau, float *scale, float *percentiles, void *stream) {
    if (!h || !x || !scale) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n < 1) return fail(TDMPC2_ERR_INVALID, "n %d < 1", n);
    if (n > PL_SCALE_MAX_N) return fail(TDMPC2_ERR_UNSUPPORTED, "the running scale takes at most %d values; got %d", (int)PL_SCALE_MAX_N, n);
    ENTER_ON(h, stream);
    return pl_launch_scale(RunningScaleParams{x, n, tau, scale, percentiles, nullptr}, (hipStream_t)stream);
}
int tdmpc2_plan_termination_stats(tdmpc2_plan_t *h, int n, const float *term_logit, const float *terminated, float *stats,
                                  void *stream) {
    if (!h || !term_logit || !terminated || !stats) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n < 1) return fail(TDMPC2_ERR_INVALID, "n %d < 1", n);
    ENTER_ON(h, stream);
    return pl_launch_term_stats(TerminationStatsParams{term_logit, terminated, n, stats}, (hipStream_t)stream);
}

}  // extern "C"
