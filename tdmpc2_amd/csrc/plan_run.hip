// Host unit of planning.  Reference (nicklashansen/tdmpc2, paths relative to its root):
//   TDMPC2._plan after encode()            tdmpc2/tdmpc2.py:154-206
//   TDMPC2._estimate_value                 tdmpc2/tdmpc2.py:123-136
//   WorldModel.next / reward / pi / Q      tdmpc2/common/world_model.py:114-216
//
// This unit: the host side of the fused 512-wide family (fused_route.h decides; fused_in, launch_setup, launch_pitraj,
// fill_rollout and launch_rollout fill the parameter blocks of k_fused.hip / k_cluster.hip and launch what the route says), run_impl
// and tdmpc2_plan_run, tdmpc2_plan_estimate_value(_trace), tdmpc2_plan_refit, one plan sharded over several GPUs
// (tdmpc2_plan_shard_begin / shard_values / shard_refit) and tdmpc2_plan_export_noise.  The layered family's host side is
// k_layered.hip's (lay_* of launch.h); the refit and noise-export kernels are k_plan.hip's.  Shared services: plan_host.h.
#include "plan_host.h"

namespace {

// What fused_route.h decides from: the handle's scalars and the call's plan count.
FusedIn fused_in(const tdmpc2_plan *h, int E) {
    const tdmpc2_plan_cfg &c = h->cfg;
    FusedIn in{};
    in.E = E; in.tiles = h->tiles; in.N = c.num_samples; in.K = c.num_elites; in.H = c.horizon; in.A = c.action_dim;
    in.P = c.num_pi_trajs; in.num_cus = h->num_cus; in.cluster_mode = h->cluster_mode; in.cl_max_clusters = h->cl_max_clusters;
    in.cl2 = h->cl2_xbuf && h->cl2_mode; in.episodic = c.episodic != 0; in.cl_fault = h->cl_fault != 0;
    in.force_rows = h->force_rows; in.fold_refit = h->fold_refit;
    in.lds_bytes = h->lds_bytes; in.row_bytes = h->row_bytes; in.cl_lds = h->cl_lds;
    return in;
}

// Cluster launches of different streams are serialised per device: a launch whose workgroups are only partly resident
// spins on members that wait for a CU, and two such launches could wait for each other.  (Other kernels may share the
// device: they finish without the cluster's help.)  The lock covers [wait for the previous plan's event, this plan's
// launches, record]; nothing here blocks the host on the GPU.
struct ClusterGate {
    std::mutex mu;
    hipEvent_t ev[64] = {};
    bool have[64] = {};
    hipStream_t last[64] = {};
};
ClusterGate g_cluster_gate;

int launch_setup(tdmpc2_plan *h, const FusedRoute &r, int E, const float *z0, const float *task_emb, const float *prev_mean,
                 const unsigned char *t0, hipStream_t st) {
    SetupParams p{};
    p.E = E; p.H = h->cfg.horizon; p.A = h->cfg.action_dim; p.T = h->cfg.task_dim; p.multitask = h->cfg.multitask;
    p.nq = h->cfg.num_q; p.nnets = h->nnets; p.stride = h->stride; p.max_std = h->cfg.max_std;
    p.dyn = to_dev(h->dyn); p.rew = to_dev(h->rew); p.pi = to_dev(h->pi);
    for (int i = 0; i < h->cfg.num_q; ++i) p.q[i] = to_dev(h->q[i]);
    p.wemb[BE_DYN] = h->dyn.l[0].wemb; p.wemb[BE_REW] = h->rew.l[0].wemb; p.wemb[BE_PI] = h->pi.l[0].wemb;
    for (int i = 0; i < h->cfg.num_q; ++i) p.wemb[BE_Q0 + i] = h->q[i].l[0].wemb;
    p.z0 = z0; p.task_emb = task_emb; p.prev_mean = prev_mean; p.t0 = t0;
    p.beff = h->beff; p.cvec = h->cvec; p.mean = h->mean; p.std = h->std;
    p.cl_flags = r.arm_cl ? h->cl_flags : nullptr;
    p.cl_flag_words = h->tiles * 2 * CL_FLAG_STRIDE;
    p.cl2_flags = r.arm_cl2 ? h->cl2_flags : nullptr;
    p.cl2_flag_words = h->tiles * 4 * CL_FLAG_STRIDE;
    p.skip_cvec = r.skip_cvec ? 1 : 0;
    p.err_clear = h->cl_err_dev;  // word 0 of the error line back to zero, in stream order (fault_fresh)
    fused_ops(h->Apad).setup(h->split ? 0 : 1, p, E, h->lds_bytes, st);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the policy-prior pass of its own (whole plans that do not fold it into the first rollout launch, sharded plans)
int launch_pitraj(tdmpc2_plan *h, const FusedRoute &r, int E, const float *z0, const float *act_mask, const tdmpc2_noise *tape,
                  uint64_t seed, unsigned call, hipStream_t st) {
    const tdmpc2_plan_cfg &c = h->cfg;
    PiTrajParams p{};
    p.E = E; p.N = c.num_samples; p.H = c.horizon; p.A = c.action_dim; p.Apad = h->Apad; p.P = c.num_pi_trajs; p.stride = h->stride;
    p.multitask = c.multitask; p.nnets = h->nnets; p.log_std_min = c.log_std_min; p.log_std_dif = c.log_std_dif;
    p.dyn = to_dev(h->dyn); p.pi = to_dev(h->pi);
    p.z0 = z0; p.beff = h->beff; p.act_mask = act_mask; p.pi_traj_eps = tape ? tape->pi_traj_eps : nullptr;
    p.seed = seed; p.call = call; p.actions = h->actions; p.zscratch = h->zscratch;
    p.zscratch_estride = (long)h->tiles * ROWS * WIDTH;
    fused_ops(h->Apad).pitraj(h->split ? 0 : 1, r.pitraj_nst, p, E, r.pitraj_lds, st);
    HIP_TRY(hipGetLastError());
    return 0;
}

// what every rollout launch of a call shares; the route's row tiles
void fill_rollout(tdmpc2_plan *h, const FusedRoute &r, RolloutParams &p, int E) {
    const tdmpc2_plan_cfg &c = h->cfg;
    p.E = E; p.N = c.num_samples; p.H = c.horizon; p.A = c.action_dim; p.Apad = h->Apad; p.P = c.num_pi_trajs;
    p.stride = h->stride; p.tiles = r.tiles; p.tile_off = r.tile_off; p.nq = c.num_q; p.num_bins = c.num_bins; p.multitask = c.multitask;
    p.nnets = h->nnets; p.log_std_min = c.log_std_min; p.log_std_dif = c.log_std_dif;
    p.dyn = to_dev(h->dyn); p.rew = to_dev(h->rew); p.pi = to_dev(h->pi);
    if (c.episodic) p.term = to_dev(h->term);
    for (int i = 0; i < c.num_q; ++i) p.q[i] = to_dev(h->q[i]);
    p.bins = h->bins; p.beff = h->beff; p.cvec = h->cvec; p.mean = h->mean; p.std = h->std;
    p.actions = h->actions; p.value = h->value; p.zscratch = h->zscratch;
    p.ticket = h->ticket; p.fold_refit = 0;
    p.iters_total = c.iterations;
    p.timing = h->timing;
}
// the per-tile rollout launch of a route (ks_rollout; a trace call runs its tracing instantiation)
int launch_rollout(tdmpc2_plan *h, const FusedRoute &r, const RolloutParams &p, hipStream_t st) {
    fused_ops(h->Apad).rollout(h->split ? 0 : 1, r.nst, h->cfg.episodic != 0, p.trace_tiles || p.trace_scalars, p, r.grid, r.lds, st);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Everything of TDMPC2._plan after encode() (tdmpc2/tdmpc2.py:154-206) on the fused 512-wide path: fused_route_plan decides,
// this launches.
int fused_run(tdmpc2_plan *h, hipStream_t st, int E, const float *z0, const float *task_emb, const float *act_mask,
              const float *disc_pow, float *prev_mean, const uint8_t *t0, int eval_mode, const tdmpc2_noise *tape,
              uint64_t seed, float *action, const tdmpc2_debug *dbg) {
    const tdmpc2_plan_cfg &c = h->cfg;
    const int H = c.horizon, N = c.num_samples, A = c.action_dim, P = c.num_pi_trajs, I = c.iterations;
    const unsigned call = h->call++;
    int rc;
    const FusedRoute r = fused_route_plan(fused_in(h, E));
    const bool cluster = r.kind != FR_TILE;
    if ((rc = launch_setup(h, r, E, z0, task_emb, prev_mean, t0, st))) return rc;
    if (r.pitraj && (rc = launch_pitraj(h, r, E, z0, act_mask, tape, seed, call, st))) return rc;
    RolloutParams rp{};
    fill_rollout(h, r, rp, E);
    rp.z0 = z0; rp.act_mask = act_mask; rp.disc_pow = disc_pow; rp.seed = seed; rp.call = call; rp.given_actions = 0;
    rp.pi_fold = r.pi_fold ? 1 : 0;
    rp.pi_traj_eps = tape ? tape->pi_traj_eps : nullptr;
    rp.cl_xbuf = h->cl_xbuf; rp.cl_flags = h->cl_flags; rp.cl_err = h->cl_err_dev; rp.cl_zs = h->cl_zs;
    rp.cl_fault = h->cl_fault;
    rp.cl2_xbuf = h->cl2_xbuf; rp.cl2_flags = h->cl2_flags; rp.cl2_zs = h->cl2_zs; rp.cl2_mail = h->cl2_mail;
    rp.fold_refit = r.fold ? 1 : 0;
    std::unique_lock<std::mutex> gate;
    bool gate_record = false;
    const int gdev = c.device >= 0 && c.device < 64 ? c.device : 0;
    if (cluster) {
        gate = std::unique_lock<std::mutex>(g_cluster_gate.mu);
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(st, &cap);
        if (cap == hipStreamCaptureStatusNone) {  // (a captured plan replays on one stream: ordered by the graph itself)
            if (!g_cluster_gate.have[gdev]) {
                HIP_TRY(hipEventCreateWithFlags(&g_cluster_gate.ev[gdev], hipEventDisableTiming));
                g_cluster_gate.have[gdev] = true;
                g_cluster_gate.last[gdev] = st;
            } else if (g_cluster_gate.last[gdev] != st) {
                HIP_TRY(hipStreamWaitEvent(st, g_cluster_gate.ev[gdev], 0));
            }
            gate_record = true;
        }
    }
    for (int it = 0; it < I; ++it) {
        rp.iter = it;
        if (tape) {
            rp.sample_eps = tape->sample_eps + (size_t)it * H * (N - P) * A;
            rp.sample_eps_estride = (long)I * H * (N - P) * A;
            rp.pi_eps = tape->pi_eps + (size_t)it * N * A;
            rp.pi_eps_estride = (long)I * N * A;
            rp.qidx = tape->qidx + (size_t)it * 2;
            rp.qidx_estride = (long)I * 2;
        }
        RefitParams &fp = rp.rf;
        fill_refit(h, fp, E, it, eval_mode, h->value, act_mask, tape, seed, call, prev_mean, action, dbg, r.refit_stage,
                   cluster ? h->cl_err_dev : nullptr);
        if (r.fold) {
            fp.regen = 1; fp.P = P; fp.Apad = h->Apad;
            fp.sample_eps = rp.sample_eps; fp.sample_eps_estride = rp.sample_eps_estride;
        }
        if (h->profiling && h->ev_used + 2 <= (int)h->ev.size()) HIP_TRY(hipEventRecord(h->ev[h->ev_used], st));
        if (r.kind == FR_TILE) {
            if ((rc = launch_rollout(h, r, rp, st))) return rc;
        } else {
            if (r.kind == FR_CLUSTER2) cluster_ops(h->Apad).rollout_cl2(rp, r.grid, r.lds, st);
            else cluster_ops(h->Apad).rollout_cl(c.episodic != 0, rp, r.grid, r.lds, st);
            HIP_TRY(hipGetLastError());
        }
        if (h->profiling && h->ev_used + 2 <= (int)h->ev.size()) {
            HIP_TRY(hipEventRecord(h->ev[h->ev_used + 1], st));
            h->ev_used += 2;
        }
        if (!r.fold && (rc = launch_refit(fp, E, N, r.refit_lds, st))) return rc;
        // the per-iteration action dump reads h->actions after the refit (which does not write them)
        if ((rc = dump_actions(h, dbg, E, it, st))) return rc;
    }
    if (gate_record) {
        HIP_TRY(hipEventRecord(g_cluster_gate.ev[gdev], st));
        g_cluster_gate.last[gdev] = st;
    }
    return TDMPC2_OK;
}

// TDMPC2._estimate_value (tdmpc2/tdmpc2.py:122-136) on given action sequences, fused path.
int fused_estimate_value(tdmpc2_plan *h, hipStream_t st, int E, const float *z0, const float *task_emb,
                         const float *act_mask, const float *disc_pow, const float *actions, const float *pi_eps,
                         const int32_t *qidx, float *value, float *trace_tiles, float *trace_scalars) {
    const tdmpc2_plan_cfg &c = h->cfg;
    const int N = c.num_samples, A = c.action_dim;
    int rc;
    const FusedRoute r = fused_route_value(fused_in(h, E), trace_tiles != nullptr || trace_scalars != nullptr);
    // setup needs prev_mean / t0 only for mean/std init, which this entry does not use: feed dummies
    HIP_TRY(hipMemsetAsync(h->mean, 0, (size_t)E * c.horizon * A * 4, st));
    HIP_TRY(hipMemsetAsync(h->value, 1, (size_t)E, st));  // E bytes of ones used as t0 = 1 flags (no warm start read)
    if ((rc = launch_setup(h, r, E, z0, task_emb, h->mean, reinterpret_cast<const unsigned char *>(h->value), st))) return rc;
    RolloutParams rp{};
    fill_rollout(h, r, rp, E);
    rp.z0 = z0; rp.act_mask = act_mask; rp.disc_pow = disc_pow; rp.given_actions = 1; rp.iter = 0;
    rp.actions = const_cast<float *>(actions);
    rp.value = value;
    rp.pi_eps = pi_eps; rp.pi_eps_estride = (long)N * A;
    rp.qidx = qidx; rp.qidx_estride = 2;
    rp.trace_tiles = trace_tiles; rp.trace_scalars = trace_scalars;
    return launch_rollout(h, r, rp, st);
}

}  // namespace

// A whole plan on a handle the caller has entered: the checks, then the family's run.
int tdk::run_impl(tdmpc2_plan *h, int n_envs, const float *z0, const float *task_emb, const float *act_mask, const float *disc_pow,
             float *prev_mean, const uint8_t *t0, int eval_mode, const tdmpc2_noise *tape, uint64_t seed, float *action,
             const tdmpc2_debug *dbg, void *stream) {
    if (h) h->in_shard = false;  // a whole plan on this handle abandons whatever sharded plan was left open (an exception in the caller)
    int rc = validate_envs(h, n_envs);
    if (rc) return rc;
    if (!z0 || !disc_pow || !prev_mean || !t0 || !action) return fail(TDMPC2_ERR_INVALID, "null argument");
    const tdmpc2_plan_cfg &c = h->cfg;
    if (c.multitask && (!task_emb || !act_mask)) return fail(TDMPC2_ERR_INVALID, "multitask plan needs task_emb and act_mask");
    if (!c.multitask) { task_emb = nullptr; act_mask = nullptr; }
    if (tape && (!tape->sample_eps || !tape->pi_eps || !tape->qidx || !tape->gumbel_exp ||
                 (c.num_pi_trajs > 0 && !tape->pi_traj_eps) || (!eval_mode && !tape->final_eps)))
        return fail(TDMPC2_ERR_INVALID, "noise tape has null fields");
    hipStream_t st = (hipStream_t)stream;
    struct SafeOnce {  // TDMPC2_TUNE_SAFE_ONCE covers exactly this plan
        tdmpc2_plan *h;
        ~SafeOnce() { if (h->safe_once) { h->safe_once = false; apply_modes(h); } }
    } once{h};
    if (h->lay.on) {
        if ((rc = fault_fresh(h, st))) return rc;
        return lay_run(h, st, n_envs, z0, task_emb, act_mask, disc_pow, prev_mean, t0, eval_mode, tape, seed, action, dbg);
    }
    return fused_run(h, st, n_envs, z0, task_emb, act_mask, disc_pow, prev_mean, t0, eval_mode, tape, seed, action, dbg);
}

extern "C" {

int tdmpc2_plan_run(tdmpc2_plan_t *h, int n_envs, const float *z0, const float *task_emb, const float *act_mask,
                    const float *disc_pow, float *prev_mean, const uint8_t *t0, int eval_mode, const tdmpc2_noise *tape,
                    uint64_t seed, float *action, const tdmpc2_debug *dbg, void *stream) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    ENTER_ON(h, stream);
    return run_impl(h, n_envs, z0, task_emb, act_mask, disc_pow, prev_mean, t0, eval_mode, tape, seed, action, dbg, stream);
}

int tdmpc2_plan_estimate_value(tdmpc2_plan_t *h, int n_envs, const float *z0, const float *task_emb,
                               const float *act_mask, const float *disc_pow, const float *actions, const float *pi_eps,
                               const int32_t *qidx, float *value, void *stream) {
    return tdmpc2_plan_estimate_value_trace(h, n_envs, z0, task_emb, act_mask, disc_pow, actions, pi_eps, qidx, value,
                                            nullptr, nullptr, stream);
}

int tdmpc2_plan_estimate_value_trace(tdmpc2_plan_t *h, int n_envs, const float *z0, const float *task_emb,
                                     const float *act_mask, const float *disc_pow, const float *actions,
                                     const float *pi_eps, const int32_t *qidx, float *value, float *trace_tiles,
                                     float *trace_scalars, void *stream) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    ENTER_ON(h, stream);
    int rc = validate_envs(h, n_envs);
    if (rc) return rc;
    if (!z0 || !disc_pow || !actions || !pi_eps || !qidx || !value) return fail(TDMPC2_ERR_INVALID, "null argument");
    const tdmpc2_plan_cfg &c = h->cfg;
    if (c.multitask && (!task_emb || !act_mask)) return fail(TDMPC2_ERR_INVALID, "multitask needs task_emb and act_mask");
    if (!c.multitask) { task_emb = nullptr; act_mask = nullptr; }
    hipStream_t st = (hipStream_t)stream;
    const int E = n_envs, N = c.num_samples, A = c.action_dim;
    if ((rc = fault_fresh(h, st))) return rc;
    if (h->lay.on) {
        if (trace_tiles) return fail(TDMPC2_ERR_UNSUPPORTED, "the layered path dumps trace_scalars only");
        if ((rc = lay_setup(h, st, E, task_emb, nullptr, nullptr, false))) return rc;
        if ((rc = lay_cvec(h, st, E, z0))) return rc;
        if ((rc = lay_set_qidx(h, st, E, qidx, 2L, c.num_q, 0, 0, 0, h->lay.qidx))) return rc;
        return lay_estimate_value(h, st, E, z0, act_mask, disc_pow, actions, pi_eps, (long)N * A, h->lay.qidx, 0, 0, 0, value,
                                  trace_scalars);
    }
    return fused_estimate_value(h, st, E, z0, task_emb, act_mask, disc_pow, actions, pi_eps, qidx, value, trace_tiles,
                                      trace_scalars);
}

int tdmpc2_plan_refit(tdmpc2_plan_t *h, int n_envs, float *value, const float *actions, const float *act_mask,
                      float *mean, float *std, float *score, int32_t *elite_idx, void *stream) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    if (n_envs < 1 || n_envs > h->cfg.max_envs) return fail(TDMPC2_ERR_INVALID, "n_envs=%d outside [1, %d]", n_envs, h->cfg.max_envs);
    if (!value || !actions) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    const tdmpc2_plan_cfg &c = h->cfg;
    hipStream_t st = (hipStream_t)stream;
    int refit_stage = 0;
    const size_t refit_lds = refit_lds_bytes(c.num_samples, c.num_elites, c.horizon, c.action_dim, &refit_stage);
    RefitParams fp{};
    fp.Nvalid = c.num_valid_samples; fp.E = n_envs; fp.N = c.num_samples; fp.H = c.horizon; fp.A = c.action_dim; fp.K = c.num_elites; fp.last = 0; fp.stage = refit_stage;
    fp.temperature = c.temperature; fp.min_std = c.min_std; fp.max_std = c.max_std;
    fp.value = value; fp.actions = actions; fp.act_mask = c.multitask ? act_mask : nullptr;
    fp.mean = mean ? mean : h->mean; fp.std = std ? std : h->std; fp.score = score; fp.elite_idx = elite_idx;
    return launch_refit(fp, n_envs, c.num_samples, refit_lds, st);
}

// ---------------------------------------------------------------- one plan sharded over several GPUs (last row)
// The sample rows of every plan are split over the ranks; everything else is replicated: every rank holds the weights, runs
// the identical set-up, draws the identical actions (same tape / same Philox seed) and performs the identical elite
// selection + refit on the all-gathered values.  Per CEM iteration a rank calls shard_values for ITS row range, the host
// all-gathers value[E, N / G] over RCCL (4 KB per plan), and every rank calls shard_refit.  tdmpc2_amd/dist.py drives it.
int tdmpc2_plan_shard_begin(tdmpc2_plan_t *h, int n_envs, const float *z0, const float *task_emb, const float *act_mask,
                            const float *prev_mean, const uint8_t *t0, const tdmpc2_noise *tape, uint64_t seed, void *stream) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    ENTER_ON(h, stream);
    int rc = validate_envs(h, n_envs);
    if (rc) return rc;
    if (!z0 || !prev_mean || !t0) return fail(TDMPC2_ERR_INVALID, "null argument");
    const tdmpc2_plan_cfg &c = h->cfg;
    if (c.multitask && (!task_emb || !act_mask)) return fail(TDMPC2_ERR_INVALID, "multitask plan needs task_emb and act_mask");
    if (!c.multitask) { task_emb = nullptr; act_mask = nullptr; }
    if (tape && c.num_pi_trajs > 0 && !tape->pi_traj_eps) return fail(TDMPC2_ERR_INVALID, "noise tape has null fields");
    hipStream_t st = (hipStream_t)stream;
    const unsigned call = h->call++;
    h->shard_call = call;
    // in_shard: no re-arm between the calls of this plan (fault_clean), word 0 of the error line kept until the final pick.  Set
    // only when the whole prologue has been enqueued: a shard_begin that fails leaves the handle as an ordinary call would.
    struct ShardGuard {
        tdmpc2_plan *h; bool ok;
        ~ShardGuard() { h->in_shard = ok; }
    } guard{h, false};
    const int E = n_envs, P = c.num_pi_trajs;
    if (h->lay.on) {
        if ((rc = fault_fresh(h, st))) return rc;
        if ((rc = lay_setup(h, st, E, task_emb, prev_mean, t0, true))) return rc;
        if ((rc = lay_cvec(h, st, E, z0))) return rc;
        if (P > 0 && (rc = lay_pitraj(h, st, E, z0, act_mask, tape ? tape->pi_traj_eps : nullptr, seed, call))) return rc;
        guard.ok = true;
        return TDMPC2_OK;
    }
    const FusedRoute r = fused_route_shard(fused_in(h, E), 0, c.num_samples);
    if ((rc = launch_setup(h, r, E, z0, task_emb, prev_mean, t0, st))) return rc;
    if (r.pitraj && (rc = launch_pitraj(h, r, E, z0, act_mask, tape, seed, call, st))) return rc;
    guard.ok = true;
    return TDMPC2_OK;
}

int tdmpc2_plan_shard_values(tdmpc2_plan_t *h, int n_envs, int iter, int row_begin, int row_end, const float *z0,
                             const float *act_mask, const float *disc_pow, const tdmpc2_noise *tape, uint64_t seed,
                             float *value, void *stream) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    ENTER_ON(h, stream);
    int rc = validate_envs(h, n_envs);
    if (rc) return rc;
    if (!z0 || !disc_pow || !value) return fail(TDMPC2_ERR_INVALID, "null argument");
    const tdmpc2_plan_cfg &c = h->cfg;
    const int E = n_envs, N = c.num_samples, A = c.action_dim, I = c.iterations;
    if (iter < 0 || iter >= I) return fail(TDMPC2_ERR_INVALID, "iteration %d outside [0, %d)", iter, I);
    const int gran = h->lay.on ? GBM : ROWS;
    if (row_begin < 0 || row_end > N || row_begin >= row_end || row_begin % gran || row_end % gran)
        return fail(TDMPC2_ERR_INVALID, "row range [%d, %d) must be non-empty, inside [0, %d) and aligned to %d rows", row_begin, row_end, N, gran);
    if (c.multitask && !act_mask) return fail(TDMPC2_ERR_INVALID, "multitask plan needs act_mask");
    if (!c.multitask) act_mask = nullptr;
    if (tape && (!tape->sample_eps || !tape->pi_eps || !tape->qidx)) return fail(TDMPC2_ERR_INVALID, "noise tape has null fields");
    hipStream_t st = (hipStream_t)stream;
    const unsigned call = h->shard_call;
    // (1) the actions of ALL rows of this iteration (replicated: the refit needs every elite's actions)
    int *qbuf = h->lay.on ? h->lay.qidx : h->qidx_buf;
    if ((rc = lay_sample_iteration(h, st, E, iter, act_mask, tape, seed, call, qbuf))) return rc;
    const float *pi_eps = tape ? tape->pi_eps + (size_t)iter * N * A : nullptr;
    // (2) this rank's rows
    if (h->lay.on)
        return lay_estimate_value(h, st, E, z0, act_mask, disc_pow, h->actions, pi_eps, (long)I * N * A, qbuf, seed, call, iter, value,
                                  nullptr, row_begin, row_end - row_begin);
    const FusedRoute r = fused_route_shard(fused_in(h, E), row_begin, row_end);
    RolloutParams rp{};
    fill_rollout(h, r, rp, E);
    rp.z0 = z0; rp.act_mask = act_mask; rp.disc_pow = disc_pow; rp.seed = seed; rp.call = call; rp.given_actions = 1; rp.iter = iter;
    rp.value = value; rp.pi_eps = pi_eps; rp.pi_eps_estride = (long)I * N * A; rp.qidx = qbuf; rp.qidx_estride = 2;
    return launch_rollout(h, r, rp, st);
}

int tdmpc2_plan_shard_refit(tdmpc2_plan_t *h, int n_envs, int iter, float *value, const float *act_mask, float *prev_mean,
                            int eval_mode, const tdmpc2_noise *tape, uint64_t seed, float *action, const tdmpc2_debug *dbg,
                            void *stream) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    ENTER_ON(h, stream);
    if (n_envs < 1 || n_envs > h->cfg.max_envs) return fail(TDMPC2_ERR_INVALID, "n_envs=%d outside [1, %d]", n_envs, h->cfg.max_envs);
    if (!value || !prev_mean || !action) return fail(TDMPC2_ERR_INVALID, "null argument");
    const tdmpc2_plan_cfg &c = h->cfg;
    if (iter < 0 || iter >= c.iterations) return fail(TDMPC2_ERR_INVALID, "iteration %d outside [0, %d)", iter, c.iterations);
    if (tape && (!tape->gumbel_exp || (!eval_mode && !tape->final_eps))) return fail(TDMPC2_ERR_INVALID, "noise tape has null fields");
    hipStream_t st = (hipStream_t)stream;
    int stage = 0, rc;
    const size_t lds = refit_lds_bytes(c.num_samples, c.num_elites, c.horizon, c.action_dim, &stage);
    RefitParams fp;
    // err: a bounded inter-workgroup wait (fused NormedLinear epilogue) that gave up in ANY iteration of this sharded plan: NaN
    // action, prev_mean kept -- word 0 is cleared by shard_begin only (in stream order), not by the calls in between
    fill_refit(h, fp, n_envs, iter, eval_mode, value, c.multitask ? act_mask : nullptr, tape, seed, h->shard_call, prev_mean, action, dbg,
               stage, h->cl_err_dev);
    if ((rc = launch_refit(fp, n_envs, c.num_samples, lds, st))) return rc;
    if (fp.last) {
        h->in_shard = false;
        if (h->safe_once) { h->safe_once = false; apply_modes(h); }
    }
    return dump_actions(h, dbg, n_envs, iter, st);
}

int tdmpc2_plan_export_noise(tdmpc2_plan_t *h, int env_first, int n_envs, uint64_t seed, uint32_t call,
                             const tdmpc2_noise_out *out, void *stream) {
    if (!h || !out) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (env_first < 0 || n_envs < 1) return fail(TDMPC2_ERR_INVALID, "environment range [%d, +%d)", env_first, n_envs);
    ENTER_ON(h, stream);
    const tdmpc2_plan_cfg &c = h->cfg;
    NoiseExportArgs p{};
    p.e0 = env_first; p.n = n_envs; p.H = c.horizon; p.N = c.num_samples; p.P = c.num_pi_trajs; p.A = c.action_dim;
    p.K = c.num_elites; p.I = c.iterations; p.nq = c.num_q; p.hp = (c.action_dim + 15) / 16 * 8;
    p.seed = seed; p.call = call; p.o = *out;
    launch_export_noise(p, 2048, 256, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return TDMPC2_OK;
}

}  // extern "C"
