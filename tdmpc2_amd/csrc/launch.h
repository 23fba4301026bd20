// Launcher interfaces between the translation units of libtdmpc2_plan.so (see common.cuh).  A kernel family is instantiated
// in exactly one translation unit; everything else reaches it through these functions / tables.
#pragma once
#include "handle.h"
#include "encoder_params.h"  // state encoder (k_plan.hip: encoder_kernels.cuh)
#include "pixel_batch_route.h"
#include "policy_route.h"
#include "seed_route.h"  // at file scope before refresh_route.h (below, inside tdk) includes it for its __host__ / __device__ shim

// ---- policy prior (k_policy.hip: policy_kernels.cuh, routes in policy_route.h)
struct PolLayerDev {
    const float *wt, *bias, *g, *b;  // [in][out] weights, bias, LayerNorm affine (g / b unused by the output layer)
    int in, out;
};
struct PolHeadArgs {
    int A, row0, eval_mode;   // row0: row index of this launch's first row in the call (Philox key)
    float lmin, ldif;         // log_std_min, log_std_dif
    const float *mask, *eps;  // [n, A] each, or null (single-task / in-kernel draws)
    unsigned long long seed;
    unsigned call;
    float *action, *mean, *log_std, *entropy, *scaled_entropy, *eps_out;  // all but action may be null
};
struct PolRowParams {
    PolLayerDev enc[6];  // acting: the encoder's layers (enc_nl > 0), else z is the input
    int enc_nl, obs_dim;
    const float *obs;    // [n, obs_dim]
    const float *z;      // [n, L] (enc_nl == 0)
    const float *task_emb;  // [n, T] or null
    int L, T, maxw, simnorm_dim;
    PolLayerDev pi[3];
    PolHeadArgs head;
};
struct PolGemvParams {
    const float *wt, *bias;  // [in][out], [out]
    const float *x;          // [n, ldx] activations, or null: layer 0 reads z [n, L] | emb [n, T]
    const float *z, *emb;
    int ldx, L, T, in, out, n;
    float *y;                // [n, out]
};
struct PolHeadParams {
    const float *y;  // [n, 2A] output-layer pre-activations
    PolHeadArgs head;
};

// Kernel parameter types.  The state encoder's, the pixel planning routes' and the noise export's kernels were written with their
// parameter blocks beside them, inside their unit's anonymous namespace, and a kernel's symbol carries its parameter type's
// namespace.  The blocks the host fills are the *Args below (and encoder_params.h's); a kernel unit derives its own empty
// `struct XParams : XArgs {}` from them, so those kernels keep their symbols -- what tools/isa_digest.py and recorded profiles
// key on -- and their code.
// ---- pixel encoder, planning routes (k_plan.hip: pixel_kernels.cuh, routes in pixel_route.h)
struct PixArgs {
    const float *wp[PIX_LAYERS];    // [cin][k][k][C] re-packed Conv2d weights
    const float *bias[PIX_LAYERS];  // [C]
    const void *obs;                // [E, cin, 64, 64] uint8 (obs_u8) or fp32
    int obs_u8, cin, C;
    const int32_t *shift;           // [E, 2] (dx, dy), clamped to [0, 6] in the kernels
    const PixTap *tab;              // [PIX_SHIFTS][PIX_IN]
    float *ws;                      // spread route: [E][pix_ws_floats(C)] outputs of layers 0..2
    float *z;                       // [E, 16 C]
};

// ---- the in-kernel generator as a noise tape (k_export_noise, k_plan.hip; tdmpc2_plan_export_noise): environments [e0, e0 + n)
struct NoiseExportArgs {
    int e0, n, H, N, P, A, K, I, nq, hp;
    unsigned long long seed;
    unsigned int call;
    tdmpc2_noise_out o;
};

// ---- pixel encoder, batch route (k_pixel_batch.hip: pixel_batch_kernels.cuh, decisions in pixel_batch_route.h)
struct PixbParams {
    const float *wp[PIX_LAYERS];    // [cin][k][k][C] re-packed Conv2d weights (the planning routes' copy)
    const float *bias[PIX_LAYERS];  // [C]
    const void *obs;                // this pass's images: [n, cin, 64, 64] uint8 or fp32
    int cin, C, n;
    const int32_t *shift;           // [n, 2] (dx, dy), clamped to [0, 6] in the kernel
    const PixTap *tab;              // [PIX_SHIFTS][PIX_IN]
    float *ws;                      // [chunk][pix_ws_floats(C)] outputs of layers 0..2
    float *z;                       // [n, 16 C]
};

namespace tdk {

// the refusal of a launch whose grid would not fit a dim3's x (used with LAUNCH_CHECK of handle.h)
inline int grid_fits(uint64_t blocks, const char *what) {
    if (blocks > 0x7fffffffull) return fail(TDMPC2_ERR_UNSUPPORTED, "%s: more than 2^31 workgroups in one launch", what);
    return 0;
}

#include "model_params.h"  // model rollout / losses (k_model.hip, model_layered.cuh in k_layered.hip)

// ---- fused 512-wide family: one table per action padding (k_fused.hip, compiled once per -DTU_APAD=16|32|48|64).
// ar: 0 = f16x2 split, 1 = exact fp32 MFMA; nst: 32-row sample tiles per workgroup (1 | 2).
struct FusedOps {
    void (*setup)(int ar, const SetupParams &p, int E, size_t lds, hipStream_t st);
    void (*pitraj)(int ar, int nst, const PiTrajParams &p, int E, size_t lds, hipStream_t st);
    void (*rollout)(int ar, int nst, int ep, int tracing, const RolloutParams &p, int grid, size_t lds, hipStream_t st);
    void (*value)(int ar, const ValueParams &p, int grid, size_t lds, hipStream_t st);
    int (*set_lds)(int ar, int episodic, size_t lds_bytes);  // hipFuncAttributeMaxDynamicSharedMemorySize of every instantiation
};
// ---- cluster path of the fused family (k_cluster.hip, per action padding; split arithmetic only)
struct ClusterOps {
    void (*rollout_cl)(int ep, const RolloutParams &p, int grid, size_t lds, hipStream_t st);
    int (*set_lds)(int episodic, size_t lds_bytes);
    // two clusters per 32-row tile (reward chain beside the dynamics chain): single non-episodic plans, every launch (launch 0 with the policy-prior fold)
    void (*rollout_cl2)(const RolloutParams &p, int grid, size_t lds, hipStream_t st);
};
// (accessor functions, not global tables: hipcc would emit a constant-initialised table on the device side as well)
const FusedOps &fused_ops_ap16(); const FusedOps &fused_ops_ap32(); const FusedOps &fused_ops_ap48(); const FusedOps &fused_ops_ap64();
const ClusterOps &cluster_ops_ap16(); const ClusterOps &cluster_ops_ap32(); const ClusterOps &cluster_ops_ap48(); const ClusterOps &cluster_ops_ap64();

template <typename K>
inline int set_lds(K kernel, size_t bytes) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

// ---- state encoder (k_plan.hip): the host computes grid, block and LDS and checks hipGetLastError after a call's launches
void enc_launch_encode(const EncodeArgs &p, int grid, int threads, size_t lds, hipStream_t st);
void enc_launch_gemv(const EncGemvArgs &p, int gx, int gy, int threads, size_t lds, hipStream_t st);
void enc_launch_norm(const EncNormArgs &p, int grid, int threads, hipStream_t st);  // (the policy prior's spread route as well)
// ---- pixel encoder, planning routes (k_plan.hip); checked by the host like the state encoder's
void pix_launch_image(const PixArgs &p, const PixGrid &g, hipStream_t st);
void pix_launch_spread(int layer, const PixArgs &p, const PixGrid &g, hipStream_t st);  // (static LDS only)
void pix_launch_pack(const float *w, float *wp, int C, int cin, int kk, int grid, int threads, hipStream_t st);
// ---- per-task first-layer biases of the fused family's value calls, and the noise export (k_plan.hip); checked by the host
void launch_task_bias(const TaskBiasParams &p, int n_tasks, hipStream_t st);
void launch_export_noise(const NoiseExportArgs &p, int grid, int threads, hipStream_t st);

// ---- elite selection + refit, one workgroup per plan (k_refit, k_plan.hip)
int launch_refit(const RefitParams &fp, int E, int N, size_t lds, hipStream_t st);
// The refit of CEM iteration `it` of a plan (both families, whole and sharded plans).  err: the handle's error word where the
// plan ran kernels with bounded waits (the final pick then returns NaN and keeps prev_mean), else null.
inline void fill_refit(const tdmpc2_plan *h, RefitParams &fp, int E, int it, int eval_mode, float *value, const float *act_mask,
                       const tdmpc2_noise *tape, uint64_t seed, unsigned call, float *prev_mean, float *action,
                       const tdmpc2_debug *dbg, int stage, const unsigned int *err) {
    const tdmpc2_plan_cfg &c = h->cfg;
    const int H = c.horizon, N = c.num_samples, A = c.action_dim, K = c.num_elites, I = c.iterations;
    fp = RefitParams{};
    fp.Nvalid = c.num_valid_samples; fp.E = E; fp.N = N; fp.H = H; fp.A = A; fp.K = K; fp.iter = it; fp.last = (it == I - 1); fp.eval_mode = eval_mode; fp.stage = stage;
    fp.temperature = c.temperature; fp.min_std = c.min_std; fp.max_std = c.max_std;
    fp.value = value; fp.actions = h->actions; fp.act_mask = act_mask; fp.mean = h->mean; fp.std = h->std;
    fp.gumbel_exp = tape ? tape->gumbel_exp : nullptr; fp.final_eps = tape ? tape->final_eps : nullptr;
    fp.seed = seed; fp.call = call; fp.prev_mean = prev_mean; fp.action = action;
    fp.err = err;
    if (dbg) {
        if (dbg->value) { fp.dbg_value = dbg->value + (size_t)it * N; fp.dbg_value_es = (long)I * N; }
        if (dbg->elite_idx) { fp.dbg_idx = dbg->elite_idx + (size_t)it * K; fp.dbg_idx_es = (long)I * K; }
        if (dbg->score) { fp.dbg_score = dbg->score + (size_t)it * K; fp.dbg_score_es = (long)I * K; }
        if (dbg->mean) { fp.dbg_mean = dbg->mean + (size_t)it * H * A; fp.dbg_mean_es = (long)I * H * A; }
        if (dbg->std) { fp.dbg_std = dbg->std + (size_t)it * H * A; fp.dbg_std_es = (long)I * H * A; }
    }
}
// the per-iteration action dump of a debug call: h->actions [E,H,N,A] -> dbg->actions [E,I,H,N,A] at iteration `it`
inline int dump_actions(const tdmpc2_plan *h, const tdmpc2_debug *dbg, int E, int it, hipStream_t st) {
    if (!dbg || !dbg->actions) return 0;
    const size_t hna = (size_t)h->cfg.horizon * h->cfg.num_samples * h->cfg.action_dim;
    HIP_TRY(hipMemcpy2DAsync(dbg->actions + (size_t)it * hna, (size_t)h->cfg.iterations * hna * 4, h->actions, hna * 4, hna * 4, E,
                             hipMemcpyDeviceToDevice, st));
    return 0;
}

// ---- layer-at-a-time family (k_layered.hip: kernels + their host orchestration, layered_host.cuh)
int lay_setup(tdmpc2_plan *h, hipStream_t st, int E, const float *task_emb, const float *prev_mean, const unsigned char *t0,
              bool init_dist, float *beff_out = nullptr, const HostNet *qarr = nullptr);
int lay_cvec(tdmpc2_plan *h, hipStream_t st, int E, const float *z0);
int lay_pitraj(tdmpc2_plan *h, hipStream_t st, int E, const float *z0, const float *act_mask, const float *tape_eps,
               unsigned long long seed, unsigned call);
int lay_estimate_value(tdmpc2_plan *h, hipStream_t st, int E, const float *z0, const float *act_mask, const float *disc_pow,
                       const float *actions, const float *pi_eps, long pi_eps_estride, const int *qidx /* dense [E,2] */,
                       unsigned long long seed, unsigned call, int iter, float *value, float *trace, int n_off = 0, int n_sub = 0);
int lay_run(tdmpc2_plan *h, hipStream_t st, int E, const float *z0, const float *task_emb, const float *act_mask,
            const float *disc_pow, float *prev_mean, const uint8_t *t0, int eval_mode, const tdmpc2_noise *tape, uint64_t seed,
            float *action, const tdmpc2_debug *dbg);
int lay_value(tdmpc2_plan *h, hipStream_t st, int rows, const float *z, bool target, bool reduce_min, const float *pi_eps,
              const int *qidx_dev /* [2] */, unsigned long long seed, unsigned call, const float *reward, const float *terminated,
              float discount, const int *row_task /* padded [rows_p] or null */, float *action, float *out, int n_off = 0,
              float *entropy = nullptr, float *scaled_entropy = nullptr);  // (policy loss: a piece of rows, the entropy terms)
// one CEM iteration's sampled actions (rows n >= P of h->actions, every step) and its two Q heads per plan -> qbuf [E, 2]
// (used by both families when a plan is sharded: tdmpc2_plan_shard_values)
int lay_sample_iteration(tdmpc2_plan *h, hipStream_t st, int E, int iter, const float *act_mask, const tdmpc2_noise *tape,
                         uint64_t seed, unsigned call, int *qbuf);
// the two Q heads of a single evaluation (td_target / estimate_value entry points): copied from `qidx` ([E, 2], row stride
// `stride`) or drawn (Philox) when it is null
int lay_set_qidx(tdmpc2_plan *h, hipStream_t st, int E, const int *qidx, long stride, int nq, int iter, uint64_t seed, unsigned call, int *dst);

// ---- model rollout / losses (k_model.hip per action padding: the fused family's kernels; its generic unit: the row kernels;
// k_layered.hip: the layered family's stages).  Routes: model_route.h.
struct ModelOps {
    void (*dyn)(int ar, const ModelParams &p, int gx, size_t lds, hipStream_t st);
    void (*chain)(int ar, const ModelParams &p, int gx, int gy, int gz, size_t lds, hipStream_t st);
    int (*set_lds)(int ar, size_t lds_bytes);
};
const ModelOps &model_ops_ap16(); const ModelOps &model_ops_ap32(); const ModelOps &model_ops_ap48(); const ModelOps &model_ops_ap64();
int model_launch_cons(const ModelConsParams &p, int gx, hipStream_t st);
int model_launch_tail(const ModelTailParams &p, hipStream_t st);
int model_launch_tile_tasks(const int *task_ids, int B, int rows, int rows_p, int *out, hipStream_t st);
// layered family: the stages of a call (r: model_route's answer).  zs [H + 1, B, L] with zs[0] already written; row_task: the
// row -> task map tiled over (H + 1) * B rows and padded, or null.
int lay_model(tdmpc2_plan *h, hipStream_t st, const ModelRoute &r, int B, int H, const float *actions, float *zs, bool target,
              const int *row_task, const ModelOutArgs &out, const ModelLossArgs &ls);

// ---- policy loss (k_policy_loss.hip per action padding: ks_value_ent of the fused family; its generic unit: the one-workgroup kernels)
#include "policy_loss_params.h"
struct PolicyLossOps {
    void (*value_ent)(int ar, const ValueEntParams &p, int grid, size_t lds, hipStream_t st);
    int (*set_lds)(int ar, size_t lds_bytes);
};
const PolicyLossOps &policy_loss_ops_ap16(); const PolicyLossOps &policy_loss_ops_ap32(); const PolicyLossOps &policy_loss_ops_ap48(); const PolicyLossOps &policy_loss_ops_ap64();
int pl_set_lds();  // k_running_scale's dynamic LDS limit (once per handle, at creation)
int pl_launch_scale(const RunningScaleParams &p, hipStream_t st);
int pl_launch_tail(const PolicyLossTailParams &p, hipStream_t st);
int pl_launch_term_stats(const TerminationStatsParams &p, hipStream_t st);

// ---- the weight packer: binds, grouped refresh, soft update (k_refresh.hip: refresh_kernels.cuh, launch list in refresh_route.h)
#include "refresh_params.h"
int refresh_launch(int op /* RO_* */, const RfParams &p, hipStream_t st);

// ---- pixel encoder, batch route (k_pixel_batch.hip)
int pixb_set_lds(size_t bytes);  // layer 0's dynamic LDS limit (at reserve)
int pixb_launch(int layer, bool obs_u8, const PixbParams &p, const PixGrid &g, hipStream_t st);

// ---- policy prior (k_policy.hip)
int pol_set_lds();  // the GEMV instantiations' dynamic LDS limit (once per handle, at bind)
int pol_launch_row(const PolRowParams &p, const PolGrid &g, hipStream_t st);
int pol_launch_gemv(const PolGemvParams &p, const PolGrid &g, hipStream_t st);
int pol_launch_head(const PolHeadParams &p, const PolGrid &g, hipStream_t st);

}  // namespace tdk
