/*
 * tdmpc2_plan.h — C ABI of the MI355X-native TD-MPC2 MPPI/CEM planner.
 *
 * The reference (nicklashansen/tdmpc2) is pure Python and has no FFI layer; its
 * boundary for this path is the method pair
 *     TDMPC2.act(obs, t0, eval_mode, task)        tdmpc2/tdmpc2.py:97-120
 *     TDMPC2.plan -> _plan(obs, t0, eval_mode, task)  tdmpc2/tdmpc2.py:45-55,138-206
 * The entry points below are what a ctypes binding of that path needs (the
 * reference-side stub is shown in INTEGRATION.md).  They replace, one for one:
 *
 *   tdmpc2_plan_create        <- TDMPC2.__init__ planner state         tdmpc2/tdmpc2.py:17-43
 *   tdmpc2_plan_bind_weights  <- WorldModel parameters / load_state_dict tdmpc2/common/world_model.py:20-36,
 *                                                                       tdmpc2/tdmpc2.py:81-95
 *   tdmpc2_plan_run           <- TDMPC2._plan after encode()            tdmpc2/tdmpc2.py:154-206
 *   tdmpc2_plan_estimate_value<- TDMPC2._estimate_value                 tdmpc2/tdmpc2.py:122-136
 *   tdmpc2_plan_refit         <- the elite select + refit block         tdmpc2/tdmpc2.py:184-197
 *   tdmpc2_plan_bind_encoder  <- the state encoder's parameters         tdmpc2/common/layers.py:153-164
 *   tdmpc2_plan_encode        <- WorldModel.encode (state observations) tdmpc2/common/world_model.py:103-112
 *   tdmpc2_plan_run_obs       <- TDMPC2._plan including encode()        tdmpc2/tdmpc2.py:152-206
 *   tdmpc2_plan_bind_pixel_encoder <- the pixel encoder's parameters    tdmpc2/common/layers.py:136-150
 *   tdmpc2_plan_encode_pix    <- WorldModel.encode (rgb observations)   tdmpc2/common/layers.py:36-71,136-150
 *   tdmpc2_plan_encode_pix_batch <- the same on the frame stacks of a training batch (TDMPC2._update, tdmpc2.py:259-267)
 *   tdmpc2_plan_run_pix       <- TDMPC2._plan including encode(), rgb   tdmpc2/tdmpc2.py:152-206
 *   tdmpc2_plan_bind_policy   <- the policy prior's parameters (_pi)    tdmpc2/common/world_model.py:32
 *   tdmpc2_plan_pi            <- WorldModel.pi                          tdmpc2/common/world_model.py:144-184
 *   tdmpc2_plan_act_pi[_pix]  <- TDMPC2.act with cfg.mpc == False       tdmpc2/tdmpc2.py:114-120
 *   tdmpc2_plan_td_target[_mt]    <- TDMPC2._td_target                  tdmpc2/tdmpc2.py:239-254
 *   tdmpc2_plan_policy_value[_mt] <- forward half of TDMPC2.update_pi   tdmpc2/tdmpc2.py:208-225
 *   tdmpc2_plan_policy_loss[_mt]  <- TDMPC2.update_pi's whole forward   tdmpc2/tdmpc2.py:208-239
 *   tdmpc2_plan_running_scale     <- RunningScale.update                tdmpc2/common/scale.py:39-42
 *   tdmpc2_plan_termination_stats <- math.termination_statistics        tdmpc2/common/math.py:97-109
 *   tdmpc2_plan_model_rollout[_mt] <- the open-loop latent rollout and predictions of TDMPC2._update  tdmpc2/tdmpc2.py:268-283
 *   tdmpc2_plan_model_losses[_mt]  <- ... and its four losses                                       tdmpc2/tdmpc2.py:285-304
 *   tdmpc2_plan_export_packed / import_packed <- TDMPC2.save / load of the planner's weights  tdmpc2/tdmpc2.py:72-95
 *   tdmpc2_plan_export_noise  <- the six RNG draw sites of one plan    tdmpc2/tdmpc2.py:176,204, tdmpc2/common/world_model.py:156,212,
 *                                (what torch.manual_seed pins there)   tdmpc2/common/math.py:90
 *   tdmpc2_buffer_create / add / load / sample <- Buffer (torchrl slice sampler)               tdmpc2/common/buffer.py:13-115
 *
 * Conventions
 *   - plain C types only; every tensor is a DEVICE pointer to fp32 (or int32 /
 *     uint8 where stated), densely packed, last index fastest.
 *   - the caller owns every buffer it passes; the library owns only what it
 *     allocates in create/bind and frees in destroy.  `run` allocates nothing.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *     a handle is not re-entrant: a call entered while another thread is inside
 *     the same handle returns TDMPC2_ERR_STATE (use one handle per thread; handles
 *     share nothing).  A handle is one workspace, so its calls must not overlap on
 *     the device either: calls on ONE stream are ordered by the stream; when a handle
 *     moves to another stream its first call there waits (hipStreamWaitEvent) for the
 *     handle's last call on the previous stream -- the library does that itself.
 *     The exception is stream capture: a captured call neither waits nor leaves an
 *     event (the graph replays wherever it is launched); ordering a graph launch
 *     against eager calls of the same handle on other streams is the caller's.
 *     Every call runs on the handle's device (cfg.device) and
 *     restores the caller's current device.  Return value 0 = ok, otherwise an error code
 *     (no C++ exception crosses the ABI); `tdmpc2_last_error()` has the text.
 *   - E = number of independent environments planned in one call (the reference
 *     is E = 1: tdmpc2/tdmpc2.py:111,163).  H horizon, N num_samples,
 *     K num_elites, P num_pi_trajs, I iterations, A action_dim, L latent_dim,
 *     M mlp_dim, T task_dim, B num_bins, nq num_q.
 */
#ifndef TDMPC2_PLAN_H
#define TDMPC2_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDMPC2_PLAN_ABI_VERSION 14

typedef struct tdmpc2_plan tdmpc2_plan_t;

/* Planner constants; field names follow the reference config
 * (tdmpc2/config.yaml:33-64).  `iterations` is the value AFTER the reference's
 * "+2 if action_dim >= 20" adjustment (tdmpc2/tdmpc2.py:34) — the host applies it. */
typedef struct tdmpc2_plan_cfg {
    int32_t horizon, num_samples, num_elites, num_pi_trajs, iterations;
    int32_t action_dim, latent_dim, mlp_dim, task_dim, num_bins, num_q, simnorm_dim;
    /* num_bins: 2 .. 128 two-hot bins, or 0 / 1 = the reference's regression heads (one output column; two_hot_inv is the
     * identity / symexp, common/math.py:76-79).  simnorm_dim: 8 (layers.py:84-88; every released model). */
    float vmin, vmax, min_std, max_std, temperature;
    float log_std_min, log_std_dif;   /* WorldModel buffers, world_model.py:34-35 */
    int32_t multitask, episodic;
    int32_t max_envs;                 /* workspace is sized for this many concurrent plans */
    int32_t device;                   /* HIP device ordinal */
    int32_t path;                     /* enum tdmpc2_path: which kernel family runs the rollout */
    int32_t precision;                /* enum tdmpc2_precision: how the fp32 contractions are carried out */
    int32_t num_valid_samples;        /* ABI 8.  0 = num_samples.  Otherwise (num_elites <= . <= num_samples): the reference's
                                       * cfg.num_samples when that is not a multiple of the kernels' row tile (config.yaml:36 allows
                                       * any value; the kernels want 64 / 128): create the handle with num_samples rounded UP, pass the
                                       * true count here, and pad the noise tapes' sample axis to the rounded count.  The padding rows
                                       * are rolled out like the others but can never be elites: they sort behind every real row
                                       * in the top-k of tdmpc2.py:185 (as the -inf rows of a masked topk would), so mean / std / action
                                       * are those of a plan over the true count.  tdmpc2_amd.NativePlanner does all of this itself. */
} tdmpc2_plan_cfg;

/* Two kernel families implement the same math (results agree to fp32 round-off):
 *   FUSED   one persistent workgroup per 64 sample rows keeps activations in LDS for a whole CEM
 *           iteration; built for latent_dim == mlp_dim == 512 (every 5M model), episodic or not.
 *   LAYERED one MFMA GEMM launch per nn.Linear over all E*N rows, activations in HBM; any
 *           latent_dim / mlp_dim that are multiples of 32 (1M ... 317M models), episodic or not.
 * AUTO picks FUSED when the configuration fits it, else LAYERED. */
enum tdmpc2_path { TDMPC2_PATH_AUTO = 0, TDMPC2_PATH_FUSED = 1, TDMPC2_PATH_LAYERED = 2 };

/* Arithmetic of the nn.Linear contractions (everything else is fp32 in both modes):
 *   FP32       v_mfma_f32_32x32x2_f32: exact fp32 products and accumulation (bitwise an fmaf chain).
 *   SPLIT_F16  every fp32 operand is carried as hi + lo f16 pieces (22 significand bits) and a product is
 *              a_hi b_hi + a_hi b_lo + a_lo b_hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation: fp32-class
 *              error (checked against fp64 in the tests) at up to 16/3 of the fp32 matrix rate.
 * AUTO = SPLIT_F16. */
enum tdmpc2_precision { TDMPC2_PREC_AUTO = 0, TDMPC2_PREC_FP32 = 1, TDMPC2_PREC_SPLIT_F16 = 2 };

enum tdmpc2_net {
    TDMPC2_NET_DYNAMICS = 0,    /* WorldModel._dynamics     world_model.py:26 */
    TDMPC2_NET_REWARD = 1,      /* WorldModel._reward       world_model.py:27 */
    TDMPC2_NET_PI = 2,          /* WorldModel._pi           world_model.py:29 */
    TDMPC2_NET_Q = 3,           /* WorldModel._Qs (stacked) world_model.py:30 */
    TDMPC2_NET_TERMINATION = 4, /* WorldModel._termination  world_model.py:28 */
    TDMPC2_NET_TARGET_Q = 5     /* WorldModel._target_Qs (stacked, optional)  world_model.py:38-53 */
};

enum tdmpc2_status {
    TDMPC2_OK = 0,
    TDMPC2_ERR_INVALID = 1,      /* bad argument */
    TDMPC2_ERR_UNSUPPORTED = 2,  /* configuration outside what the kernels are built for */
    TDMPC2_ERR_HIP = 3,          /* a HIP runtime call failed */
    TDMPC2_ERR_STATE = 4         /* e.g. run before all weights are bound */
};

/* The reference's six RNG draw sites as input tensors.
 * Passing a tape makes a plan a pure function of its inputs (parity runs);
 * passing NULL selects the in-kernel Philox4x32-10 generator (fast mode). */
typedef struct tdmpc2_noise {
    const float *pi_traj_eps;  /* [E,H,P,A]      randn_like, world_model.py:156 via tdmpc2.py:158,160 */
    const float *sample_eps;   /* [E,I,H,N-P,A]  randn,      tdmpc2.py:176 */
    const float *pi_eps;       /* [E,I,N,A]      randn_like, world_model.py:156 via tdmpc2.py:135 */
    const int32_t *qidx;       /* [E,I,2]        randperm(nq)[:2], world_model.py:212 */
    const float *gumbel_exp;   /* [E,K]          exponential_(), math.py:90 */
    const float *final_eps;    /* [E,A]          randn, tdmpc2.py:204 (unused when eval_mode) */
} tdmpc2_noise;

/* The same six tensors as OUTPUTS (tdmpc2_plan_export_noise): device pointers the library writes; any may be NULL. */
typedef struct tdmpc2_noise_out {
    float *pi_traj_eps;  /* [n,H,P,A] */
    float *sample_eps;   /* [n,I,H,N-P,A] */
    float *pi_eps;       /* [n,I,N,A] */
    int32_t *qidx;       /* [n,I,2] */
    float *gumbel_exp;   /* [n,K] */
    float *final_eps;    /* [n,A] */
} tdmpc2_noise_out;

/* Optional stage-wise outputs (any pointer may be NULL). */
typedef struct tdmpc2_debug {
    float *value;       /* [E,I,N]   value after nan_to_num, tdmpc2.py:184 */
    int32_t *elite_idx; /* [E,I,K]   topk indices (value desc, index asc on ties), tdmpc2.py:185 */
    float *score;       /* [E,I,K]   normalised elite scores, tdmpc2.py:190-191 */
    float *mean;        /* [E,I,H,A] tdmpc2.py:192,196 */
    float *std;         /* [E,I,H,A] tdmpc2.py:193-194,197 */
    float *actions;     /* [E,I,H,N,A] sampled actions of every iteration, tdmpc2.py:176-181 */
} tdmpc2_debug;

int tdmpc2_plan_abi_version(void);
const char *tdmpc2_last_error(void);

/* Allocate a planner for `cfg` on cfg->device.  TDMPC2_ERR_UNSUPPORTED if the
 * configuration is outside the compiled kernels' envelope. */
int tdmpc2_plan_create(const tdmpc2_plan_cfg *cfg, tdmpc2_plan_t **out);
void tdmpc2_plan_destroy(tdmpc2_plan_t *h);

/* Bytes of device memory held by the handle (packed weights + workspace). */
uint64_t tdmpc2_plan_device_bytes(const tdmpc2_plan_t *h);

/* The kernel family / arithmetic the handle resolved to (never the AUTO values). */
int tdmpc2_plan_path(const tdmpc2_plan_t *h);
int tdmpc2_plan_precision(const tdmpc2_plan_t *h);

/* Hand one layer of one network to the planner.  Pointers are device fp32 in
 * the checkpoint's own layout (nn.Linear: W[out,in] row-major, b[out];
 * LayerNorm ln_g/ln_b[out], NULL for the plain output layers).  For
 * TDMPC2_NET_Q every tensor carries the leading ensemble dim num_q
 * ("_Qs.params.<layer>.<name>", tdmpc2/common/layers.py:167-199).  The first
 * layer's input columns are ordered [z | task_emb | action]
 * (world_model.py:118-120).  The library re-packs into its own MFMA fragment
 * layout; the source buffers may be freed after the stream reaches this call.
 * One job (this layer, every ensemble member) for the packer that
 * tdmpc2_plan_refresh_weights runs over a whole table: the same kernels, at
 * most 4 launches (csrc/refresh_route.h). */
int tdmpc2_plan_bind_weights(tdmpc2_plan_t *h, int net, int layer, const float *W, const float *b,
                             const float *ln_g, const float *ln_b, int out_features, int in_features,
                             void *stream);

/* One plan per environment: everything of TDMPC2._plan after encode().
 *   z0         [E,L]     latent from WorldModel.encode (tdmpc2.py:153)
 *   task_emb   [E,T]     looked-up (max_norm-renormalised) task embedding rows, NULL if !multitask
 *   act_mask   [E,A]     WorldModel._action_masks[task], NULL if !multitask
 *   disc_pow   [E,H+1]   discount^0..discount^H exactly as tdmpc2.py:126,130-132 accumulates them
 *   prev_mean  [E,H,A]   in: TDMPC2._prev_mean, out: new mean (tdmpc2.py:166-167,205)
 *   t0         [E] u8    first step of an episode (no warm start)
 *   eval_mode            0: add std*noise to the chosen action (tdmpc2.py:203-204)
 *   tape                 NULL -> Philox(seed); `seed` is ignored when a tape is given
 *   action     [E,A]     out: the clamped action (tdmpc2.py:206) */
int tdmpc2_plan_run(tdmpc2_plan_t *h, int n_envs, const float *z0, const float *task_emb,
                    const float *act_mask, const float *disc_pow, float *prev_mean, const uint8_t *t0,
                    int eval_mode, const tdmpc2_noise *tape, uint64_t seed, float *action,
                    const tdmpc2_debug *dbg, void *stream);

/* The in-kernel generator, made visible (parity of the fast mode).  A plan run with tape = NULL draws its noise from
 * Philox4x32-10 keyed by (seed, the handle's call counter at entry, draw site, CEM iteration, environment, element) --
 * the six sites of the reference (tdmpc2/tdmpc2.py:176,204; tdmpc2/common/world_model.py:156,212; tdmpc2/common/math.py:90).
 * export_noise writes exactly those draws, for environments [env_first, env_first + n_envs) of such a call, as the tensors
 * of a noise tape: tdmpc2_plan_run(..., tape = the export, ...) then reproduces the tape = NULL plan bit for bit, and the
 * same tape replays through a CPU restatement of the reference.  Every kernel family draws the same numbers.
 *   call  = the value tdmpc2_plan_call_counter returned BEFORE the run being reproduced (run / run_obs / shard_begin /
 *           policy_value / td_target / model_rollout / model_losses each consume one count). */
int tdmpc2_plan_export_noise(tdmpc2_plan_t *h, int env_first, int n_envs, uint64_t seed, uint32_t call,
                             const tdmpc2_noise_out *out, void *stream);
/* The per-handle call counter mixed into the Philox key (so that consecutive plans under one seed draw fresh noise).
 * Ranks that shard ONE plan (tdmpc2_plan_shard_*) must agree on it: set it from one rank's value before shard_begin. */
int tdmpc2_plan_call_counter(const tdmpc2_plan_t *h, uint32_t *next_call);
int tdmpc2_plan_set_call_counter(tdmpc2_plan_t *h, uint32_t next_call);

/* State-observation encoder: WorldModel.encode for cfg.obs == 'state'
 * (tdmpc2/common/world_model.py:103-112) with the network of layers.enc (tdmpc2/common/layers.py:153-164):
 * n_layers NormedLinear blocks, Mish after all but the last, SimNorm after the last.  Pixel observations have an encoder
 * of their own (tdmpc2_plan_bind_pixel_encoder / encode_pix / run_pix below).  bind_encoder takes one nn.Linear (`W` [out, in] row-major, `b` [out]) and its LayerNorm (`ln_g`,
 * `ln_b` [out]) per call, DEVICE pointers, copied (weights transposed) into library memory; layer 0 takes
 * obs_dim + task_dim inputs, the last layer has latent_dim outputs; widths up to 4096. */
int tdmpc2_plan_bind_encoder(tdmpc2_plan_t *h, int layer, int n_layers, const float *W, const float *b,
                             const float *ln_g, const float *ln_b, int out_features, int in_features,
                             void *stream);
/*   obs [E, obs_dim], task_emb [E, T] (NULL if !multitask; the rows the reference concatenates in
 *   WorldModel.task_emb, world_model.py:88-101) -> z_out [E, L].  n_envs is not limited by max_envs unless a layer
 *   is wider than 1024 (those encoders run layer by layer through a workspace sized for max_envs rows). */
int tdmpc2_plan_encode(tdmpc2_plan_t *h, int n_envs, const float *obs, int obs_dim, const float *task_emb,
                       float *z_out, void *stream);
/* TDMPC2._plan from the observation on (tdmpc2/tdmpc2.py:152-206): encode into library memory, then exactly
 * tdmpc2_plan_run.  One call per environment step, no framework kernel in between. */
int tdmpc2_plan_run_obs(tdmpc2_plan_t *h, int n_envs, const float *obs, int obs_dim, const float *task_emb,
                        const float *act_mask, const float *disc_pow, float *prev_mean, const uint8_t *t0,
                        int eval_mode, const tdmpc2_noise *tape, uint64_t seed, float *action, void *stream);

/* Pixel-observation encoder (ABI 10): WorldModel.encode for cfg.obs == 'rgb' with the network of layers.conv
 * (tdmpc2/common/layers.py:36-71, 136-150): ShiftAug (replicate pad 3 + bilinear resampling by an integer shift), x / 255 - 0.5,
 * Conv2d 7x7/2, 5x5/2, 3x3/2, 3x3/1 with bias and ReLU between, Flatten, SimNorm; fp32 throughout.  Frames are 64 x 64;
 * C = out_channels = cfg.num_channels, a multiple of 8 in [8, 64] with 16 C == latent_dim; Cin = in_channels in [1, 16] (9 for
 * three stacked RGB frames).  Single-task handles only (a multitask handle: TDMPC2_ERR_UNSUPPORTED -- the reference cannot
 * concatenate task_emb onto an image either, world_model.py:88-112).  Not part of the packed blob: re-bind after import_packed.
 * bind_pixel_encoder takes one Conv2d per call, checkpoint keys _encoder.rgb.{2,4,6,8}.{weight,bias} for layers 0..3:
 * W [C, Cin (layer 0) | C, k, k], b [C], kernel = 7, 5, 3, 3; DEVICE pointers, copied (re-packed).  The first call allocates
 * every buffer the encoder uses (a workspace for max_envs images): encode_pix / run_pix allocate nothing. */
int tdmpc2_plan_bind_pixel_encoder(tdmpc2_plan_t *h, int layer, const float *W, const float *b, int out_channels,
                                   int in_channels, int kernel, void *stream);
/*   obs [E, Cin, 64, 64] as uint8 (obs_dtype 0: what the reference's Pixels wrapper returns) or float32 (obs_dtype 1), raw
 *   pixel levels; shift int32 [E, 2] = (dx, dy) of ShiftAug (dx moves the columns), DEVICE memory: the reference draws it with
 *   torch.randint(0, 7, (E, 1, 1, 2)) in train and eval mode alike, so a caller that draws it the same way keeps its RNG stream
 *   identical to the reference's.  Values outside [0, 6] are clamped.  -> z_out [E, 16 C].  1 <= n_envs <= max_envs.  No host
 *   synchronisation: the call can be captured in a hipGraph. */
int tdmpc2_plan_encode_pix(tdmpc2_plan_t *h, int n_envs, const void *obs, int obs_dtype, int in_channels,
                           const int32_t *shift, float *z_out, void *stream);
/* TDMPC2._plan from the frame stack on: encode_pix into library memory, then exactly tdmpc2_plan_run (no task_emb / act_mask). */
int tdmpc2_plan_run_pix(tdmpc2_plan_t *h, int n_envs, const void *obs, int obs_dtype, int in_channels, const int32_t *shift,
                        const float *disc_pow, float *prev_mean, const uint8_t *t0, int eval_mode, const tdmpc2_noise *tape,
                        uint64_t seed, float *action, void *stream);

/* Pixel encoder, batch route (additions to ABI 14; the version number stays 14): the same network on TRAINING batches -- the
 * (H + 1) B frame stacks of TDMPC2._update -- as exact-fp32 MFMA implicit GEMMs (one fmaf chain per output element, like the
 * planning routes).  Reads the weights tdmpc2_plan_bind_pixel_encoder bound (binding again after a reservation keeps working).
 * Single-task handles only.
 * pix_batch_reserve: workspace of the batch route for `chunk_images` images per pass; may be called again with a larger value
 * (grows, never shrinks); needs a bound pixel encoder; allocates -- encode_pix_batch never does.  Not part of create:
 * device_bytes of a handle that never reserves is unchanged. */
int tdmpc2_plan_pix_batch_reserve(tdmpc2_plan_t *h, int chunk_images, void *stream);
/* obs [n, Cin, 64, 64] uint8 / float32, shift int32 [n, 2] (as encode_pix) -> z_out [n, 16 C]; any n >= 1 (not bounded by
 * max_envs): passes of the reserved chunk, four launches each, ordered by the stream.  No host synchronisation.
 * TDMPC2_ERR_STATE without a bound encoder or a reservation. */
int tdmpc2_plan_encode_pix_batch(tdmpc2_plan_t *h, int n_images, const void *obs, int obs_dtype, int in_channels,
                                 const int32_t *shift, float *z_out, void *stream);

/* Policy prior (ABI 11): WorldModel.pi (tdmpc2/common/world_model.py:144-184, common/math.py:12-29) and TDMPC2.act's branch
 * without planning (tdmpc2/tdmpc2.py:114-120), plain fp32.  bind_policy takes _pi.{layer}: layer 0 [M, L + T] and 1 [M, M]
 * with their LayerNorm (ln_g / ln_b), layer 2 [2A, M] without (ln_g / ln_b ignored); DEVICE pointers, copied transposed into an
 * fp32 [in][out] copy of its own -- separate from tdmpc2_plan_bind_weights(TDMPC2_NET_PI), whose MFMA layouts a GEMV cannot read,
 * so that only handles which use the policy prior pay for it (2 MB on the 5M model, 90 MB on the 317M model).  The first call
 * allocates every buffer the policy prior uses; pi / act_pi / act_pi_pix allocate nothing and never synchronise the host (they
 * can be captured in a hipGraph).  Not part of the packed blob: re-bind after import_packed.
 *   z [n, L]; task_emb [n, T] and act_mask [n, A] (multitask handles: both required; per row, action_dims = act_mask.sum(-1) per
 *   row); eps [n, A] the normal draws of torch.randn_like, or NULL: drawn in the kernel from Philox(seed, call counter, row,
 *   action index) -- every call advances the call counter by exactly one.  eval_mode: out->action = info["mean"].
 * Routes (TDMPC2_TUNE_POLICY_ROUTE, tdmpc2_amd/csrc/policy_route.h): the row route runs one workgroup per row and the whole chain
 * in one launch -- acting with an encoder no wider than 1024, the encoder too; the spread route one launch per layer (GEMVs that
 * read each weight once per 8 rows, a LayerNorm + Mish row kernel, the head), chunks of at most max_envs rows.  Refusals: nothing
 * bound -- TDMPC2_ERR_STATE; a layer shape other than (L + T) -> M -> 2A, n_envs outside [1, max_envs] when acting, a null
 * `out` or `out->action` -- TDMPC2_ERR_INVALID; act_pi_pix on a multitask handle -- TDMPC2_ERR_UNSUPPORTED. */
typedef struct tdmpc2_policy_out {   /* device pointers; all but action may be NULL */
    float *action;          /* [n, A]  tanh(mean + eps*exp(log_std)); eval_mode: info["mean"] */
    float *mean;            /* [n, A]  info["mean"] (after tanh, masked) */
    float *log_std;         /* [n, A]  info["log_std"] (masked) */
    float *entropy;         /* [n]     info["entropy"] */
    float *scaled_entropy;  /* [n]     info["scaled_entropy"] */
    float *eps_out;         /* [n, A]  the normal draws used (before masking): passed back as eps they replay the call */
} tdmpc2_policy_out;
int tdmpc2_plan_bind_policy(tdmpc2_plan_t *h, int layer, const float *W, const float *b, const float *ln_g, const float *ln_b,
                            int out_features, int in_features, void *stream);
int tdmpc2_plan_pi(tdmpc2_plan_t *h, int n_rows, const float *z, const float *task_emb, const float *act_mask, const float *eps,
                   uint64_t seed, const tdmpc2_policy_out *out, void *stream);
/* act(): encode (tdmpc2_plan_bind_encoder) then pi, 1 <= n_envs <= max_envs; obs [n_envs, obs_dim]. */
int tdmpc2_plan_act_pi(tdmpc2_plan_t *h, int n_envs, const float *obs, int obs_dim, const float *task_emb, const float *act_mask,
                       const float *eps, int eval_mode, uint64_t seed, const tdmpc2_policy_out *out, void *stream);
/* the same for rgb observations: encode_pix (its obs / obs_dtype / in_channels / shift) then pi; single-task handles only. */
int tdmpc2_plan_act_pi_pix(tdmpc2_plan_t *h, int n_envs, const void *obs, int obs_dtype, int in_channels, const int32_t *shift,
                           const float *eps, int eval_mode, uint64_t seed, const tdmpc2_policy_out *out, void *stream);

/* Training-side consumers of the planner's layer code, forward only, no gradients.  Both kernel
 * families, single-task and multitask models.  The fused family takes any number of rows; the layered family at most
 * max_envs * num_samples rows per call (its activation workspace).  Multitask tables are (re)built inside the call and
 * their storage grows on demand (the first such call allocates: keep it outside a hipGraph capture).
 *
 * policy_value: a = pi(z) (world_model.py:144-184, sampled with pi_eps [n_rows, A] or Philox(seed) when NULL), then the
 * two heads qidx[0..1] (device int32[2]; NULL: drawn like randperm(num_q)[:2], world_model.py:212) of the online ensemble
 * (use_target = 0: what update_pi evaluates, tdmpc2.py:220-221) or of the target ensemble (use_target = 1: bind net
 * TDMPC2_NET_TARGET_Q first), reduced 'avg' (reduce_min = 0) or 'min' (1), world_model.py:213-216.
 *   z [n_rows, L] -> action [n_rows, A] (may be NULL), q [n_rows]. */
int tdmpc2_plan_policy_value(tdmpc2_plan_t *h, int n_rows, const float *z, int use_target, int reduce_min,
                             const float *pi_eps, const int32_t *qidx, uint64_t seed, float *action, float *q,
                             void *stream);
/* TDMPC2._td_target (tdmpc2.py:239-254): td = reward + discount (1 - terminated) min_{2 target heads} Q(next_z, pi(next_z)).
 *   next_z [n_rows, L] (the reference's [H, B, L] flattened), reward, terminated [n_rows] -> td [n_rows]. */
int tdmpc2_plan_td_target(tdmpc2_plan_t *h, int n_rows, const float *next_z, const float *reward,
                          const float *terminated, float discount, const float *pi_eps, const int32_t *qidx,
                          uint64_t seed, float *td, void *stream);

/* The same on multitask models, where a training batch carries ONE TASK PER ROW (WorldModel.task_emb with a task
 * vector, world_model.py:88-101; the reference repeats task [B] over the H leading rows of next_z [H, B, L]):
 * the row -> task map plus the per-task tables the reference indexes with it.  All DEVICE pointers. */
typedef struct tdmpc2_task_tables {
    const int32_t *task_ids;  /* [n_rows]            task of each row */
    const float *task_emb;    /* [n_tasks, T]        WorldModel._task_emb rows, max_norm renorm applied (world_model.py:21) */
    const float *act_mask;    /* [n_tasks, A]        WorldModel._action_masks (world_model.py:22-24) */
    const float *discount;    /* [n_tasks] or NULL   TDMPC2.discount (tdmpc2.py:35-37); td_target only */
    int32_t n_tasks;
} tdmpc2_task_tables;
/* `tasks` must be NULL for single-task handles and non-NULL for multitask ones. */
int tdmpc2_plan_policy_value_mt(tdmpc2_plan_t *h, int n_rows, const float *z, const tdmpc2_task_tables *tasks,
                                int use_target, int reduce_min, const float *pi_eps, const int32_t *qidx, uint64_t seed,
                                float *action, float *q, void *stream);
/* `discount` is used by single-task handles; multitask handles take tasks->discount[task of the row]. */
int tdmpc2_plan_td_target_mt(tdmpc2_plan_t *h, int n_rows, const float *next_z, const float *reward,
                             const float *terminated, float discount, const tdmpc2_task_tables *tasks,
                             const float *pi_eps, const int32_t *qidx, uint64_t seed, float *td, void *stream);

/* Model rollout and losses (ABI 12): the rest of the forward half of TDMPC2._update (tdmpc2/tdmpc2.py:259-304) -- what
 * tdmpc2_plan_encode and tdmpc2_plan_td_target do not cover.  Forward only, EVAL MODE, fp32 in / fp32 out, no gradients.  Eval
 * mode means dropout off: the Q heads' first layer has Dropout(cfg.dropout) in the reference (common/layers.py, mlp(..., dropout=)),
 * which is active inside _update (model.train(), tdmpc2.py:266); the numbers here equal what _update reports when cfg.dropout == 0
 * and are the dropout-free values otherwise.  Both kernel families, both arithmetics (the contractions run in the handle's
 * arithmetic; log-softmax, two-hot targets, MSE, BCE and every reduction are plain fp32); single-task and multitask handles.
 *
 * model_rollout: z0 [B, L], actions [steps, B, A] (used as given: the reference does not mask recorded actions in _update),
 * 0 <= steps <= 8, use_target: the online (0) or target (1: bind TDMPC2_NET_TARGET_Q first) Q ensemble.  Outputs are optional
 * device pointers (NULL = not wanted; a chain whose outputs are all NULL is not computed):
 *   zs            [steps + 1, B, L]   zs[0] = z0, zs[t+1] = next(zs[t], actions[t])        tdmpc2.py:269-276, world_model.py:114-121
 *   reward_logits [steps, B, nb]      WorldModel.reward(zs[:-1], actions), nb = max(num_bins, 1)   world_model.py:123-130
 *   reward        [steps, B]          two_hot_inv of them                                  math.py:74-83
 *   q_logits      [num_q, steps, B, nb]  EVERY head: WorldModel.Q(zs[:-1], actions, return_type='all')  world_model.py:186-210
 *   q             [num_q, steps, B]   two_hot_inv of them
 *   term_logit    [steps + 1, B]      WorldModel.termination(zs, unnormalized=True); episodic handles only  world_model.py:132-141
 * steps = 1 is WorldModel.next / reward / Q on a batch of rows; steps = 0 is WorldModel.termination(z0).
 * _mt: tasks->task_ids is [B], ONE TASK PER ROW of the batch (the reference repeats task [B] over the leading step axis); rows use
 * the first-layer bias of their task (tasks->discount is not read).
 *
 * model_losses: the same inputs and optional outputs (`out` may be NULL) plus the targets of _update ->
 *   losses [5] = consistency, reward, value, termination, total (tdmpc2.py:285-304): mse(zs[t+1], next_z[t]) rho^t summed, / steps;
 *   soft_ce (math.py:5-9: log_softmax of the logits against two_hot of the target, math.py:58-71) averaged over the batch per
 *   step, rho^t, / steps and for the value loss also / num_q; binary_cross_entropy_with_logits(term_logit[1:], terminated) over all
 *   steps x B rows (0 when not episodic); total = the coefficient-weighted sum.
 *   Non-finite targets: a NaN in reward / td_target / next_z / terminated makes exactly the losses that consume it NaN (that loss,
 *   its step_means entry and total; the others keep their bits), as every torch op of the reference propagates it; +-Inf in
 *   reward / td_target stays finite, the vmin / vmax-clamped bin as in two_hot.
 *   step_means [4, steps] (may be NULL): the unweighted per-step batch means of consistency, reward, value (mean over the heads
 *   too) and termination -- loss against rollout depth.
 * When only losses are asked for, no logits go through HBM.  Deterministic: per-row terms go to a workspace and ONE workgroup adds
 * them in a fixed order (no float atomics) -- the same inputs give the same bits, whatever else is asked for.
 * Launches (tdmpc2_amd/csrc/model_route.h): FUSED one workgroup per 64-row tile rolls the dynamics chain, then ONE launch of
 * tiles x steps x (1 + num_q) workgroups runs the reward and Q chains of every step side by side, one more for the termination
 * head; LAYERED the dynamics chain per step over B rows, then every other chain once over all steps x B rows.  No workgroup
 * waits for another one in the new kernels; the LAYERED GEMMs keep their NormedLinear epilogue (TDMPC2_TUNE_FUSE_LN), whose fault
 * contract applies unchanged: NaN in every output and tdmpc2_plan_take_fault.
 * Workspace (zs when not asked for, per-row loss terms, the multitask tables) grows at the first call of a shape: keep that call
 * outside a hipGraph capture; after it the calls allocate nothing and never synchronise the host.
 * Refusals: steps outside [0, 8], batch < 1, model_losses with steps < 1, a missing target, `terminated` on a non-episodic handle or
 * term_logit asked of one, tasks on a single-task handle (or none on a multitask one), LAYERED: batch x steps beyond max_envs x
 * num_samples rows -- TDMPC2_ERR_INVALID; use_target without the target ensemble -- TDMPC2_ERR_STATE; model_losses with
 * num_bins < 2 (the reference's soft_ce is identically 0 there) -- TDMPC2_ERR_UNSUPPORTED. */
typedef struct tdmpc2_model_out {   /* device pointers, any may be NULL */
    float *zs, *reward_logits, *reward, *q_logits, *q, *term_logit;
} tdmpc2_model_out;
typedef struct tdmpc2_model_targets {
    const float *next_z;      /* [steps, B, L]  encode(obs[1:])                                    tdmpc2.py:262 */
    const float *reward;      /* [steps, B] */
    const float *td_target;   /* [steps, B]     tdmpc2_plan_td_target's output                     tdmpc2.py:263 */
    const float *terminated;  /* [steps, B] in {0, 1}; NULL unless episodic */
    float rho, consistency_coef, reward_coef, value_coef, termination_coef;   /* config.yaml:17-21 */
} tdmpc2_model_targets;
int tdmpc2_plan_model_rollout(tdmpc2_plan_t *h, int batch, int steps, const float *z0, const float *actions, int use_target,
                              const tdmpc2_model_out *out, void *stream);
int tdmpc2_plan_model_rollout_mt(tdmpc2_plan_t *h, int batch, int steps, const float *z0, const float *actions,
                                 const tdmpc2_task_tables *tasks, int use_target, const tdmpc2_model_out *out, void *stream);
int tdmpc2_plan_model_losses(tdmpc2_plan_t *h, int batch, int steps, const float *z0, const float *actions, int use_target,
                             const tdmpc2_model_targets *targets, const tdmpc2_model_out *out, float *losses, float *step_means,
                             void *stream);
int tdmpc2_plan_model_losses_mt(tdmpc2_plan_t *h, int batch, int steps, const float *z0, const float *actions,
                                const tdmpc2_task_tables *tasks, int use_target, const tdmpc2_model_targets *targets,
                                const tdmpc2_model_out *out, float *losses, float *step_means, void *stream);

/* Policy loss (ABI 13): the forward of TDMPC2.update_pi (tdmpc2/tdmpc2.py:208-239), with the running Q scale.  Forward only, EVAL
 * MODE (the caveat of model_losses applies: the reference's dropout on the Q heads' first layer is active inside update_pi), fp32
 * in / fp32 out, no gradients.
 *   action, info = pi(zs, task)         pi_eps [steps + 1, B, A], or Philox(seed) when NULL; the call advances the handle's
 *                                       counter by one, as policy_value does
 *   qs = Q(zs, action, 'avg')           two heads of the ONLINE ensemble (the reference's _detach_Qs carries the same weights):
 *                                       qidx (device int32[2]) or drawn once per call like randperm(num_q)[:2]
 *   scale.update(qs[0]); qs /= scale    update_scale = 1: *scale is lerped towards max(p95 - p5, 1) of q[0] BEFORE the division, as
 *                                       update_pi does; 0: *scale is read only
 *   pi_loss = mean_t(-mean_B(entropy_coef * scaled_entropy + qs) * rho^t) over the steps + 1 rows of zs.
 * zs [steps + 1, B, L], 0 <= steps <= 8.  scale: DEVICE float[1] (RunningScale.value).  loss: DEVICE float[4] = pi_loss, mean
 * entropy, mean scaled_entropy, the scale after the call.  _mt: tasks->task_ids is [B] as in model_rollout_mt; the action mask and
 * action_dims of a row are its task's.
 * Rows (both kernel families, both arithmetics): the value chain of policy_value with the entropy terms of WorldModel.pi per row
 * (log_prob = sum_a(-0.5 eps^2 - log_std - log(2 pi)/2), the squash correction sum_a log(relu(1 - a^2) + 1e-6), entropy =
 * -log_prob, scaled_entropy = -log_prob * scaled / (log_prob + 1e-8)): FUSED ks_value_ent, one launch; LAYERED the GEMM chain of
 * lay_value with the row kernel l_pi_head_ent, in pieces of max_envs x num_samples rows when the call has more (the two heads are
 * drawn once per call and a row's Philox / tape index is its row in the call: piece boundaries change no bit).  q, entropy and
 * scaled_entropy go to a workspace; k_running_scale, then k_policy_loss_tail -- ONE workgroup each, fixed order, no float atomics:
 * the same inputs give the same bits whatever optional outputs are asked for.  No new inter-workgroup wait; the LAYERED GEMMs keep
 * their fault contract: NaN in every output, *scale left as it was, tdmpc2_plan_take_fault.  The workspace grows at the first call
 * of a shape (keep that call outside a hipGraph capture); after it the call allocates nothing, never synchronises the host and
 * can be captured.
 * Refusals: NULL zs / in / scale / loss, batch < 1, steps outside [0, 8], tasks on a single-task handle (or none on a multitask
 * one) -- TDMPC2_ERR_INVALID; update_scale with batch > 16384 (the percentile kernel's limit) -- TDMPC2_ERR_UNSUPPORTED. */
typedef struct tdmpc2_policy_loss_in {
    float rho, entropy_coef, tau;   /* config.yaml rho, entropy_coef, tau */
    int update_scale;               /* 1: RunningScale.update(qs[0]) BEFORE the division, as update_pi does; 0: divide by *scale as it is */
} tdmpc2_policy_loss_in;
typedef struct tdmpc2_policy_loss_out {  /* device pointers, any may be NULL */
    float *action;          /* [steps+1, B, A] */
    float *q;               /* [steps+1, B]  avg of the two heads, UNSCALED */
    float *entropy;         /* [steps+1, B]  info["entropy"] */
    float *scaled_entropy;  /* [steps+1, B]  info["scaled_entropy"] */
    float *step_means;      /* [3, steps+1]  per-step batch means of q/scale, scaled_entropy, entropy */
    float *percentiles;     /* [2]           the 5th / 95th percentile of q[0] (written only when update_scale) */
} tdmpc2_policy_loss_out;
int tdmpc2_plan_policy_loss(tdmpc2_plan_t *h, int batch, int steps, const float *zs, const float *pi_eps, const int32_t *qidx,
                            uint64_t seed, const tdmpc2_policy_loss_in *in, float *scale, const tdmpc2_policy_loss_out *out,
                            float *loss, void *stream);
int tdmpc2_plan_policy_loss_mt(tdmpc2_plan_t *h, int batch, int steps, const float *zs, const tdmpc2_task_tables *tasks,
                               const float *pi_eps, const int32_t *qidx, uint64_t seed, const tdmpc2_policy_loss_in *in,
                               float *scale, const tdmpc2_policy_loss_out *out, float *loss, void *stream);
/* RunningScale.update alone (common/scale.py:21-42): x [n] (device) -> *scale += tau (max(p95 - p5, 1) - *scale); percentiles [2]
 * optional.  torch.sort's order (NaN last, after +Inf); positions pct (n - 1) / 100, floor, min(floor + 1, n - 1) and the weights
 * in fp32, products and sum unfused, as the reference forms them.  Non-finite inputs give what the formula gives (a NaN that the
 * order statistics do not touch leaves the scale finite).  Any handle (no weights needed).  n < 1 or NULL x / scale --
 * TDMPC2_ERR_INVALID; n > 16384 -- TDMPC2_ERR_UNSUPPORTED. */
int tdmpc2_plan_running_scale(tdmpc2_plan_t *h, int n, const float *x, float tau, float *scale, float *percentiles, void *stream);
/* math.termination_statistics(sigmoid(term_logit), terminated) (common/math.py:97-109): n rows (device) -> stats [2] = rate, f1.
 * pred = sigmoid(logit) > 0.5 with the library's fp32 sigmoid; integer tp / fn / fp counts; eps = 1e-9.  n < 1 or a NULL
 * pointer -- TDMPC2_ERR_INVALID. */
int tdmpc2_plan_termination_stats(tdmpc2_plan_t *h, int n, const float *term_logit, const float *terminated, float *stats,
                                  void *stream);

/* Weight refresh (ABI 14): the whole model re-packed from the trainer's own parameter tensors in a constant, small number of
 * launches -- what a training loop needs after every optimiser step (TDMPC2._update, tdmpc2/tdmpc2.py:259-316, changes every
 * parameter; the per-layer binds above run the same packer but cost up to four launches per layer and call).
 *
 * tdmpc2_weight_table: device pointers, fp32, in the checkpoint's layout -- per net and layer exactly the W, b, ln_g, ln_b that
 * tdmpc2_plan_bind_weights takes (the Q nets stacked over num_q; ln_g / ln_b NULL where the layer has no LayerNorm), and the
 * state encoder's layers as tdmpc2_plan_bind_encoder takes them (enc_layers of them, shapes in enc_out / enc_in;
 * enc_layers = 0: the encoder is left as it is).  A net whose twelve entries are all NULL is left as it is; a net that is
 * named must bring all three layers.  Shapes of the nets come from the handle's cfg.  The table is read on the host at call
 * time and travels to the kernels as a kernel argument: no host-to-device copy is enqueued, and a call captured into a
 * hipGraph reads, at every replay, THE TENSORS WHOSE POINTERS THE TABLE HELD AT CAPTURE (update them in place). */
typedef struct tdmpc2_weight_entry {
    const float *W, *b, *ln_g, *ln_b;
} tdmpc2_weight_entry;
typedef struct tdmpc2_weight_table {
    tdmpc2_weight_entry net[6][3];   /* [enum tdmpc2_net][layer] */
    tdmpc2_weight_entry enc[6];      /* state encoder, layers 0 .. enc_layers - 1 */
    int32_t enc_layers;
    int32_t enc_out[6], enc_in[6];   /* nn.Linear out_features / in_features of the encoder's layers */
} tdmpc2_weight_table;
/* Produces, for every net the table names, exactly what the sequence of tdmpc2_plan_bind_weights / tdmpc2_plan_bind_encoder
 * calls produces (the same kernels over a larger job table; tdmpc2_plan_export_packed is byte-identical): operand slabs, per-layer scale records, padded biases,
 * LayerNorm vectors, task-embedding columns, the transposed encoder; if the policy prior's fp32 copy is bound
 * (tdmpc2_plan_bind_policy) and TDMPC2_NET_PI is named, that copy as well.  Both kernel families, both arithmetics.  At most 4
 * launches on a SPLIT_F16 handle (reset of the maxima, scan, scales, pack of everything), 1 on an FP32 handle, whatever num_q
 * and however many nets (csrc/refresh_route.h).  Storage of a (net, layer) is allocated at its first refresh or bind; after
 * that the call neither allocates nor synchronises and may be captured.  A handle whose nets were never bound becomes ready
 * through this call alone.  The pixel encoder is not part of the table (tdmpc2_plan_bind_pixel_encoder).
 * TDMPC2_ERR_INVALID: NULL handle / table, a named net with a missing W / b (or LayerNorm vector where the layer has one),
 * termination entries on a non-episodic handle, encoder shapes that tdmpc2_plan_bind_encoder refuses; the encoder's
 * TDMPC2_ERR_UNSUPPORTED / TDMPC2_ERR_STATE cases are its own.  The handle stays usable after a refusal. */
int tdmpc2_plan_refresh_weights(tdmpc2_plan_t *h, const tdmpc2_weight_table *tab, void *stream);
/* WorldModel.soft_update_target_Q (common/world_model.py:82-86; the last line of TDMPC2._update, tdmpc2.py:316): the caller's
 * fp32 target tensors target[layer] = {weight, bias, ln.weight, ln.bias} of _target_Qs_params (stacked over num_q; the
 * LayerNorm entries of layer 2 NULL) are lerped IN PLACE towards online->net[TDMPC2_NET_Q] with torch.lerp's forms
 * (t + tau (o - t) for tau < 0.5, else o - (o - t) (1 - tau)), and TDMPC2_NET_TARGET_Q is re-packed from the lerped values in
 * the same call: the lerp is part of the scan launch, every element is written once, and the packed target is the pack of the
 * tensors the caller now holds.  Launches: those of a one-net refresh (FP32 handles: 2).  Only online->net[TDMPC2_NET_Q] is
 * read.  TDMPC2_ERR_INVALID: tau outside [0, 1] or NaN, online Q missing from the table, a NULL target tensor. */
int tdmpc2_plan_soft_update_target(tdmpc2_plan_t *h, const tdmpc2_weight_table *online, float *const target[3][4], float tau,
                                   void *stream);

/* Packed weight file (the native counterpart of TDMPC2.save / load, tdmpc2.py:72-95).
 * export_packed copies everything the binds produced -- weights in MFMA fragment order (hi / lo split and scaled for the
 * SPLIT_F16 arithmetic), padded biases, LayerNorm parameters, task-embedding columns, per-layer scale records, the
 * transposed encoder, the target ensemble when bound -- into ONE host buffer of packed_size bytes; import_packed
 * restores a handle created with the same model dimensions, kernel family and arithmetic from such a buffer with plain
 * host-to-device copies (no packing kernels, no fp32 checkpoint on the device).  The blob is specific to (path, precision);
 * TDMPC2_ERR_INVALID on any mismatch.  Both synchronise `stream`. */
int tdmpc2_plan_packed_size(tdmpc2_plan_t *h, uint64_t *bytes);
int tdmpc2_plan_export_packed(tdmpc2_plan_t *h, void *host_buf, uint64_t bytes, void *stream);
int tdmpc2_plan_import_packed(tdmpc2_plan_t *h, const void *host_buf, uint64_t bytes, void *stream);

/* TDMPC2._estimate_value on given action sequences (stage-wise parity).
 *   actions [E,H,N,A], pi_eps [E,N,A], qidx [E,2] -> value [E,N] (before nan_to_num). */
int tdmpc2_plan_estimate_value(tdmpc2_plan_t *h, int n_envs, const float *z0, const float *task_emb,
                               const float *act_mask, const float *disc_pow, const float *actions,
                               const float *pi_eps, const int32_t *qidx, float *value, void *stream);

/* The same, additionally dumping the activation tile after every fused phase (layer-level parity:
 * each fused stage is checked against its unfused counterpart at its own scale).
 *   trace_tiles   [E*N/64, 5H+7, 64, L]  per 64-row tile, in execution order: for t < H {reward h1, reward h2,
 *                 dynamics h1, dynamics h2, z_{t+1}}, then {pi h1, pi h2, z_H, Q_a h1, Q_a h2, Q_b h1, Q_b h2}
 *   trace_scalars [E, N, H+2+A]          r_0..r_{H-1}, Q_a, Q_b, a_H[A]
 * Either may be NULL.  LAYERED handles dump scalars only (trace_tiles must be NULL there). */
int tdmpc2_plan_estimate_value_trace(tdmpc2_plan_t *h, int n_envs, const float *z0, const float *task_emb,
                                     const float *act_mask, const float *disc_pow, const float *actions,
                                     const float *pi_eps, const int32_t *qidx, float *value,
                                     float *trace_tiles, float *trace_scalars, void *stream);

/* Elite select + refit on given values (stage-wise parity).
 *   value [E,N] in/out (nan_to_num applied), actions [E,H,N,A], act_mask [E,A]|NULL
 *   -> mean,std [E,H,A]; score [E,K]; elite_idx [E,K] (outputs may be NULL). */
int tdmpc2_plan_refit(tdmpc2_plan_t *h, int n_envs, float *value, const float *actions,
                      const float *act_mask, float *mean, float *std, float *score,
                      int32_t *elite_idx, void *stream);

/* ONE plan sharded over G GPUs (last row: worth it for 317M-class models at E = 1).  The N sample rows of
 * every plan are split over the ranks; weights, set-up, action sampling (same tape or same Philox seed on every rank) and
 * the elite selection + refit are replicated.  Per plan: shard_begin once (= the prologue of tdmpc2_plan_run: warm start,
 * policy-prior trajectories, tdmpc2.py:154-170); per CEM iteration shard_values for this rank's rows
 * [row_begin, row_end) (a multiple of 64 rows, FUSED, or 128, LAYERED) writing value[E, N] at those rows only, then the
 * HOST all-gathers the value slices (RCCL, N * 4 bytes per plan), then shard_refit on the complete value[E, N]
 * (tdmpc2.py:184-197; at iter == iterations - 1 also the final pick, tdmpc2.py:199-206).  With one rank and the full row
 * range the three calls compute what tdmpc2_plan_run computes.  tdmpc2_amd/dist.py: sharded_plan.
 * Faults: a bounded inter-workgroup wait that gave up in ANY of the plan's calls makes the final pick return NaN actions and
 * keep prev_mean (every call consumes the handle's error word, so the library keeps a second, sticky word per plan in flight);
 * tdmpc2_plan_take_fault after a sync reports it, and every rank has to plan the step again (dist.sharded_plan all-reduces the
 * verdict).  The sticky word is written by the host: synchronise with the final shard_refit (the caller needs its action
 * anyway) before the next shard_begin on the same handle. */
int tdmpc2_plan_shard_begin(tdmpc2_plan_t *h, int n_envs, const float *z0, const float *task_emb, const float *act_mask,
                            const float *prev_mean, const uint8_t *t0, const tdmpc2_noise *tape, uint64_t seed, void *stream);
int tdmpc2_plan_shard_values(tdmpc2_plan_t *h, int n_envs, int iter, int row_begin, int row_end, const float *z0,
                             const float *act_mask, const float *disc_pow, const tdmpc2_noise *tape, uint64_t seed,
                             float *value, void *stream);
int tdmpc2_plan_shard_refit(tdmpc2_plan_t *h, int n_envs, int iter, float *value, const float *act_mask, float *prev_mean,
                            int eval_mode, const tdmpc2_noise *tape, uint64_t seed, float *action, const tdmpc2_debug *dbg,
                            void *stream);

/* Tuning knobs that never change results beyond fp32 round-off.  key TDMPC2_TUNE_ROWS_PER_WORKGROUP: sample rows a
 * fused split-arithmetic rollout workgroup owns -- 0 = automatic (32 when a call brings too few plans to occupy the
 * chip, i.e. single-environment latency; 64 otherwise), or 32 / 64 to force one.  key TDMPC2_TUNE_FOLD_REFIT (fused
 * family): 1 = the last workgroup of a plan to finish its rollouts does the elite selection + refit (tdmpc2.py:184-206)
 * inside the rollout launch, one launch per CEM iteration; 0 = always a launch of its own (k_refit); 2 (default) = inside
 * the rollout launch when the call's workgroups fit the chip in one round (few plans: single-environment latency), a
 * launch of its own otherwise (many plans: the in-launch refits would delay the next round of workgroups).
 * key TDMPC2_TUNE_CLUSTER (fused family, f16x2-split arithmetic): single-plan latency path -- every 512-wide
 * layer of a 32-row sample tile is split over a cluster of 8 workgroups on 8 CUs that exchange the layer's raw sums through
 * L2 (tdmpc2_amd/csrc/cluster_kernels.cuh); used when all of a call's clusters fit the chip at once (one or two plans of
 * 512 samples on 256 CUs).  0 = never, 1 = whenever the call fits, 2 (default) = 1, and for a SINGLE non-episodic plan every
 * launch -- the first included, which also folds the policy-prior trajectories in -- gives each tile a second cluster that runs
 * the reward chain (and the second Q head) beside the dynamics chain (cluster2_kernels.cuh: all 256 CUs, 16 instead of 23 hand-overs on the critical path; identical values).
 * key TDMPC2_TUNE_FUSE_LN (layered family, f16x2-split arithmetic): 1 (default) = the LayerNorm + Mish / SimNorm + operand split
 * of every NormedLinear (tdmpc2/common/layers.py:94-118) runs in the epilogue of its GEMM -- the column blocks of a row block
 * exchange per-row (mean, M2) partials through L2, a bounded wait like the cluster path's (tdmpc2_plan_take_fault) --;
 * 0 = fp32 pre-activations to HBM and a row kernel per layer.
 * key TDMPC2_TUNE_REARM_AFTER: consecutive clean calls after which a handle that was downgraded by a reported wait goes back to
 * the CLUSTER / FUSE_LN paths (default 8 -- 64 before ABI 8; 0 = never: the downgrade is for good, as in ABI <= 6).  See
 * tdmpc2_plan_take_fault.
 * key TDMPC2_TUNE_SAFE_ONCE (ABI 8): 1 = the NEXT whole plan on this handle (tdmpc2_plan_run / run_obs, or shard_begin .. the last
 * shard_refit) runs on the paths without inter-workgroup waits, whatever CLUSTER / FUSE_LN say; the caller's settings, the
 * downgrade state and the re-arm counter are not touched and the flag clears itself when that plan has been enqueued (the
 * re-plan of a sharded plan after a reported wait: dist.sharded_plan).
 * key TDMPC2_TUNE_KSPLIT (ABI 8; layered family, f16x2-split arithmetic): the 256 x 256 output tiles of a GEMM's last, partly
 * filled round of the chip can each be computed by 2-4 workgroups over disjoint K ranges whose partial sums meet in a workspace
 * and are added in a fixed order (tdmpc2_amd/csrc/layered_wide.cuh, tile_order.h: gemm_w_order).  0 = never: every tile whole -- a
 * plan then computes the same bits alone, in any batch and with its rows split over ranks; 1 = whenever the round arithmetic
 * says so (measured: slower on launches that fill the chip -- the partial sums' traffic); 2 (default) = only for launches of
 * 16 .. 128 tiles, which leave most of the chip idle (one or two plans of the 317M model: single-plan latency -9 %).  Same values
 * to fp32 round-off (1e-5 of the trajectory values); the bits of a plan then depend on how many plans share the call.
 * key TDMPC2_TUNE_FEWROW (ABI 9; layered family, f16x2-split arithmetic): 1 (default) = calls with so few sample rows that one round
 * of 64 x 256 output tiles does not fill the chip -- single plans, the reference's own call pattern (evaluate.py:80): the 48M
 * model up to 4 plans, the 317M model 1 -- run every nn.Linear as K-PARTS of such tiles (tdmpc2_amd/csrc/layered_mid.cuh: an 8-wave
 * LDS-DMA ring GEMM writing raw partial sums) followed by a row kernel that adds the parts in a fixed order and applies the
 * NormedLinear / two-hot / policy-head math; two chains per launch, one stream, no workgroup ever waits for another one (no fault
 * path).  Same values to fp32 round-off; needs TDMPC2_TUNE_KSPLIT != 0 (with KSPLIT = 0 a plan keeps computing the same bits alone and
 * in any batch).  0 = the per-layer tiles of the batch path for every call size.
 * key TDMPC2_TUNE_WAIT_US (ABI 9): the wall-clock bound of the inter-workgroup waits in microseconds (default 5000; 100 .. 10 000 000).
 * A handle that shares its GPU with another process's multi-millisecond kernels may want more; the hot path never reads it (the
 * clock is only consulted from the 256th poll of a wait on).
 * keys TDMPC2_TUNE_EXPERT + tdmpc2_expert_knob (ABI 9): the measurement knobs of the layered family's tile choice -- thresholds between
 * kernels that compute the same values to fp32 round-off.  They were environment variables of the library until ABI 8; the library
 * now reads exactly the environment variables listed in INTEGRATION.md section C and nothing else.  value INT32_MIN = the default.
 * key TDMPC2_TUNE_POLICY_ROUTE (ABI 11): the route of tdmpc2_plan_pi / act_pi / act_pi_pix -- 0 (default) = auto (policy_route.h),
 * 1 = the row route (where its LDS holds the widest layer), 2 = the spread route. */
enum tdmpc2_tuning { TDMPC2_TUNE_ROWS_PER_WORKGROUP = 0, TDMPC2_TUNE_FOLD_REFIT = 1, TDMPC2_TUNE_CLUSTER = 2, TDMPC2_TUNE_FUSE_LN = 3,
                     TDMPC2_TUNE_REARM_AFTER = 4, TDMPC2_TUNE_SAFE_ONCE = 5, TDMPC2_TUNE_KSPLIT = 6, TDMPC2_TUNE_FEWROW = 7,
                     TDMPC2_TUNE_WAIT_US = 8,
                     TDMPC2_TUNE_POLICY_ROUTE = TDMPC2_TUNE_WAIT_US + 1, /* = 9 (tests/test_host_logic.py pins ABI 10's literal keys) */
                     TDMPC2_TUNE_EXPERT = 100 };
/* (what each knob decides, its default and the values it accepts -- anything else: TDMPC2_ERR_INVALID: tdmpc2_amd/csrc/layer_route.h) */
enum tdmpc2_expert_knob { TDMPC2_X_GEMM_W256_MIN = 0, TDMPC2_X_GEMM_W_SPLIT_MIN, TDMPC2_X_GEMM_W_SPLIT_MAX, TDMPC2_X_GEMM_W_SPLIT_OVH,
                          TDMPC2_X_KSPLIT_AUTO_LO, TDMPC2_X_KSPLIT_AUTO_MIN, TDMPC2_X_GEMM_W_XCD_ROWS, TDMPC2_X_GEMM_NCT1,
                          TDMPC2_X_GEMM_WIDE_MIN, TDMPC2_X_GEMM_RT4, TDMPC2_X_GEMM_FILL_PERMILLE, TDMPC2_X_GEMM_FILL_HEAD_PERMILLE,
                          TDMPC2_X_GEMM_SD1, TDMPC2_X_GEMM_XCD_ROWS, TDMPC2_X_GEMM_COL_PAD, TDMPC2_X_TWOHOT_UNFUSED, TDMPC2_X_Z0_SHARED_OFF,
                          TDMPC2_X_MID_PARTS_MAX, TDMPC2_X_MID_FUSE_LN, TDMPC2_X_MID_SPLIT_XCD, TDMPC2_X_MID_PIFOLD, TDMPC2_X_COUNT };
int tdmpc2_plan_set_tuning(tdmpc2_plan_t *h, int key, int value);

/* Fault report of the paths whose workgroups wait for each other: the cluster path (TDMPC2_TUNE_CLUSTER) and the NormedLinear
 * epilogue inside the layered family's GEMMs (TDMPC2_TUNE_FUSE_LN).  Those waits are bounded by the wall clock (5 ms of the constant
 * 100 MHz clock -- a poll count worth a third of a second before ABI 8; a healthy wait is microseconds to one tile's run time); when one gives up -- another process or a foreign kernel held
 * the compute units -- the call in flight is invalid AND SAYS SO: a plan's action[E, A] comes back as NaN with prev_mean left as
 * it was (the step can simply be planned again); tdmpc2_plan_td_target / policy_value (LAYERED family) return NaN in every
 * element of out[] (and action[]).  The reference has no analogue (its only guard is the nan_to_num of tdmpc2.py:184).
 * Call this after synchronising the stream of such a call: *faults = number of invalid calls since the last take_fault (0 = none).
 * After a fault the handle runs the paths without inter-workgroup waits; it switches back to the fast ones after
 * TDMPC2_TUNE_REARM_AFTER (default 8) consecutive clean calls, doubling that number (up to 4096) every time a fault follows a
 * re-arm and forgetting the back-off after a long clean run; an explicit tdmpc2_plan_set_tuning(CLUSTER / FUSE_LN) re-arms at
 * once.  Calls enqueued back to back without a synchronisation in between each carry their own verdict: the word a call's last
 * kernel reads is raised on the device and cleared by the NEXT call in stream order, never by the host (which looks at a
 * separate sticky word with one atomic exchange: the count reported here is "looks that found it set", at most one per API
 * call -- a lower bound on the waits that gave up).  The later calls of a
 * sharded plan (shard_values / shard_refit) do not clear it: a wait that gave up in any iteration invalidates the final pick. */
int tdmpc2_plan_take_fault(tdmpc2_plan_t *h, int *faults);

/* The verdict of the call(s) in flight WITHOUT a host synchronisation (ABI 8): enqueues a 4-byte copy of the device-visible
 * verdict word (0 = no bounded wait has given up since the last call that cleared it: tdmpc2_plan_run*, shard_begin, ...) into
 * dst_dev[0] on `stream`, behind the kernels enqueued so far.  A rank of a sharded plan appends the word to the value slice it
 * all-gathers anyway, so that every rank learns every rank's verdict with the one synchronisation the caller needs for the
 * action (dist.sharded_plan); the host-side bookkeeping (downgrade, re-arm, take_fault) is untouched.  No reference analogue. */
int tdmpc2_plan_fault_word(tdmpc2_plan_t *h, uint32_t *dst_dev, void *stream);

/* The fault history of a handle (no synchronisation, nothing consumed): how often a bounded wait has given up, how long ago the
 * last one was, whether the handle is currently on the downgraded paths and how far the re-arm counter has got. */
typedef struct tdmpc2_fault_info {
    int32_t faults_total;        /* bounded waits that gave up since tdmpc2_plan_create */
    int32_t rearms;              /* times the fast paths were switched back on */
    int32_t degraded;            /* 1: running the paths without inter-workgroup waits right now */
    int32_t clean_calls;         /* consecutive clean calls since the downgrade (re-arm at rearm_after) */
    int32_t rearm_after;         /* current threshold (doubles after a re-arm, TDMPC2_TUNE_REARM_AFTER resets it; 0: never) */
    int32_t reserved;
    double seconds_since_fault;  /* wall-clock seconds since the last fault was noted; -1: never */
} tdmpc2_fault_info;
int tdmpc2_plan_fault_info(tdmpc2_plan_t *h, tdmpc2_fault_info *info);

/* Live timing of the dominant (rollout) stage: after set_profiling(h, n > 0) every rollout launch
 * (FUSED: one ks_rollout kernel; LAYERED: the GEMM / row-kernel sequence of one CEM iteration's
 * _estimate_value) is bracketed by HIP events recorded on the caller's stream (up to n are kept;
 * n = 0 turns it off).  profile_read synchronises those events, returns their summed duration and the number of
 * launches measured, and rewinds the buffer. */
int tdmpc2_plan_set_profiling(tdmpc2_plan_t *h, int max_launches);
int tdmpc2_plan_profile_read(tdmpc2_plan_t *h, float *rollout_ms_total, int *rollout_launches);

/* Replay buffer (additions to ABI 14; the version number stays 14): the reference's Buffer (tdmpc2/common/buffer.py:13-115), a
 * torchrl ReplayBuffer with SliceSampler(num_slices = batch_size, traj_key = 'episode', strict_length = True), restated as an
 * episode ring on the device.  A handle of its own: it needs no planner and shares nothing with one.
 *   Storage   `capacity` steps; per step up to 8 FIELDS (obs, action, reward, terminated, task, ...) of row_bytes opaque bytes each
 *             (fp32 state rows, uint8 [9, 64, 64] frame stacks, an int64 task id): the library copies bytes and never interprets
 *             them.  Device memory only, one allocation made by create; there is no host-resident storage.
 *   Ring      a step's LOGICAL index is the count of steps written before it (64-bit); its physical row is logical % capacity.
 *             Writing evicts the oldest logical steps; an episode that loses its front stays a shorter trajectory (as in a torchrl
 *             storage whose cursor has passed it).
 *   Table     S = slice_len (= horizon + 1).  An episode is ELIGIBLE while it has at least S live steps; the eligible ones are kept
 *             as {first_logical, len} in a device-side ring of capacity / S + 1 entries, appended at the tail, shrunk or popped at
 *             the head.  Shorter episodes occupy storage and count in num_eps but are never sampled.
 *   Sampling  slice b of a call takes ONE Philox4x32-10 draw r, counter (b, site 8, 0, call), key = seed:
 *             episode e = (u64(r.x) * eligible) >> 32 of the table (uniform over eligible episodes), start s = (u64(r.y) *
 *             (len_e - S + 1)) >> 32 (uniform over the starts that fit).  This is what torchrl documents for a strict-length slice
 *             sampler; torchrl itself was not run against it.
 *   Outputs   time-major, as Buffer._prepare_batch returns them (buffer.py:93-110): a field that delivers steps
 *             [step_first, step_first + step_count) of the slice writes [step_count, batch, row_bytes] bytes.
 * The call counter and the table's head / count live on the device: a tdmpc2_buffer_sample captured in a hipGraph draws fresh
 * slices at every replay and sees episodes added between replays.  sample is two launches (draw, grouped gather over all
 * fields), allocates nothing and never synchronises the host.  A handle is not re-entrant. */
typedef struct tdmpc2_buffer tdmpc2_buffer_t;
#define TDMPC2_BUFFER_MAX_FIELDS 8
typedef struct tdmpc2_buffer_field {
    uint32_t row_bytes;                /* bytes per step, > 0 */
    int32_t step_first, step_count;    /* the steps of a slice this field delivers: obs 0, S; action / reward 1, S - 1; task 0, 1 */
} tdmpc2_buffer_field;
typedef struct tdmpc2_buffer_cfg {
    uint64_t capacity;                 /* steps; >= slice_len */
    int32_t slice_len;                 /* S = horizon + 1 >= 2 */
    int32_t device;                    /* HIP device ordinal */
    int32_t n_fields;                  /* 1 .. 8 */
    int32_t max_batch;                 /* slices per sample call the workspace is reserved for; 0 = 4096 */
    tdmpc2_buffer_field field[TDMPC2_BUFFER_MAX_FIELDS];
} tdmpc2_buffer_cfg;
typedef struct tdmpc2_buffer_info {
    uint64_t num_eps;                  /* episodes ever written (Buffer.num_eps, buffer.py:33-36) */
    uint64_t live_steps;               /* min(steps ever written, capacity) */
    uint64_t cursor;                   /* steps ever written: the next step's logical index */
    uint32_t eligible;                 /* entries in the table */
    uint32_t next_call;                /* the device's call counter: the `call` of the next sample */
} tdmpc2_buffer_info;
/* Buffer.__init__ + _init (buffer.py:13-67).  create validates, sizes and builds the host side only; like the reference's lazy
 * storage, the device memory -- storage, table, state words and the draw workspace, ONE allocation -- is made by the first add /
 * load (keep that call outside a hipGraph capture).  TDMPC2_ERR_INVALID (the device is never touched): NULL cfg / out,
 * slice_len < 2, capacity < slice_len, n_fields outside [1, 8], a field with row_bytes == 0 or steps outside the slice,
 * max_batch < 0.  A failed allocation (in add / load): TDMPC2_ERR_HIP, nothing is left allocated and the handle is unchanged
 * (there is no host fallback, unlike buffer.py:61-63).  The host keeps a mirror of the table: 16 bytes per capacity / S. */
int tdmpc2_buffer_create(const tdmpc2_buffer_cfg *cfg, tdmpc2_buffer_t **out);
void tdmpc2_buffer_destroy(tdmpc2_buffer_t *b);
/* Buffer.add (buffer.py:84-91): ONE episode of `steps` steps.  fields[f]: DEVICE pointer to [steps, row_bytes of field f].  Per
 * field at most two copies around the physical wrap, then one tiny kernel that takes the new table / state values by value:
 * everything is ordered by `stream`.  Host cost O(table entries touched).  TDMPC2_ERR_INVALID: NULL handle / fields / a NULL
 * field pointer, steps < 1, an episode longer than capacity. */
int tdmpc2_buffer_add(tdmpc2_buffer_t *b, uint32_t steps, const void *const *fields, void *stream);
/* Buffer.load (buffer.py:69-82): n_episodes episodes of `steps` steps each, fields[f] [n_episodes, steps, row_bytes]; the state
 * it leaves (table, samples) is that of n_episodes add calls.  The table entries are filled arithmetically in one launch; steps
 * that the same load would evict are not copied.  Refusals as add (n_episodes < 1 too). */
int tdmpc2_buffer_load(tdmpc2_buffer_t *b, uint64_t n_episodes, uint32_t steps, const void *const *fields, void *stream);
/* Buffer.sample + _prepare_batch (buffer.py:93-115): `batch` slices.  outs[f]: DEVICE pointer to [step_count of f, batch,
 * row_bytes of f], or NULL (field not wanted); index_out: DEVICE int64 [batch], the logical index of step 0 of every slice, or
 * NULL.  Accesses are 16 bytes wide where row_bytes % 16 == 0 and outs[f] is 16-byte aligned, 4 bytes where both allow that, else
 * single bytes.  TDMPC2_ERR_INVALID: NULL handle / outs, batch outside [1, max_batch]; TDMPC2_ERR_STATE: no eligible episode (by
 * the host's count).  A captured replay that meets an empty table on the device reads nothing, leaves the outputs untouched and
 * writes -1 to index_out. */
int tdmpc2_buffer_sample(tdmpc2_buffer_t *b, int32_t batch, void *const *outs, int64_t *index_out, uint64_t seed, void *stream);
/* Buffer.num_eps and the ring's state (buffer.py:28-36).  next_call is read from the device: the call synchronises `stream`. */
int tdmpc2_buffer_stats(tdmpc2_buffer_t *b, tdmpc2_buffer_info *info, void *stream);
/* The call counter of the NEXT sample (the reproducibility handle torch.manual_seed gives the reference's sampler), stream-ordered. */
int tdmpc2_buffer_set_call_counter(tdmpc2_buffer_t *b, uint32_t next_call, void *stream);

/* ---- trainable layer (additions to ABI 14): forward and backward of the one layer every MLP of the model is made of ----------
 * NormedLinear (tdmpc2/common/layers.py:94-118): Linear -> dropout mask -> LayerNorm -> Mish, or -> SimNorm(simnorm_dim) on the
 * last layer of the encoder and the dynamics; kind LINEAR is the plain nn.Linear that closes the other MLPs.  `groups` stacks
 * identically shaped layers (the Q ensemble).  No handle, no state: a call is its descriptor, its pointers and, for backward, a
 * caller-owned workspace.  A call allocates nothing and never synchronises the host, so it can be captured in a hipGraph.
 *   Layout    contiguous fp32 on the current device.  G = groups, R = rows, K = in_dim, N = out_dim.  w [G, N, K]; b, ln_w, ln_b
 *             [G, N]; y, pre, mask, dy [G, R, N]; x, dx [G, R, K], or [R, K] with shared_x (the ensemble's first layer reads one
 *             input; dx is then the sum over groups, one chain in the order g = 0 .. G - 1); stat [G, R, 2] = (mean, rstd).
 *   Forward   pre = (x w^T + b) * mask (mask optional: dropout's 0 or 1 / (1 - p)); stat from F.layer_norm's biased variance,
 *             rstd = 1 / sqrt(var + ln_eps); y = mish(u) (softplus threshold 20) or softmax over contiguous groups of simnorm_dim
 *             with the max subtracted, u = (pre - mean) rstd ln_w + ln_b.  LINEAR: y = (x w^T + b) * mask; ln_*, pre, stat ignored.
 *   Backward  OVERWRITES dx [as x], dw [G, N, K], db, dln_w, dln_b [G, N].  dx may be NULL (a first layer); the parameter
 *             gradients may be NULL together (frozen parameters; LINEAR has two, dw and db, and ignores dln_*).  ln_b is read
 *             because u is recomputed from pre and stat rather than stored.
 *   Numerics  exact fp32.  The three contractions run on v_mfma_f32_32x32x2_f32: every output element is one fmaf chain in
 *             rising reduction index, never split, so a row's y and dx do not depend on the other rows of the call and results
 *             are bit-identical from run to run.  Row and column sums have fixed orders (tdmpc2_amd/csrc/layer_grad_route.h).
 * TDMPC2_ERR_INVALID before the device is touched: NULL descriptor or required pointer; groups, rows, in_dim or out_dim < 1;
 * unknown kind; SIMNORM with simnorm_dim < 1 or out_dim % simnorm_dim != 0; shared_x with groups == 1; ws NULL or ws_bytes too
 * small (a LINEAR backward without mask needs none); only some of the parameter gradients; dx and all of them NULL.  A descriptor whose GEMM grids would pass 2^31 workgroups:
 * TDMPC2_ERR_UNSUPPORTED, also before the device is touched. */
enum { TDMPC2_LAYER_LINEAR = 0, TDMPC2_LAYER_MISH = 1, TDMPC2_LAYER_SIMNORM = 2 };
typedef struct tdmpc2_layer_desc {
    int32_t kind, groups, rows, in_dim, out_dim, shared_x, simnorm_dim;
    float ln_eps;
} tdmpc2_layer_desc;   /* 32 bytes, no padding */
/* Bytes of workspace a backward call of this descriptor needs.  Host only: never touches a device. */
int tdmpc2_layer_workspace_bytes(const tdmpc2_layer_desc *desc, size_t *backward_ws_bytes);
int tdmpc2_layer_forward(const tdmpc2_layer_desc *desc, const float *x, const float *w, const float *b, const float *ln_w,
                         const float *ln_b, const float *mask, float *y, float *pre, float *stat, void *stream);
int tdmpc2_layer_backward(const tdmpc2_layer_desc *desc, const float *x, const float *w, const float *ln_w, const float *ln_b,
                          const float *pre, const float *stat, const float *mask, const float *dy, float *dx, float *dw, float *db,
                          float *dln_w, float *dln_b, void *ws, size_t ws_bytes, void *stream);

/* ---- optimiser step (additions to ABI 14): gradient clip and Adam over flat arenas --------------------------------------------
 * What the learner does between backward and the re-pack (tdmpc2/tdmpc2.py:22-31, 227-230, 307-310): clip_grad_norm_ over an
 * optimiser's parameters, Adam, zero_grad -- in three launches whatever the number of tensors.  A handle of its own: it shares
 * nothing with a planner handle, and the re-pack stays tdmpc2_plan_refresh_weights, issued after the step.  No weight decay,
 * amsgrad or maximize (the reference uses none).
 *   Segments  a handle covers a fixed list of fp32 parameter tensors ("segments"), each in a group with its own lr (the reference's
 *             encoder group; an empty group is allowed).  Parameters stay the model's own tensors, addressed by pointer, aligned to
 *             4 bytes or better (a view into a stacked tensor may be misaligned for 16-byte accesses: whole quads of such a segment
 *             are read and written as four dwords, its 1 .. 3 tail elements one by one).
 *   Arenas    gradients and both moments are three flat fp32 arrays of arena_floats floats that the CALLER owns and passes to every
 *             step; segment i starts at offsets[i] (tdmpc2_optim_layout), every segment padded to a multiple of 4 floats.  The
 *             padding must be zero at the first step and stays zero: the kernels write zeros there.
 *   Step      in stream order (tdmpc2_amd/csrc/optim_route.h: chunks, the norm's order and its longest addition chain):
 *             1. norm = L2 norm of the whole gradient arena in a fixed order -- no float atomics, no waits between workgroups,
 *                bit-identical from run to run and independent of the grid;
 *             2. c = min(1, max_norm / (norm + 1e-6)) in fp32 (torch's form; always multiplied in; a NaN norm gives a NaN c);
 *             3. device scalars, so that a captured step advances on replay: step += 1 (int64), b1p *= beta1, b2p *= beta2 (fp64
 *                running products from 1, betas widened from fp32; no pow), ss_g = fp32(lr_g / (1 - b1p)) per group and
 *                bc = fp32(sqrt(1 - b2p)), computed in fp64 and rounded once;
 *             4. per element, every operation a separately rounded fp32 operation in this order (divide and sqrt correctly
 *                rounded, no contraction), a1 = fp32(1 - beta1), a2 = fp32(1 - beta2) rounded once from the fp64 difference:
 *                    g = g * c;  m = m + (g - m) * a1;  v = v * beta2 + (g * a2) * g;  d = sqrt(v) / bc + eps;  p = p - ss_g * (m / d)
 *             5. zero_grad != 0: g = 0 in the same pass (zero_grad with the tensors kept); zero_grad == 0: the CLIPPED gradient is
 *                stored back, as torch's clip_grad_norm_ scales in place.
 *             EVERY segment is stepped on every call: a zero gradient counts as a gradient.  This equals the reference, where each
 *             parameter of an optimiser receives a gradient on every step.  Non-finite gradients propagate exactly as in torch with
 *             error_if_nonfinite=False: nothing filters them.
 *   norm_out  DEVICE pointer to one float, or NULL.  A step allocates nothing, copies nothing from the host and never
 *             synchronises: it can be captured in a hipGraph.
 * TDMPC2_ERR_INVALID before the device is touched: NULL cfg / out / lr / segs; n_segs < 1, n_groups < 1, a count < 1, a group out
 * of range, a NULL param; betas outside [0, 1), eps <= 0, max_norm <= 0, or NaN in any of them; a NULL arena or handle in step;
 * step < 0 in set_step.  An arena of more than 2^31 chunks of 2048 floats: TDMPC2_ERR_UNSUPPORTED. */
typedef struct tdmpc2_optim tdmpc2_optim_t;
typedef struct tdmpc2_optim_seg {
    float *param;      /* DEVICE pointer to `count` contiguous floats */
    int64_t count;
    int32_t group, reserved;
} tdmpc2_optim_seg;
typedef struct tdmpc2_optim_cfg {
    int32_t device, n_segs, n_groups, reserved;
    float beta1, beta2, eps, max_norm;
    const float *lr;                 /* [n_groups], host */
    const tdmpc2_optim_seg *segs;    /* [n_segs], host */
} tdmpc2_optim_cfg;
/* offsets [n_segs] and the length of each arena, in floats.  Host only: never touches a device. */
int tdmpc2_optim_layout(const tdmpc2_optim_cfg *cfg, int64_t *offsets, int64_t *arena_floats);
/* Validates, then makes the handle's one device allocation (segment table, scalars, the norm's partial sums) and uploads it once. */
int tdmpc2_optim_create(const tdmpc2_optim_cfg *cfg, tdmpc2_optim_t **out);
void tdmpc2_optim_destroy(tdmpc2_optim_t *o);
int tdmpc2_optim_step(tdmpc2_optim_t *o, float *grad, float *exp_avg, float *exp_avg_sq, int zero_grad, float *norm_out,
                      void *stream);
/* The device's step counter; synchronises `stream`. */
int tdmpc2_optim_get_step(tdmpc2_optim_t *o, int64_t *step, void *stream);
/* Resume a saved optimiser: step, and b1p / b2p rebuilt by the same repeated fp64 product, so the scalars of the next step are
 * bit-identical to those of an uninterrupted run.  Synchronises `stream`; host cost O(step). */
int tdmpc2_optim_set_step(tdmpc2_optim_t *o, int64_t step, void *stream);

/* ---- loss seeds (additions to ABI 14): the four losses of TDMPC2._update and the gradients they send into the layer backward ---
 * The arithmetic between the last layer's output and loss.backward() (tdmpc2/tdmpc2.py:272-304): consistency (mse of the rollout's
 * latents against encode(obs[1:])), reward and value (soft_ce: log_softmax against two_hot, math.py:5-9, 58-71), termination
 * (binary_cross_entropy_with_logits), their coefficient-weighted total, and d total / d (z_pred, reward_logits, q_logits,
 * term_logit).  No handle, no state: a call is its descriptor, its pointers and, for the forward, a caller-owned workspace.  A call
 * allocates nothing and never synchronises the host, so forward + backward can be captured in a hipGraph.  No atomics, no wait
 * between workgroups: the same inputs give the same bits.
 *   Layout    contiguous fp32 on the current device.  T = steps, B = batch, L = latent_dim, NB = num_bins, Q = num_q.
 *             z_pred, next_z [T, B, L] (zs[1:], the outputs of `next`, and encode(obs[1:])); reward_logits [T, B, NB]; q_logits
 *             [Q, T, B, NB] (the layout of Q(..., 'all')); reward, td_target, term_logit, terminated [T, B].  term_logit and
 *             terminated are both NULL exactly when episodic == 0.
 *   Descriptor  vmin, vmax, bin_size, rho and the coefficients are fp32 and are widened, never re-derived (bin_size is the
 *             caller's (vmax - vmin) / (NB - 1)).
 *   Forward   2 launches.  losses [5] = consistency, reward, value, termination, total and step_means [4, steps] (may be NULL),
 *             both defined exactly as for tdmpc2_plan_model_losses above.  Per-row terms go to ws (tdmpc2_loss_workspace_bytes) and
 *             ONE workgroup adds them in the fixed order that tdmpc2_amd/csrc/loss_grad_route.h publishes.
 *   Backward  1 launch over all row kinds; OVERWRITES the outputs that are not NULL (a NULL output drops its rows from the grid).
 *             Nothing is saved by the forward: a row's max and sum are computed again.  With g = *grad_total (device float[1];
 *             NULL = 1) and w_t = rho^t, every per-step constant computed on the host in fp64 and rounded once, g multiplied in as
 *             one fp32 factor (g = 2 doubles every output bit for bit):
 *               d_z_pred[t,b,l]        = c_t (z_pred - next_z),             c_t = g fp32(consistency_coef 2 w_t / (T B L))
 *               d_reward_logits[t,b,k] = c_t (softmax_k S - th_k),          c_t = g fp32(reward_coef w_t / (T B))
 *               d_q_logits[q,t,b,k]    = the same against td_target[t,b],   c_t = g fp32(value_coef w_t / (T Q B))
 *               d_term_logit[t,b]      = c (sigmoid(x) - y),                c   = g fp32(termination_coef / (T B))
 *             th is the two-hot row of math.two_hot (1 - off at the lower bin, off at the upper one, which wraps to bin 0 at vmax
 *             with off = 0) and S = (1 - off) + off in fp32, as the backward of torch's log_softmax sums its incoming gradient.
 *   Non-finite targets: a NaN in reward / td_target / next_z / terminated makes NaN exactly the loss terms (that loss, its
 *             step_means entry, total) and the seed rows that read it; every other output keeps its bits.  +-Inf in reward /
 *             td_target clamps to vmin / vmax as in two_hot.
 * TDMPC2_ERR_INVALID before the device is touched: NULL descriptor or required pointer (all six model inputs, losses; backward: the
 * same inputs); steps outside [1, 8]; batch, latent_dim or num_q < 1; termination pointers that do not match episodic (d_term_logit
 * included); ws NULL or ws_bytes too small; a backward with all four outputs NULL.  TDMPC2_ERR_UNSUPPORTED, also before the device
 * is touched: num_bins < 2 (as model_losses refuses it); a grid past 2^31 workgroups. */
typedef struct tdmpc2_loss_desc {
    int32_t steps, batch, latent_dim, num_q, num_bins, episodic;
    float vmin, vmax, bin_size;
    float rho, consistency_coef, reward_coef, value_coef, termination_coef;
} tdmpc2_loss_desc;   /* 56 bytes, no padding */
/* Bytes of workspace a forward call of this descriptor needs.  Host only: never touches a device. */
int tdmpc2_loss_workspace_bytes(const tdmpc2_loss_desc *d, size_t *ws_bytes);
int tdmpc2_loss_forward(const tdmpc2_loss_desc *d, const float *z_pred, const float *next_z, const float *reward_logits,
                        const float *reward, const float *q_logits, const float *td_target, const float *term_logit,
                        const float *terminated, float *losses, float *step_means, void *ws, size_t ws_bytes, void *stream);
int tdmpc2_loss_backward(const tdmpc2_loss_desc *d, const float *z_pred, const float *next_z, const float *reward_logits,
                         const float *reward, const float *q_logits, const float *td_target, const float *term_logit,
                         const float *terminated, const float *grad_total, float *d_z_pred, float *d_reward_logits,
                         float *d_q_logits, float *d_term_logit, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TDMPC2_PLAN_H */
