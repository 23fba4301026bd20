// Host unit of observations and the policy prior.  Reference (nicklashansen/tdmpc2, paths relative to its root):
//   WorldModel.encode                      tdmpc2/common/world_model.py:103-112 (layers.enc / conv: tdmpc2/common/layers.py:136-164)
//   WorldModel.pi                          tdmpc2/common/world_model.py:144-184
//   TDMPC2.act (mpc and mpc = False)       tdmpc2/tdmpc2.py:98-120
//
// This unit: the state encoder's host side (launch_encode: the one-launch and the layer-at-a-time route; kernels in
// k_plan.hip) with tdmpc2_plan_encode / run_obs, the pixel encoder's planning routes (launch_encode_pix; k_plan.hip) with
// tdmpc2_plan_encode_pix / run_pix, its batch route (tdmpc2_plan_pix_batch_reserve / encode_pix_batch; k_pixel_batch.hip), and the
// policy prior (launch_pi; k_policy.hip) with tdmpc2_plan_pi / act_pi / act_pi_pix.  Shared services: plan_host.h.
#include "plan_host.h"

namespace {

// ---- state observations (k_plan.hip: encoder_kernels.cuh, encoder_params.h)
int launch_encode(tdmpc2_plan *h, int E, const float *obs, int obs_dim, const float *task_emb, float *z, hipStream_t st) {
    const tdmpc2_plan_cfg &c = h->cfg;
    if (!h->enc_layers) return fail(TDMPC2_ERR_STATE, "no encoder bound (tdmpc2_plan_bind_encoder)");
    EncodeArgs p{};
    int maxw = 0;
    for (int l = 0; l < h->enc_layers; ++l) {
        const tdmpc2_plan::Enc &L = h->enc[l];
        if (!L.bound) return fail(TDMPC2_ERR_STATE, "encoder layer %d of %d is not bound", l, h->enc_layers);
        const int exp_in = l == 0 ? obs_dim + c.task_dim : h->enc[l - 1].out;
        if (L.in != exp_in) return fail(TDMPC2_ERR_INVALID, "encoder layer %d takes %d inputs, the data brings %d", l, L.in, exp_in);
        if (L.in > ENC_MAX_IN)  // checked for every layer before the first launch
            return fail(TDMPC2_ERR_UNSUPPORTED, "encoder layer %d: %d inputs, at most %d (a layer's input row is held in %zu bytes of LDS)",
                        l, L.in, ENC_MAX_IN, ENC_GEMV_LDS_MAX);
        p.l[l] = EncLayerDev{L.wt, L.bias, L.g, L.b, L.in, L.out};
        maxw = std::max(maxw, std::max(L.in, L.out));
    }
    if (c.task_dim > 0 && !task_emb) return fail(TDMPC2_ERR_INVALID, "multitask encoder needs task_emb");
    if (maxw > ENC_WIDE) {  // layer-at-a-time across the chip (encoder_kernels.cuh)
        if (E > c.max_envs) return fail(TDMPC2_ERR_INVALID, "encoders wider than %d take at most max_envs = %d rows per call (got %d)", ENC_WIDE, c.max_envs, E);
        if (!h->enc_y || h->enc_ws_width < maxw) return fail(TDMPC2_ERR_STATE, "encoder workspace missing (bind every layer first)");
        for (int l = 0; l < h->enc_layers; ++l) {
            const tdmpc2_plan::Enc &L = h->enc[l];
            EncGemvArgs g{};
            g.wt = L.wt; g.bias = L.bias; g.in = L.in; g.out = L.out; g.y = h->enc_y;
            if (l == 0) { g.obs = obs; g.emb = task_emb; g.obs_dim = obs_dim; g.T = c.task_dim; }
            else { g.x = h->enc_x; g.ldx = h->enc[l - 1].out; }
            enc_launch_gemv(g, (L.out + 63) / 64, E, 256, ((size_t)L.in + 256) * 4, st);
            EncNormArgs n{};
            const bool last = l == h->enc_layers - 1;
            n.y = h->enc_y; n.g = L.g; n.b = L.b; n.out = last ? z : h->enc_x; n.width = L.out; n.last = last; n.simnorm_dim = c.simnorm_dim;
            enc_launch_norm(n, E, ENC_THREADS, st);
        }
        HIP_TRY(hipGetLastError());
        return 0;
    }
    p.nl = h->enc_layers; p.obs_dim = obs_dim; p.T = c.task_dim; p.maxw = maxw; p.simnorm_dim = c.simnorm_dim;
    p.obs = obs; p.task_emb = task_emb; p.z = z;
    const size_t lds = ((size_t)2 * maxw + ENC_THREADS / 64) * 4;
    enc_launch_encode(p, E, ENC_THREADS, lds, st);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- pixel observations (k_plan.hip: pixel_kernels.cuh, pixel_route.h)
int check_pix_call(tdmpc2_plan *h, int n_envs, int obs_dtype, int in_channels) {
    const tdmpc2_plan::Pix &P = h->pix;
    if (n_envs < 1 || n_envs > h->cfg.max_envs) return fail(TDMPC2_ERR_INVALID, "n_envs %d outside [1, %d]", n_envs, h->cfg.max_envs);
    if (obs_dtype != 0 && obs_dtype != 1) return fail(TDMPC2_ERR_INVALID, "obs_dtype %d (0 = uint8, 1 = float32)", obs_dtype);
    for (int l = 0; l < PIX_LAYERS; ++l)
        if (!P.bound[l]) return fail(TDMPC2_ERR_STATE, "no pixel encoder bound (layer %d; tdmpc2_plan_bind_pixel_encoder)", l);
    if (in_channels < 1 || in_channels > PIX_MAX_CIN)
        return fail(TDMPC2_ERR_INVALID, "pixel encoder: %d input channels outside [1, %d]", in_channels, PIX_MAX_CIN);
    if (in_channels != P.cin)
        return fail(TDMPC2_ERR_INVALID, "pixel encoder: the observation has %d channels, layer 0 was bound with %d", in_channels, P.cin);
    return 0;
}

int launch_encode_pix(tdmpc2_plan *h, int E, const void *obs, int obs_dtype, const int32_t *shift, float *z, hipStream_t st) {
    const tdmpc2_plan::Pix &P = h->pix;
    PixArgs p{};
    for (int l = 0; l < PIX_LAYERS; ++l) { p.wp[l] = P.wp[l]; p.bias[l] = P.bias[l]; }
    p.obs = obs; p.obs_u8 = obs_dtype == 0; p.cin = P.cin; p.C = P.C;
    p.shift = shift; p.tab = static_cast<const PixTap *>(P.tab); p.ws = P.ws; p.z = z;
    const PixRoute r = pix_route(E, P.C, h->num_cus);
    if (r.kind == PIX_PER_IMAGE) {
        pix_launch_image(p, r.g[0], st);
    } else {
        for (int l = 0; l < PIX_LAYERS; ++l) pix_launch_spread(l, p, r.g[l], st);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- policy prior (k_policy.hip: policy_kernels.cuh, policy_route.h)
int check_pol_call(tdmpc2_plan *h, const float *task_emb, const float *act_mask, const tdmpc2_policy_out *out) {
    if (!out || !out->action) return fail(TDMPC2_ERR_INVALID, "null policy output (out / out->action)");
    for (int l = 0; l < 3; ++l)
        if (!h->pol.bound[l]) return fail(TDMPC2_ERR_STATE, "policy layer %d is not bound (tdmpc2_plan_bind_policy)", l);
    if (h->cfg.multitask && (!task_emb || !act_mask)) return fail(TDMPC2_ERR_INVALID, "a multitask policy prior needs task_emb and act_mask");
    return 0;
}

// the state encoder as row-route layers (acting), with launch_encode's checks; maxw = its widest layer
int pol_enc_chain(tdmpc2_plan *h, int obs_dim, PolRowParams &p, int &maxw) {
    if (!h->enc_layers) return fail(TDMPC2_ERR_STATE, "no encoder bound (tdmpc2_plan_bind_encoder)");
    maxw = 0;
    for (int l = 0; l < h->enc_layers; ++l) {
        const tdmpc2_plan::Enc &L = h->enc[l];
        if (!L.bound) return fail(TDMPC2_ERR_STATE, "encoder layer %d of %d is not bound", l, h->enc_layers);
        const int exp_in = l == 0 ? obs_dim + h->cfg.task_dim : h->enc[l - 1].out;
        if (L.in != exp_in) return fail(TDMPC2_ERR_INVALID, "encoder layer %d takes %d inputs, the data brings %d", l, L.in, exp_in);
        p.enc[l] = PolLayerDev{L.wt, L.bias, L.g, L.b, L.in, L.out};
        maxw = std::max(maxw, std::max(L.in, L.out));
    }
    p.enc_nl = h->enc_layers;
    p.obs_dim = obs_dim;
    return 0;
}

// WorldModel.pi of n rows.  obs != null: the rows are observations and the encoder runs first -- inside the row-route launch when
// it is narrow enough for k_encode's own one-launch route, else through launch_encode into h->zenc.
int launch_pi(tdmpc2_plan *h, int n, const float *z, const float *obs, int obs_dim, const float *emb, const float *mask,
              const float *eps, uint64_t seed, int eval_mode, const tdmpc2_policy_out *out, hipStream_t st) {
    const tdmpc2_plan_cfg &c = h->cfg;
    const tdmpc2_plan::Pol &P = h->pol;
    const int L = c.latent_dim, T = c.task_dim, M = c.mlp_dim, A = c.action_dim, in0 = L + T;
    PolRowParams rp{};
    int maxw = std::max(in0, std::max(M, 2 * A)), rc;
    if (obs) {
        int enc_w = 0;
        if ((rc = pol_enc_chain(h, obs_dim, rp, enc_w))) return rc;
        const PolRoute r = pol_route(n, in0, M, A, std::max(maxw, enc_w), P.mode);
        if (enc_w <= ENC_WIDE && r.kind == POL_ROW) {
            maxw = std::max(maxw, enc_w);
            rp.obs = obs;
        } else {  // the encoder's own route, unchanged, then the policy from its latents
            if ((rc = launch_encode(h, n, obs, obs_dim, emb, h->zenc, st))) return rc;
            rp.enc_nl = 0;
            z = h->zenc;
        }
    }
    PolHeadArgs hd{};
    hd.A = A; hd.eval_mode = eval_mode; hd.lmin = c.log_std_min; hd.ldif = c.log_std_dif;
    hd.seed = seed; hd.call = h->call++;  // exactly one per call
    auto at = [](float *p, size_t off) { return p ? p + off : nullptr; };
    auto cat = [](const float *p, size_t off) { return p ? p + off : nullptr; };
    const PolRoute r = pol_route(n, in0, M, A, maxw, P.mode);
    if (r.kind == POL_ROW) {
        rp.z = z; rp.task_emb = emb;
        rp.L = L; rp.T = T; rp.maxw = maxw; rp.simnorm_dim = c.simnorm_dim;
        for (int l = 0; l < 3; ++l) rp.pi[l] = PolLayerDev{P.wt[l], P.bias[l], l < 2 ? P.g[l] : nullptr, l < 2 ? P.b[l] : nullptr,
                                                            l == 0 ? in0 : M, l == 2 ? 2 * A : M};
        hd.row0 = 0; hd.mask = mask; hd.eps = eps;
        hd.action = out->action; hd.mean = out->mean; hd.log_std = out->log_std; hd.entropy = out->entropy;
        hd.scaled_entropy = out->scaled_entropy; hd.eps_out = out->eps_out;
        rp.head = hd;
        return tdk::pol_launch_row(rp, r.g[0], st);
    }
    for (int r0 = 0; r0 < n; r0 += c.max_envs) {  // the spread route: chunks of at most max_envs rows (the workspace)
        const int m = std::min(c.max_envs, n - r0);
        const PolRoute rc_ = pol_route(m, in0, M, A, maxw, POL_FORCE_SPREAD);
        const size_t ra = (size_t)r0 * A;
        for (int l = 0; l < 3; ++l) {
            PolGemvParams g{};
            g.wt = P.wt[l]; g.bias = P.bias[l]; g.in = l == 0 ? in0 : M; g.out = l == 2 ? 2 * A : M; g.n = m; g.y = P.y;
            if (l == 0) { g.z = z + (size_t)r0 * L; g.emb = cat(emb, (size_t)r0 * T); g.L = L; g.T = T; }
            else { g.x = P.x; g.ldx = M; }
            if ((rc = tdk::pol_launch_gemv(g, rc_.g[2 * l], st))) return rc;
            if (l == 2) break;
            EncNormArgs nm{};
            nm.y = P.y; nm.g = P.g[l]; nm.b = P.b[l]; nm.out = P.x; nm.width = M; nm.last = 0; nm.simnorm_dim = c.simnorm_dim;
            const PolGrid &ng = rc_.g[2 * l + 1];
            enc_launch_norm(nm, ng.x, ng.threads, st);
            HIP_TRY(hipGetLastError());
        }
        PolHeadParams hp{};
        hp.y = P.y;
        hp.head = hd;
        hp.head.row0 = r0; hp.head.mask = cat(mask, ra); hp.head.eps = cat(eps, ra);
        hp.head.action = at(out->action, ra); hp.head.mean = at(out->mean, ra); hp.head.log_std = at(out->log_std, ra);
        hp.head.entropy = at(out->entropy, r0); hp.head.scaled_entropy = at(out->scaled_entropy, r0); hp.head.eps_out = at(out->eps_out, ra);
        if ((rc = tdk::pol_launch_head(hp, rc_.g[5], st))) return rc;
    }
    return 0;
}

// ---- pixel encoder, batch route
int check_pixb_handle(tdmpc2_plan *h) {
    if (h->cfg.multitask) return fail(TDMPC2_ERR_UNSUPPORTED, "the pixel encoder is single-task only (multitask handle)");
    for (int l = 0; l < PIX_LAYERS; ++l)
        if (!h->pix.bound[l]) return fail(TDMPC2_ERR_STATE, "no pixel encoder bound (layer %d; tdmpc2_plan_bind_pixel_encoder)", l);
    return 0;
}
}  // namespace

extern "C" {

int tdmpc2_plan_encode(tdmpc2_plan_t *h, int n_envs, const float *obs, int obs_dim, const float *task_emb, float *z_out,
                       void *stream) {
    if (!h || !obs || !z_out) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n_envs < 1) return fail(TDMPC2_ERR_INVALID, "n_envs %d < 1", n_envs);
    ENTER_ON(h, stream);
    return launch_encode(h, n_envs, obs, obs_dim, task_emb, z_out, (hipStream_t)stream);
}

int tdmpc2_plan_run_obs(tdmpc2_plan_t *h, int n_envs, const float *obs, int obs_dim, const float *task_emb,
                        const float *act_mask, const float *discount_pow, float *prev_mean, const uint8_t *t0, int eval_mode,
                        const tdmpc2_noise *tape, uint64_t seed, float *action, void *stream) {
    if (!h || !obs) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n_envs < 1 || n_envs > h->cfg.max_envs) return fail(TDMPC2_ERR_INVALID, "n_envs %d outside [1, %d]", n_envs, h->cfg.max_envs);
    ENTER_ON(h, stream);
    int rc = launch_encode(h, n_envs, obs, obs_dim, task_emb, h->zenc, (hipStream_t)stream);
    if (rc) return rc;
    return run_impl(h, n_envs, h->zenc, task_emb, act_mask, discount_pow, prev_mean, t0, eval_mode, tape, seed, action, nullptr,
                    stream);
}

int tdmpc2_plan_encode_pix(tdmpc2_plan_t *h, int n_envs, const void *obs, int obs_dtype, int in_channels, const int32_t *shift,
                           float *z_out, void *stream) {
    if (!h || !obs || !shift || !z_out) return fail(TDMPC2_ERR_INVALID, "null argument");
    int rc = check_pix_call(h, n_envs, obs_dtype, in_channels);
    if (rc) return rc;
    ENTER_ON(h, stream);
    return launch_encode_pix(h, n_envs, obs, obs_dtype, shift, z_out, (hipStream_t)stream);
}

int tdmpc2_plan_run_pix(tdmpc2_plan_t *h, int n_envs, const void *obs, int obs_dtype, int in_channels, const int32_t *shift,
                        const float *disc_pow, float *prev_mean, const uint8_t *t0, int eval_mode, const tdmpc2_noise *tape, uint64_t seed,
                        float *action, void *stream) {
    if (!h || !obs || !shift || !disc_pow || !prev_mean || !t0 || !action) return fail(TDMPC2_ERR_INVALID, "null argument");
    int rc = check_pix_call(h, n_envs, obs_dtype, in_channels);
    if (rc) return rc;
    ENTER_ON(h, stream);
    if ((rc = launch_encode_pix(h, n_envs, obs, obs_dtype, shift, h->zenc, (hipStream_t)stream))) return rc;
    return run_impl(h, n_envs, h->zenc, nullptr, nullptr, disc_pow, prev_mean, t0, eval_mode, tape, seed, action, nullptr, stream);
}

int tdmpc2_plan_pi(tdmpc2_plan_t *h, int n_rows, const float *z, const float *task_emb, const float *act_mask, const float *eps,
                   uint64_t seed, const tdmpc2_policy_out *out, void *stream) {
    if (!h || !z) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n_rows < 1) return fail(TDMPC2_ERR_INVALID, "n_rows %d < 1", n_rows);
    int rc = check_pol_call(h, task_emb, act_mask, out);
    if (rc) return rc;
    ENTER_ON(h, stream);
    return launch_pi(h, n_rows, z, nullptr, 0, task_emb, act_mask, eps, seed, 0, out, (hipStream_t)stream);
}

int tdmpc2_plan_act_pi(tdmpc2_plan_t *h, int n_envs, const float *obs, int obs_dim, const float *task_emb, const float *act_mask,
                       const float *eps, int eval_mode, uint64_t seed, const tdmpc2_policy_out *out, void *stream) {
    if (!h || !obs) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n_envs < 1 || n_envs > h->cfg.max_envs) return fail(TDMPC2_ERR_INVALID, "n_envs %d outside [1, %d]", n_envs, h->cfg.max_envs);
    int rc = check_pol_call(h, task_emb, act_mask, out);
    if (rc) return rc;
    ENTER_ON(h, stream);
    return launch_pi(h, n_envs, nullptr, obs, obs_dim, task_emb, act_mask, eps, seed, eval_mode, out, (hipStream_t)stream);
}

int tdmpc2_plan_act_pi_pix(tdmpc2_plan_t *h, int n_envs, const void *obs, int obs_dtype, int in_channels, const int32_t *shift,
                           const float *eps, int eval_mode, uint64_t seed, const tdmpc2_policy_out *out, void *stream) {
    if (!h || !obs || !shift) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (h->cfg.multitask) return fail(TDMPC2_ERR_UNSUPPORTED, "the pixel encoder is single-task only (multitask handle)");
    int rc = check_pix_call(h, n_envs, obs_dtype, in_channels);
    if (rc) return rc;
    if ((rc = check_pol_call(h, nullptr, nullptr, out))) return rc;
    ENTER_ON(h, stream);
    if ((rc = launch_encode_pix(h, n_envs, obs, obs_dtype, shift, h->zenc, (hipStream_t)stream))) return rc;
    return launch_pi(h, n_envs, h->zenc, nullptr, 0, nullptr, nullptr, eps, seed, eval_mode, out, (hipStream_t)stream);
}

// ================================================================ pixel encoder, batch route (k_pixel_batch.hip, pixel_batch_route.h)
// Training batches of frame stacks: any number of images, in passes over a workspace that tdmpc2_plan_pix_batch_reserve sized.
// The weights, biases and ShiftAug table are the ones tdmpc2_plan_bind_pixel_encoder keeps for the planning routes.
int tdmpc2_plan_pix_batch_reserve(tdmpc2_plan_t *h, int chunk_images, void *stream) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    if (chunk_images < 1) return fail(TDMPC2_ERR_INVALID, "chunk_images %d < 1", chunk_images);
    int rc = check_pixb_handle(h);
    if (rc) return rc;
    ENTER_ON(h, stream);
    tdmpc2_plan::Pix &P = h->pix;
    if (chunk_images <= P.bchunk) return TDMPC2_OK;  // grows, never shrinks
    if (!P.bchunk && (rc = tdk::pixb_set_lds(pixb_lds(0, PIX_MAX_C, PIX_MAX_CIN)))) return rc;
    if ((rc = grow_ws(h, &P.bws, &P.bws_cap, (size_t)chunk_images * pix_ws_floats(P.C), (hipStream_t)stream))) return rc;
    P.bchunk = chunk_images;
    return TDMPC2_OK;
}

int tdmpc2_plan_encode_pix_batch(tdmpc2_plan_t *h, int n_images, const void *obs, int obs_dtype, int in_channels,
                                 const int32_t *shift, float *z_out, void *stream) {
    if (!h || !obs || !shift || !z_out) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n_images < 1) return fail(TDMPC2_ERR_INVALID, "n_images %d < 1", n_images);
    if (obs_dtype != 0 && obs_dtype != 1) return fail(TDMPC2_ERR_INVALID, "obs_dtype %d (0 = uint8, 1 = float32)", obs_dtype);
    if (in_channels < 1 || in_channels > PIX_MAX_CIN)
        return fail(TDMPC2_ERR_INVALID, "pixel encoder: %d input channels outside [1, %d]", in_channels, PIX_MAX_CIN);
    int rc = check_pixb_handle(h);
    if (rc) return rc;
    const tdmpc2_plan::Pix &P = h->pix;
    if (in_channels != P.cin)
        return fail(TDMPC2_ERR_INVALID, "pixel encoder: the observation has %d channels, layer 0 was bound with %d", in_channels, P.cin);
    if (!P.bchunk) return fail(TDMPC2_ERR_STATE, "no batch workspace reserved (tdmpc2_plan_pix_batch_reserve)");
    ENTER_ON(h, stream);
    PixbParams p{};
    for (int l = 0; l < PIX_LAYERS; ++l) { p.wp[l] = P.wp[l]; p.bias[l] = P.bias[l]; }
    p.cin = P.cin; p.C = P.C; p.tab = static_cast<const PixTap *>(P.tab); p.ws = P.bws;
    const size_t img_bytes = (size_t)P.cin * PIX_IN * PIX_IN * (obs_dtype == 0 ? 1 : 4);
    for (int i = 0; i < pixb_chunks(n_images, P.bchunk); ++i) {
        const int e0 = pixb_chunk_begin(i, P.bchunk);
        p.n = pixb_chunk_count(n_images, P.bchunk, i);
        p.obs = static_cast<const char *>(obs) + (size_t)e0 * img_bytes;
        p.shift = shift + 2 * (size_t)e0;
        p.z = z_out + (size_t)e0 * 16 * P.C;
        for (int l = 0; l < PIX_LAYERS; ++l)
            if ((rc = tdk::pixb_launch(l, obs_dtype == 0, p, pixb_grid(l, p.n, P.C, P.cin), (hipStream_t)stream))) return rc;
    }
    return TDMPC2_OK;
}

}  // extern "C"
