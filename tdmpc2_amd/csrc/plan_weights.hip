// Host unit of the planner's weights: how checkpoint tensors reach the handle.  Reference: the networks WorldModel.__init__
// builds (tdmpc2/common/world_model.py:17-36, layers.mlp / layers.enc: tdmpc2/common/layers.py:121-164), TDMPC2.load
// (tdmpc2/tdmpc2.py:81-95) and WorldModel.soft_update_target_Q (world_model.py:82-86).
//
// This unit: the stored shape of every layer and its first-time allocation, the weight packer's job tables and run_jobs
// (kernels: k_refresh.hip; launch list: refresh_route.h), every bind (tdmpc2_plan_bind_weights / bind_encoder /
// bind_pixel_encoder / bind_policy), tdmpc2_plan_refresh_weights, tdmpc2_plan_soft_update_target, and the packed blob
// (tdmpc2_plan_packed_size / export_packed / import_packed).  Shared services: plan_host.h.
#include <cstring>

#include "plan_host.h"

namespace {
// Shape of one nn.Linear of the world model as the planner stores it (tdmpc2/common/world_model.py:26-30).
struct LayerShape {
    int in, out;      // nn.Linear in_features / out_features
    int nz, nt, na;   // source columns: latent or hidden | task embedding | action
    int KB, CT;
    bool has_ln, mish;  // LayerNorm after the Linear; Mish (hidden layers) as opposed to SimNorm / none
    int heads;
    size_t wsz /* floats' worth of packed weights per head */, bsz, gsz, esz;
};
LayerShape layer_shape(const tdmpc2_plan *h, int net, int layer) {
    const tdmpc2_plan_cfg &c = h->cfg;
    LayerShape s{};
    const bool is_q = net == TDMPC2_NET_Q || net == TDMPC2_NET_TARGET_Q;
    const bool takes_action = (net == TDMPC2_NET_DYNAMICS || net == TDMPC2_NET_REWARD || is_q);
    s.heads = is_q ? c.num_q : 1;
    if (layer == 0) {
        s.in = c.latent_dim + c.task_dim + (takes_action ? c.action_dim : 0);
        s.out = c.mlp_dim;
    } else if (layer == 1) {
        s.in = c.mlp_dim;
        s.out = c.mlp_dim;
    } else {
        s.in = c.mlp_dim;
        s.out = net == TDMPC2_NET_DYNAMICS ? c.latent_dim : net == TDMPC2_NET_PI ? 2 * c.action_dim
                : net == TDMPC2_NET_TERMINATION ? 1 : (c.num_bins > 1 ? c.num_bins : 1);
    }
    s.has_ln = (layer < 2) || net == TDMPC2_NET_DYNAMICS;
    s.mish = layer < 2;
    s.nz = (layer == 0) ? c.latent_dim : c.mlp_dim;
    s.nt = (layer == 0) ? c.task_dim : 0;
    s.na = (layer == 0 && takes_action) ? c.action_dim : 0;
    // packed contraction length: the fused kernels pad the action columns to 16, the layered GEMMs the whole row to GBK
    const int Kp = h->lay.on ? (int)round_up((size_t)s.nz + s.na, GBK) : s.nz + (s.na + 15) / 16 * 16;
    s.KB = h->split ? Kp / 16 : Kp / 8;
    s.CT = (s.out + 31) / 32;
    s.wsz = h->split ? (size_t)s.CT * s.KB * 512 /* floats' worth of 1024 halfs */ : (size_t)s.CT * s.KB * 256;
    s.bsz = (size_t)s.CT * 32;
    s.gsz = round_up((size_t)s.out, 4);
    s.esz = (size_t)s.out * (s.nt > 0 ? s.nt : 0);
    return s;
}

// One slab per tensor kind holding all ensemble members at a constant stride (the layered GEMM selects a member per plan
// by stride); allocated on the first bind (or import) of a (net, layer).
int ensure_layer_alloc(tdmpc2_plan *h, int net, int layer, const LayerShape &sh) {
    HostLayer &L0 = net_of(h, net, 0)->l[layer];
    if (L0.alloc) return 0;
    int rc;
    if (h->split && !net_of(h, net, 0)->scal) {  // the net's [heads][3] scalar table, defaults: scales 2^5, kw 0
        LayerScal *tab = nullptr;
        if ((rc = dev_alloc(h, (void **)&tab, (size_t)sh.heads * 3 * sizeof(LayerScal)))) return rc;
        std::vector<LayerScal> init((size_t)sh.heads * 3, LayerScal{1.f, 1.f / ACT_SCALE, 0u, 0, ACT_SCALE, ACT_SCALE_LOG2, 0u, 0u});
        HIP_TRY(hipMemcpy(tab, init.data(), init.size() * sizeof(LayerScal), hipMemcpyHostToDevice));
        for (int hd = 0; hd < sh.heads; ++hd) net_of(h, net, hd)->scal = tab + (size_t)hd * 3;
    }
    float *wslab = nullptr, *bslab = nullptr, *gslab = nullptr, *betaslab = nullptr, *eslab = nullptr;
    if ((rc = dev_alloc(h, (void **)&wslab, sh.heads * sh.wsz * 4))) return rc;
    if ((rc = dev_alloc(h, (void **)&bslab, sh.heads * sh.bsz * 4))) return rc;
    if (sh.has_ln) {
        if ((rc = dev_alloc(h, (void **)&gslab, sh.heads * sh.gsz * 4))) return rc;
        if ((rc = dev_alloc(h, (void **)&betaslab, sh.heads * sh.gsz * 4))) return rc;
    }
    if (sh.nt > 0 && (rc = dev_alloc(h, (void **)&eslab, sh.heads * sh.esz * 4))) return rc;
    for (int hd = 0; hd < sh.heads; ++hd) {
        HostNet *N = net_of(h, net, hd);
        HostLayer &L = N->l[layer];
        L.alloc = true;
        L.KB = sh.KB; L.CT = sh.CT; L.out = sh.out;
        L.wbytes = sh.wsz * 4;
        if (h->split) {
            L.wps = reinterpret_cast<_Float16 *>(wslab + hd * sh.wsz);
            L.scal = N->scal + layer;
            L.oscale = &L.scal->oscale;
            L.ascale = &L.scal->ascale;
        } else {
            L.wp = wslab + hd * sh.wsz;
            L.oscale = h->one;  // the exact arithmetic has no scales
            L.ascale = h->one;
        }
        L.bias = bslab + hd * sh.bsz;
        L.g = sh.has_ln ? gslab + hd * sh.gsz : nullptr;
        L.b = sh.has_ln ? betaslab + hd * sh.gsz : nullptr;
        L.wemb = sh.nt > 0 ? eslab + hd * sh.esz : nullptr;
    }
    return 0;
}

int ensure_enc_alloc(tdmpc2_plan *h, int layer, int in_features, int out_features) {
    const tdmpc2_plan_cfg &c = h->cfg;
    tdmpc2_plan::Enc &L = h->enc[layer];
    if (in_features > ENC_MAX_IN)  // binds and packed blobs both come through here, before anything is allocated or enqueued
        return fail(TDMPC2_ERR_UNSUPPORTED, "encoder layer %d: %d inputs, at most %d (a layer's input row is held in %zu bytes of LDS)",
                    layer, in_features, ENC_MAX_IN, ENC_GEMV_LDS_MAX);
    if (L.wt && (L.in != in_features || L.out != out_features))
        return fail(TDMPC2_ERR_STATE, "encoder layer %d re-bound with a different shape", layer);
    int rc;
    if (!L.wt) {
        if ((rc = dev_alloc(h, (void **)&L.wt, (size_t)in_features * out_features * 4))) return rc;
        if ((rc = dev_alloc(h, (void **)&L.bias, (size_t)out_features * 4))) return rc;
        if ((rc = dev_alloc(h, (void **)&L.g, (size_t)out_features * 4))) return rc;
        if ((rc = dev_alloc(h, (void **)&L.b, (size_t)out_features * 4))) return rc;
        L.in = in_features;
        L.out = out_features;
    }
    if (!h->zenc && (rc = dev_alloc(h, (void **)&h->zenc, (size_t)c.max_envs * c.latent_dim * 4))) return rc;
    const int w = std::max(in_features, out_features);
    if (w > ENC_WIDE && w > h->enc_ws_width) {  // workspace of the layer-at-a-time encoder path (grows with the widest layer)
        if ((rc = dev_alloc(h, (void **)&h->enc_y, (size_t)c.max_envs * w * 4))) return rc;
        if ((rc = dev_alloc(h, (void **)&h->enc_x, (size_t)c.max_envs * w * 4))) return rc;
        h->enc_ws_width = w;
    }
    return 0;
}

// ================================================================ the weight packer's host side (k_refresh.hip: refresh_kernels.cuh, refresh_route.h)
// Every entry point that stores weights describes JOBS -- one per (net, layer) with every ensemble member inside it, one per
// transposed copy (a state-encoder layer, a layer of the policy prior's fp32 copy) -- and hands them to run_jobs.  The entry
// points differ only in how they collect jobs: the per-layer binds describe one, the table calls walk their table.  Each kind
// of job has ONE function that checks it, allocates its first-time storage and appends it; everything that can refuse,
// refuses before anything is enqueued.
struct RfJobs {
    RfParams p{};
    unsigned nets = 0;          // nets with a named layer
    unsigned enc = 0, pol = 0;  // state-encoder / policy-copy layers among p.tr
    int nenc = 0;               // the encoder depth its layers were checked against
    explicit RfJobs(const tdmpc2_plan *h) {
        p.split = h->split ? 1 : 0;
        p.lerp_net = -1;
    }
};

// one nn.Linear of a net (+ its LayerNorm), every ensemble member: `e` in the checkpoint's layout, stacked over heads
int add_net_layer(tdmpc2_plan *h, RfJobs &j, int net, int l, const tdmpc2_weight_entry &e) {
    if (net == TDMPC2_NET_TERMINATION && !h->cfg.episodic)
        return fail(TDMPC2_ERR_INVALID, "termination head bound on a non-episodic planner");
    const LayerShape sh = layer_shape(h, net, l);
    if (!e.W || !e.b) return fail(TDMPC2_ERR_INVALID, "net %d is named but layer %d lacks its weight or bias", net, l);
    if (sh.has_ln && (!e.ln_g || !e.ln_b)) return fail(TDMPC2_ERR_INVALID, "net %d layer %d needs LayerNorm parameters", net, l);
    if (int rc = ensure_layer_alloc(h, net, l, sh)) return rc;
    const HostLayer &L0 = net_of(h, net, 0)->l[l];
    RfNet &N = j.p.net[net];
    RfLayer &J = N.l[l];
    J.W = e.W; J.b = e.b; J.g = sh.has_ln ? e.ln_g : nullptr; J.beta = sh.has_ln ? e.ln_b : nullptr;
    J.wdst = h->split ? reinterpret_cast<float *>(L0.wps) : L0.wp;
    J.bias = L0.bias; J.gd = L0.g; J.bd = L0.b; J.wemb = L0.wemb;
    J.out = sh.out; J.in = sh.in; J.nz = sh.nz; J.nt = sh.nt; J.na = sh.na; J.CT = sh.CT; J.KB = sh.KB;
    J.has_ln = sh.has_ln ? 1 : 0; J.mish = sh.mish ? 1 : 0;
    J.scan_nbw = rf_scan_wblocks((long)sh.out * sh.in);
    N.heads = sh.heads;
    N.scal = h->split ? net_of(h, net, 0)->scal : nullptr;
    N.mask |= 1 << l;
    j.nets |= 1u << net;
    return 0;
}

// layer `l` of a state encoder of `nenc` layers
int add_enc_layer(tdmpc2_plan *h, RfJobs &j, int l, int nenc, const tdmpc2_weight_entry &e, int out_features, int in_features) {
    const tdmpc2_plan_cfg &c = h->cfg;
    if (nenc < 1 || nenc > ENC_MAX_LAYERS) return fail(TDMPC2_ERR_INVALID, "encoder depth %d outside [1, %d]", nenc, ENC_MAX_LAYERS);
    if (l < 0 || l >= nenc) return fail(TDMPC2_ERR_INVALID, "encoder layer %d outside [0, %d)", l, nenc);
    if (!e.W || !e.b || !e.ln_g || !e.ln_b) return fail(TDMPC2_ERR_INVALID, "encoder layer %d: null tensor", l);
    if (out_features < 1 || out_features > ENC_THREADS * ENC_MAX_PER_THREAD || in_features < 1)
        return fail(TDMPC2_ERR_UNSUPPORTED, "encoder layer %d: width %d outside [1, %d]", l, out_features, ENC_THREADS * ENC_MAX_PER_THREAD);
    if (l == nenc - 1 && out_features != c.latent_dim)
        return fail(TDMPC2_ERR_INVALID, "the last encoder layer has %d outputs, latent_dim is %d", out_features, c.latent_dim);
    if (l == nenc - 1 && (c.latent_dim % c.simnorm_dim || (c.simnorm_dim & (c.simnorm_dim - 1)) || c.simnorm_dim > 64))
        return fail(TDMPC2_ERR_UNSUPPORTED, "SimNorm groups of %d over %d latents", c.simnorm_dim, c.latent_dim);
    if (h->enc_layers && h->enc_layers != nenc) return fail(TDMPC2_ERR_STATE, "encoder depth changed from %d to %d", h->enc_layers, nenc);
    if (int rc = ensure_enc_alloc(h, l, in_features, out_features)) return rc;  // refuses a re-bind with another shape
    const tdmpc2_plan::Enc &E = h->enc[l];
    j.p.tr[j.p.ntrans++] = RfTrans{e.W, e.b, e.ln_g, e.ln_b, E.wt, E.bias, E.g, E.b, E.out, E.in};
    j.enc |= 1u << l;
    j.nenc = nenc;
    return 0;
}

// layer `l` of the policy prior's fp32 copy; its buffers exist (tdmpc2_plan_bind_policy) and `e` has passed that call's checks
// or add_net_layer(TDMPC2_NET_PI)'s, which ask the same of it
void add_pol_layer(tdmpc2_plan *h, RfJobs &j, int l, const tdmpc2_weight_entry &e) {
    const bool ln = l < 2;
    const tdmpc2_plan_cfg &c = h->cfg;
    const tdmpc2_plan::Pol &P = h->pol;
    j.p.tr[j.p.ntrans++] = RfTrans{e.W, e.b, ln ? e.ln_g : nullptr, ln ? e.ln_b : nullptr, P.wt[l], P.bias[l], ln ? P.g[l] : nullptr,
                                   ln ? P.b[l] : nullptr, l == 2 ? 2 * c.action_dim : c.mlp_dim, l == 0 ? c.latent_dim + c.task_dim : c.mlp_dim};
    j.pol |= 1u << l;
}

// The launches refresh_route lists over the jobs' workgroup ranges, then the bound flags of exactly the jobs that ran.
int run_jobs(tdmpc2_plan *h, RfJobs &j, hipStream_t st) {
    RfParams &p = j.p;
    const bool pi = j.nets >> TDMPC2_NET_PI & 1;
    const RefreshRoute route = refresh_route(RefreshIn{p.split, j.nets, __builtin_popcount(j.enc), j.pol && pi, p.lerp_net >= 0,
                                                       h->cfg.num_q, h->cfg.episodic, j.pol && !pi});
    long sb = 0, pb = 0;
    for (int net = 0; net < RF_NETS; ++net)
        for (int l = 0; l < 3; ++l) {
            const RfNet &N = p.net[net];
            const RfLayer &J = N.l[l];
            p.scan_blk0[net * 3 + l] = (int)sb;
            p.pack_blk0[net * 3 + l] = (int)pb;
            if (!(N.mask >> l & 1)) continue;
            sb += (long)N.heads * (J.scan_nbw + 1);
            pb += (long)N.heads * rf_pack_blocks(J.CT, J.KB * (p.split ? 16 : 8), J.nt);
        }
    p.scan_blk0[3 * RF_NETS] = (int)sb;
    for (int t = 0; t < RF_MAX_TRANS; ++t) {
        p.pack_blk0[3 * RF_NETS + t] = (int)pb;
        if (t < p.ntrans) pb += rf_transpose_blocks(p.tr[t].out, p.tr[t].in);
    }
    p.pack_blk0[RF_SEGS] = (int)pb;
    if (pb > 0x7fffffffL || sb > 0x7fffffffL) return fail(TDMPC2_ERR_UNSUPPORTED, "weight refresh: %ld workgroups", pb);
    for (int i = 0; i < route.nops; ++i)
        if (int rc = tdk::refresh_launch(route.op[i], p, st)) return rc;
    for (int net = 0; net < RF_NETS; ++net)
        for (int l = 0; l < 3; ++l)
            if (p.net[net].mask >> l & 1)
                for (int hd = 0; hd < p.net[net].heads; ++hd) net_of(h, net, hd)->l[l].bound = true;
    for (int l = 0; l < ENC_MAX_LAYERS; ++l)
        if (j.enc >> l & 1) h->enc[l].bound = true;
    if (j.enc) h->enc_layers = j.nenc;
    for (int l = 0; l < 3; ++l)
        if (j.pol >> l & 1) h->pol.bound[l] = true;
    return TDMPC2_OK;
}
}  // namespace

extern "C" {

int tdmpc2_plan_bind_weights(tdmpc2_plan_t *h, int net, int layer, const float *W, const float *b, const float *ln_g,
                             const float *ln_b, int out_features, int in_features, void *stream) {
    if (!h || !W || !b) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (layer < 0 || layer > 2) return fail(TDMPC2_ERR_INVALID, "layer %d outside [0, 2]", layer);
    if (net < TDMPC2_NET_DYNAMICS || net > TDMPC2_NET_TARGET_Q) return fail(TDMPC2_ERR_INVALID, "unknown net %d", net);
    ENTER_ON(h, stream);
    const LayerShape sh = layer_shape(h, net, layer);  // the caller states the shape: it must be the handle's
    if (in_features != sh.in || out_features != sh.out)
        return fail(TDMPC2_ERR_INVALID, "net %d layer %d: got [%d, %d], expected [%d, %d]", net, layer, out_features,
                    in_features, sh.out, sh.in);
    RfJobs j(h);
    if (int rc = add_net_layer(h, j, net, layer, tdmpc2_weight_entry{W, b, ln_g, ln_b})) return rc;
    return run_jobs(h, j, (hipStream_t)stream);
}

int tdmpc2_plan_bind_encoder(tdmpc2_plan_t *h, int layer, int n_layers, const float *W, const float *b, const float *ln_g,
                             const float *ln_b, int out_features, int in_features, void *stream) {
    if (!h || !W || !b || !ln_g || !ln_b) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    RfJobs j(h);
    if (int rc = add_enc_layer(h, j, layer, n_layers, tdmpc2_weight_entry{W, b, ln_g, ln_b}, out_features, in_features)) return rc;
    return run_jobs(h, j, (hipStream_t)stream);
}

// ================================================================ pixel-observation encoder (k_plan.hip: pixel_kernels.cuh, pixel_route.h)
int tdmpc2_plan_bind_pixel_encoder(tdmpc2_plan_t *h, int layer, const float *W, const float *b, int out_channels, int in_channels,
                                   int kernel, void *stream) {
    if (!h || !W || !b) return fail(TDMPC2_ERR_INVALID, "null argument");
    const tdmpc2_plan_cfg &c = h->cfg;
    if (c.multitask)  // the reference cannot concatenate task_emb onto an image either (world_model.py:88-112)
        return fail(TDMPC2_ERR_UNSUPPORTED, "the pixel encoder is single-task only (multitask handle)");
    if (layer < 0 || layer >= PIX_LAYERS) return fail(TDMPC2_ERR_INVALID, "pixel encoder layer %d outside [0, %d)", layer, PIX_LAYERS);
    if (kernel != pix_kernel(layer))
        return fail(TDMPC2_ERR_INVALID, "pixel encoder layer %d has a %dx%d kernel, not %dx%d", layer, pix_kernel(layer), pix_kernel(layer),
                    kernel, kernel);
    if (out_channels < PIX_MIN_C || out_channels > PIX_MAX_C || out_channels % 8)
        return fail(TDMPC2_ERR_UNSUPPORTED, "pixel encoder: %d channels (a multiple of 8 in [%d, %d])", out_channels, PIX_MIN_C, PIX_MAX_C);
    if (16 * out_channels != c.latent_dim)
        return fail(TDMPC2_ERR_INVALID, "pixel encoder: 16 x %d channels is not latent_dim %d", out_channels, c.latent_dim);
    if (c.simnorm_dim != 8) return fail(TDMPC2_ERR_UNSUPPORTED, "pixel encoder: SimNorm groups of %d (8 only)", c.simnorm_dim);
    if (layer == 0 && (in_channels < 1 || in_channels > PIX_MAX_CIN))
        return fail(TDMPC2_ERR_INVALID, "pixel encoder: %d input channels outside [1, %d]", in_channels, PIX_MAX_CIN);
    if (layer > 0 && in_channels != out_channels)
        return fail(TDMPC2_ERR_INVALID, "pixel encoder layer %d takes %d channels, not %d", layer, out_channels, in_channels);
    ENTER_ON(h, stream);
    tdmpc2_plan::Pix &P = h->pix;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (!P.tab) {  // every buffer of the encoder, once: encode / run never allocate
        static PixTap host_tab[PIX_SHIFTS * PIX_IN];
        static std::once_flag once;
        std::call_once(once, [] { pix_shift_table(host_tab); });
        for (int l = 0; l < PIX_LAYERS; ++l) {
            const int cin = l == 0 ? PIX_MAX_CIN : out_channels;
            if ((rc = dev_alloc(h, (void **)&P.wp[l], (size_t)cin * pix_kernel(l) * pix_kernel(l) * out_channels * 4))) return rc;
            if ((rc = dev_alloc(h, (void **)&P.bias[l], (size_t)out_channels * 4))) return rc;
        }
        if ((rc = dev_alloc(h, &P.tab, sizeof(host_tab)))) return rc;
        if ((rc = dev_alloc(h, (void **)&P.ws, pix_ws_bytes(c.max_envs, out_channels)))) return rc;
        if (!h->zenc && (rc = dev_alloc(h, (void **)&h->zenc, (size_t)c.max_envs * c.latent_dim * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(P.tab, host_tab, sizeof(host_tab), hipMemcpyHostToDevice, st));
        P.C = out_channels;
    }
    const int kk = kernel * kernel;
    const int n = out_channels * in_channels * kk;
    pix_launch_pack(W, P.wp[layer], out_channels, in_channels, kk, (n + 255) / 256, 256, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(P.bias[layer], b, (size_t)out_channels * 4, hipMemcpyDeviceToDevice, st));
    if (layer == 0) P.cin = in_channels;
    P.bound[layer] = true;
    return TDMPC2_OK;
}

// ================================================================ policy prior (k_policy.hip: policy_kernels.cuh, policy_route.h)
int tdmpc2_plan_bind_policy(tdmpc2_plan_t *h, int layer, const float *W, const float *b, const float *ln_g, const float *ln_b,
                            int out_features, int in_features, void *stream) {
    if (!h || !W || !b) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (layer < 0 || layer > 2) return fail(TDMPC2_ERR_INVALID, "policy layer %d outside [0, 2]", layer);
    const tdmpc2_plan_cfg &c = h->cfg;
    const int in0 = c.latent_dim + c.task_dim, M = c.mlp_dim, A = c.action_dim;
    const int want_in = layer == 0 ? in0 : M, want_out = layer == 2 ? 2 * A : M;
    if (in_features != want_in || out_features != want_out)
        return fail(TDMPC2_ERR_INVALID, "policy layer %d: got [%d, %d], expected [%d, %d] (latent_dim + task_dim -> mlp_dim -> 2 action_dim)",
                    layer, out_features, in_features, want_out, want_in);
    if (layer < 2 && (!ln_g || !ln_b)) return fail(TDMPC2_ERR_INVALID, "policy layer %d needs its LayerNorm parameters", layer);
    if (M > POL_MAX_WIDTH || in0 > POL_MAX_WIDTH)
        return fail(TDMPC2_ERR_UNSUPPORTED, "policy prior: widths %d / %d beyond %d", in0, M, POL_MAX_WIDTH);
    ENTER_ON(h, stream);
    tdmpc2_plan::Pol &P = h->pol;
    int rc;
    if (!P.x) {  // every buffer of the policy prior, once: pi / act_pi never allocate
        for (int l = 0; l < 3; ++l) {
            const int li = l == 0 ? in0 : M, lo = l == 2 ? 2 * A : M;
            if ((rc = dev_alloc(h, (void **)&P.wt[l], (size_t)li * lo * 4))) return rc;
            if ((rc = dev_alloc(h, (void **)&P.bias[l], (size_t)lo * 4))) return rc;
            if (l < 2 && (rc = dev_alloc(h, (void **)&P.g[l], (size_t)lo * 4))) return rc;
            if (l < 2 && (rc = dev_alloc(h, (void **)&P.b[l], (size_t)lo * 4))) return rc;
        }
        if ((rc = dev_alloc(h, (void **)&P.y, pol_ws_y_floats(c.max_envs, M, A) * 4))) return rc;
        if (!h->zenc && (rc = dev_alloc(h, (void **)&h->zenc, (size_t)c.max_envs * c.latent_dim * 4))) return rc;
        if ((rc = tdk::pol_set_lds())) return rc;
        if ((rc = dev_alloc(h, (void **)&P.x, pol_ws_x_floats(c.max_envs, M) * 4))) return rc;  // last: marks the set complete
    }
    RfJobs j(h);
    add_pol_layer(h, j, layer, tdmpc2_weight_entry{W, b, ln_g, ln_b});
    return run_jobs(h, j, (hipStream_t)stream);
}

// ================================================================ weight tables: the packer's jobs, collected from a table
// Every net the table names (all three layers of it), the state encoder, and the policy prior's fp32 copy when its buffers
// exist and TDMPC2_NET_PI is named.
int tdmpc2_plan_refresh_weights(tdmpc2_plan_t *h, const tdmpc2_weight_table *tab, void *stream) {
    if (!h || !tab) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    RfJobs j(h);
    for (int net = TDMPC2_NET_DYNAMICS; net <= TDMPC2_NET_TARGET_Q; ++net) {
        int named = 0;
        for (const tdmpc2_weight_entry &e : tab->net[net]) named += (e.W != nullptr) + (e.b != nullptr) + (e.ln_g != nullptr) + (e.ln_b != nullptr);
        if (!named) continue;  // left as it is
        for (int l = 0; l < 3; ++l)
            if (int rc = add_net_layer(h, j, net, l, tab->net[net][l])) return rc;
    }
    if (tab->enc_layers < 0) return fail(TDMPC2_ERR_INVALID, "encoder depth %d outside [0, %d]", tab->enc_layers, ENC_MAX_LAYERS);
    for (int l = 0; l < tab->enc_layers; ++l)
        if (int rc = add_enc_layer(h, j, l, tab->enc_layers, tab->enc[l], tab->enc_out[l], tab->enc_in[l])) return rc;
    if (h->pol.x && (j.nets >> TDMPC2_NET_PI & 1))
        for (int l = 0; l < 3; ++l) add_pol_layer(h, j, l, tab->net[TDMPC2_NET_PI][l]);
    return run_jobs(h, j, (hipStream_t)stream);
}

// The jobs of TDMPC2_NET_TARGET_Q with the caller's target tensors as sources; RO_SCAN lerps them towards the online ensemble
// `online` names before it scans them.
int tdmpc2_plan_soft_update_target(tdmpc2_plan_t *h, const tdmpc2_weight_table *online, float *const target[3][4], float tau,
                                   void *stream) {
    if (!h || !online || !target) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (!(tau >= 0.f && tau <= 1.f)) return fail(TDMPC2_ERR_INVALID, "soft update: tau %g outside [0, 1]", (double)tau);
    ENTER_ON(h, stream);
    RfJobs j(h);
    for (int l = 0; l < 3; ++l) {
        const tdmpc2_weight_entry src{target[l][0], target[l][1], target[l][2], target[l][3]};
        const tdmpc2_weight_entry &on = online->net[TDMPC2_NET_Q][l];
        const bool ln = layer_shape(h, TDMPC2_NET_TARGET_Q, l).has_ln;
        if (!on.W || !on.b || (ln && (!on.ln_g || !on.ln_b)))
            return fail(TDMPC2_ERR_INVALID, "soft update: the table lacks the online Q ensemble (layer %d)", l);
        if (!src.W || !src.b || (ln && (!src.ln_g || !src.ln_b)))
            return fail(TDMPC2_ERR_INVALID, "soft update: null target tensor (layer %d)", l);
        if (int rc = add_net_layer(h, j, TDMPC2_NET_TARGET_Q, l, src)) return rc;
        j.p.online[l][0] = on.W; j.p.online[l][1] = on.b; j.p.online[l][2] = ln ? on.ln_g : nullptr; j.p.online[l][3] = ln ? on.ln_b : nullptr;
    }
    j.p.lerp_net = TDMPC2_NET_TARGET_Q;
    j.p.tau = tau;
    return run_jobs(h, j, (hipStream_t)stream);
}

// ---------------------------------------------------------------- packed weight file
// Everything a bind produces -- fragment-ordered (and, for the split arithmetic, hi/lo-split and scaled) weights, padded
// biases, LayerNorm parameters, task-embedding columns, the per-layer scale records, the transposed encoder -- as one
// host blob: [PackHdr][segment sizes][segment data].  Importing it is a sequence of plain host-to-device copies: no
// packing kernels, no fp32 checkpoint on the device (reference load path: tdmpc2/tdmpc2.py:81-95).
namespace {
struct PackHdr {
    char magic[8];
    uint32_t version, abi;
    tdmpc2_plan_cfg cfg;  // as resolved by create (path and precision are concrete); max_envs / device are not compared
    uint32_t has_target, enc_layers;
    int32_t enc_in[ENC_MAX_LAYERS], enc_out[ENC_MAX_LAYERS];
    uint64_t nseg, data_bytes;
};
struct Seg {
    void *p;
    size_t bytes;
};
const int kPackNets[] = {TDMPC2_NET_DYNAMICS, TDMPC2_NET_REWARD, TDMPC2_NET_PI, TDMPC2_NET_TERMINATION, TDMPC2_NET_Q, TDMPC2_NET_TARGET_Q};

bool net_in_pack(const tdmpc2_plan *h, int net, bool has_target) {
    if (net == TDMPC2_NET_TERMINATION) return h->cfg.episodic != 0;
    if (net == TDMPC2_NET_TARGET_Q) return has_target;
    return true;
}
// canonical walk; every visited layer must be allocated
void collect_segments(tdmpc2_plan *h, bool has_target, int enc_layers, std::vector<Seg> &out) {
    for (int net : kPackNets) {
        if (!net_in_pack(h, net, has_target)) continue;
        const int heads = layer_shape(h, net, 0).heads;
        for (int hd = 0; hd < heads; ++hd) {
            HostNet *N = net_of(h, net, hd);
            for (int l = 0; l < 3; ++l) {
                const LayerShape sh = layer_shape(h, net, l);
                HostLayer &L = N->l[l];
                out.push_back({h->split ? (void *)L.wps : (void *)L.wp, sh.wsz * 4});
                out.push_back({L.bias, sh.bsz * 4});
                if (sh.has_ln) {
                    out.push_back({L.g, sh.gsz * 4});
                    out.push_back({L.b, sh.gsz * 4});
                }
                if (sh.nt > 0) out.push_back({L.wemb, sh.esz * 4});
            }
            if (h->split) out.push_back({N->scal, 3 * sizeof(LayerScal)});
        }
    }
    for (int l = 0; l < enc_layers; ++l) {
        tdmpc2_plan::Enc &E = h->enc[l];
        out.push_back({E.wt, (size_t)E.in * E.out * 4});
        out.push_back({E.bias, (size_t)E.out * 4});
        out.push_back({E.g, (size_t)E.out * 4});
        out.push_back({E.b, (size_t)E.out * 4});
    }
}
bool target_bound(const tdmpc2_plan *h) {
    for (int i = 0; i < 3; ++i)
        for (int q = 0; q < h->cfg.num_q; ++q)
            if (!h->tq[q].l[i].bound) return false;
    return true;
}
bool same_model(const tdmpc2_plan_cfg &a, const tdmpc2_plan_cfg &b) {
    return a.horizon == b.horizon && a.num_samples == b.num_samples && a.action_dim == b.action_dim && a.latent_dim == b.latent_dim &&
           a.mlp_dim == b.mlp_dim && a.task_dim == b.task_dim && a.num_bins == b.num_bins && a.num_q == b.num_q &&
           a.simnorm_dim == b.simnorm_dim && a.multitask == b.multitask && a.episodic == b.episodic && a.path == b.path &&
           a.precision == b.precision;
}
}  // namespace

int tdmpc2_plan_packed_size(tdmpc2_plan_t *h, uint64_t *bytes) {
    if (!h || !bytes) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER(h);
    int rc = check_ready(h);
    if (rc) return rc;
    std::vector<Seg> segs;
    collect_segments(h, target_bound(h), h->enc_layers, segs);
    uint64_t total = sizeof(PackHdr) + segs.size() * sizeof(uint64_t);
    for (const Seg &sg : segs) total += sg.bytes;
    *bytes = total;
    return TDMPC2_OK;
}

int tdmpc2_plan_export_packed(tdmpc2_plan_t *h, void *host_buf, uint64_t bytes, void *stream) {
    if (!h || !host_buf) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    int rc = check_ready(h);
    if (rc) return rc;
    for (int l = 0; l < h->enc_layers; ++l)
        if (!h->enc[l].bound) return fail(TDMPC2_ERR_STATE, "encoder layer %d of %d is not bound", l, h->enc_layers);
    const bool has_target = target_bound(h);
    std::vector<Seg> segs;
    collect_segments(h, has_target, h->enc_layers, segs);
    PackHdr hdr{};
    memcpy(hdr.magic, "TDMPC2PK", 8);
    hdr.version = 1; hdr.abi = TDMPC2_PLAN_ABI_VERSION; hdr.cfg = h->cfg; hdr.has_target = has_target ? 1 : 0;
    hdr.enc_layers = (uint32_t)h->enc_layers;
    for (int l = 0; l < h->enc_layers; ++l) { hdr.enc_in[l] = h->enc[l].in; hdr.enc_out[l] = h->enc[l].out; }
    hdr.nseg = segs.size();
    for (const Seg &sg : segs) hdr.data_bytes += sg.bytes;
    const uint64_t need = sizeof(PackHdr) + segs.size() * sizeof(uint64_t) + hdr.data_bytes;
    if (bytes < need) return fail(TDMPC2_ERR_INVALID, "buffer of %llu bytes, the packed weights need %llu", (unsigned long long)bytes, (unsigned long long)need);
    char *dst = static_cast<char *>(host_buf);
    memcpy(dst, &hdr, sizeof hdr);
    uint64_t *sizes = reinterpret_cast<uint64_t *>(dst + sizeof hdr);
    char *data = dst + sizeof hdr + segs.size() * sizeof(uint64_t);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // binds on this stream have landed
    for (size_t i = 0; i < segs.size(); ++i) {
        sizes[i] = segs[i].bytes;
        HIP_TRY(hipMemcpy(data, segs[i].p, segs[i].bytes, hipMemcpyDeviceToHost));
        data += segs[i].bytes;
    }
    return TDMPC2_OK;
}

int tdmpc2_plan_import_packed(tdmpc2_plan_t *h, const void *host_buf, uint64_t bytes, void *stream) {
    if (!h || !host_buf) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    if (bytes < sizeof(PackHdr)) return fail(TDMPC2_ERR_INVALID, "packed weights: truncated header");
    PackHdr hdr;
    memcpy(&hdr, host_buf, sizeof hdr);
    if (memcmp(hdr.magic, "TDMPC2PK", 8) != 0 || hdr.version != 1) return fail(TDMPC2_ERR_INVALID, "not a packed weight blob (magic / version)");
    if (!same_model(hdr.cfg, h->cfg))
        return fail(TDMPC2_ERR_INVALID, "packed weights were exported for another model / kernel family / arithmetic "
                    "(latent %d mlp %d A %d path %d precision %d; this handle: %d %d %d %d %d)", hdr.cfg.latent_dim, hdr.cfg.mlp_dim,
                    hdr.cfg.action_dim, hdr.cfg.path, hdr.cfg.precision, h->cfg.latent_dim, h->cfg.mlp_dim, h->cfg.action_dim,
                    h->cfg.path, h->cfg.precision);
    if (hdr.enc_layers > (uint32_t)ENC_MAX_LAYERS) return fail(TDMPC2_ERR_INVALID, "packed weights: bad encoder depth");
    if (h->enc_layers && hdr.enc_layers && h->enc_layers != (int)hdr.enc_layers)
        return fail(TDMPC2_ERR_STATE, "encoder depth changed from %d to %u", h->enc_layers, hdr.enc_layers);
    int rc;
    for (int net : kPackNets) {
        if (!net_in_pack(h, net, hdr.has_target != 0)) continue;
        for (int l = 0; l < 3; ++l)
            if ((rc = ensure_layer_alloc(h, net, l, layer_shape(h, net, l)))) return rc;
    }
    for (uint32_t l = 0; l < hdr.enc_layers; ++l) {  // untrusted header fields: range-check before anything is allocated
        const int wmax = ENC_THREADS * ENC_MAX_PER_THREAD;
        if (hdr.enc_in[l] < 1 || hdr.enc_in[l] > 1 << 20 || hdr.enc_out[l] < 1 || hdr.enc_out[l] > wmax)
            return fail(TDMPC2_ERR_INVALID, "packed weights: encoder layer %u has shape [%d, %d]", l, hdr.enc_out[l], hdr.enc_in[l]);
    }
    for (uint32_t l = 0; l < hdr.enc_layers; ++l)
        if ((rc = ensure_enc_alloc(h, (int)l, hdr.enc_in[l], hdr.enc_out[l]))) return rc;
    std::vector<Seg> segs;
    collect_segments(h, hdr.has_target != 0, (int)hdr.enc_layers, segs);
    // the blob must hold exactly what this handle expects: header + size table + the sum of the EXPECTED segment sizes (the
    // header's own data_bytes is only compared, never trusted; no addition can wrap)
    uint64_t expect = 0;
    for (const Seg &sg : segs) {
        if (sg.bytes > (uint64_t)1 << 40 || expect > (uint64_t)1 << 41) return fail(TDMPC2_ERR_INVALID, "packed weights: implausible segment size");
        expect += sg.bytes;
    }
    const uint64_t need = sizeof(PackHdr) + (uint64_t)segs.size() * sizeof(uint64_t) + expect;
    if (segs.size() != hdr.nseg || hdr.data_bytes != expect || bytes < need)
        return fail(TDMPC2_ERR_INVALID, "packed weights: %llu segments / %llu data bytes in a buffer of %llu bytes; this handle expects %zu segments / "
                    "%llu data bytes (%llu in all)", (unsigned long long)hdr.nseg, (unsigned long long)hdr.data_bytes, (unsigned long long)bytes,
                    segs.size(), (unsigned long long)expect, (unsigned long long)need);
    const char *src = static_cast<const char *>(host_buf);
    const uint64_t *sizes = reinterpret_cast<const uint64_t *>(src + sizeof hdr);
    for (size_t i = 0; i < segs.size(); ++i)
        if (sizes[i] != segs[i].bytes) return fail(TDMPC2_ERR_INVALID, "packed weights: segment %zu has %llu bytes, expected %zu", i, (unsigned long long)sizes[i], segs[i].bytes);
    const char *data = src + sizeof hdr + segs.size() * sizeof(uint64_t);
    hipStream_t st = (hipStream_t)stream;
    for (size_t i = 0; i < segs.size(); ++i) {
        HIP_TRY(hipMemcpyAsync(segs[i].p, data, segs[i].bytes, hipMemcpyHostToDevice, st));
        data += segs[i].bytes;
    }
    HIP_TRY(hipStreamSynchronize(st));  // the host blob may be released on return
    for (int net : kPackNets) {
        if (!net_in_pack(h, net, hdr.has_target != 0)) continue;
        const int heads = layer_shape(h, net, 0).heads;
        for (int hd = 0; hd < heads; ++hd)
            for (int l = 0; l < 3; ++l) net_of(h, net, hd)->l[l].bound = true;
    }
    for (uint32_t l = 0; l < hdr.enc_layers; ++l) h->enc[l].bound = true;
    if (hdr.enc_layers) h->enc_layers = (int)hdr.enc_layers;
    return TDMPC2_OK;
}

}  // extern "C"
