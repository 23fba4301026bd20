// Translation unit of the pixel encoder in training (tdmpc2_pixgrad_*, include/tdmpc2_pixel_grad.h): the kernels of
// pixel_grad_kernels.cuh and their host side.  It shares nothing with a planner handle and keeps no state: a call is its descriptor,
// its pointers and caller-owned workspaces.  Every decision (views, grids, orders, offsets, refusals on the descriptor) is
// pixel_grad_route.h's; this file checks arguments, then launches.  The forward's four layers are the batch route's own kernels,
// reached through pixb_launch of launch.h.  Nothing is allocated, nothing synchronises the host: every call can be captured.
#include "../../include/tdmpc2_pixel_grad.h"
#include "launch.h"
#include "pixel_grad_route.h"

namespace {
using namespace tdk;
#include "pixel_grad_kernels.cuh"

static_assert(sizeof(PgDesc) == sizeof(tdmpc2_pixgrad_desc) && sizeof(PgDesc) == 24, "tdmpc2_pixgrad_desc is 24 bytes");
static_assert(sizeof(PixTap) == 16, "a ShiftAug tap is 16 bytes");

int pg_desc(const tdmpc2_pixgrad_desc *s, PgDesc &d, const char *what) {
    if (!s) return fail(TDMPC2_ERR_INVALID, "%s: null descriptor", what);
    d = PgDesc{s->n, s->cin, s->C, s->obs_dtype, s->seed_is_preact, 0u};
    switch (pg_check(d)) {
    case PG_OK: return 0;
    case PG_BAD_N: return fail(TDMPC2_ERR_INVALID, "%s: n %d < 1", what, (int)d.n);
    case PG_BAD_CIN: return fail(TDMPC2_ERR_UNSUPPORTED, "%s: %d input channels outside [1, %d]", what, (int)d.cin, PIX_MAX_CIN);
    case PG_BAD_C:
        return fail(TDMPC2_ERR_UNSUPPORTED, "%s: %d channels outside [%d, %d] or no multiple of %d", what, (int)d.C, PIX_MIN_C, PIX_MAX_C, PIX_CO);
    case PG_BAD_DTYPE: return fail(TDMPC2_ERR_INVALID, "%s: obs_dtype %d (0 = uint8, 1 = float32)", what, (int)d.obs_dtype);
    case PG_BAD_SEED: return fail(TDMPC2_ERR_INVALID, "%s: seed_is_preact %d (0 or 1)", what, (int)d.seed_is_preact);
    default: return fail(TDMPC2_ERR_UNSUPPORTED, "%s: n %d above %d images", what, (int)d.n, PG_MAX_N);
    }
}

template <int L>
int launch_da(const PgParams &p, hipStream_t st) {
    hipLaunchKernelGGL((k_pg_da<L>), dim3((uint32_t)pg_da_blocks(L, p.fw.n)), dim3(PIXB_THREADS), pg_da_lds(L, p.fw.C), st, p);
    LAUNCH_CHECK();
    return 0;
}

template <int L, bool U8>
int launch_dw(const PgParams &p, hipStream_t st) {
    const size_t lds = pg_dw_lds(L, p.fw.cin);
    if (L == 0)  // layer 0 stages the forward's patch: above the default dynamic LDS limit for most cin
        if (int rc = set_lds(k_pg_dw<L, U8>, pg_dw_lds(0, PIX_MAX_CIN))) return rc;
    const dim3 grid((uint32_t)pg_chunks(L, p.fw.n), (uint32_t)pg_dw_grid_y(L, p.fw.cin, p.fw.C));
    hipLaunchKernelGGL((k_pg_dw<L, U8>), grid, dim3(PIXB_THREADS), lds, st, p);
    LAUNCH_CHECK();
    const int M = pg_dw_m(L, p.fw.cin, p.fw.C);
    hipLaunchKernelGGL(k_pg_fold, dim3((uint32_t)pg_fold_blocks(M, p.fw.C)), dim3(PG_FOLD_THREADS), 0, st, p.part, pg_chunks(L, p.fw.n), M,
                       p.fw.C, p.dW[L], p.db[L]);
    LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" {

int tdmpc2_pixgrad_workspace_bytes(const tdmpc2_pixgrad_desc *desc, size_t *acts_bytes, size_t *fwd_ws_bytes, size_t *bwd_ws_bytes) {
    PgDesc d;
    if (int rc = pg_desc(desc, d, "pixgrad_workspace_bytes")) return rc;
    if (!acts_bytes || !fwd_ws_bytes || !bwd_ws_bytes) return fail(TDMPC2_ERR_INVALID, "pixgrad_workspace_bytes: null argument");
    *acts_bytes = pg_acts_floats(d.n, d.C) * sizeof(float);
    *fwd_ws_bytes = pg_fwd_ws_floats(d.cin, d.C) * sizeof(float);
    *bwd_ws_bytes = pg_bwd_ws_floats(d.n, d.cin, d.C) * sizeof(float);
    return 0;
}

int tdmpc2_pixgrad_shift_table(void *host_out) {
    if (!host_out) return fail(TDMPC2_ERR_INVALID, "pixgrad_shift_table: null argument");
    pix_shift_table(static_cast<PixTap *>(host_out));
    return 0;
}

int tdmpc2_pixgrad_forward(const tdmpc2_pixgrad_desc *desc, const void *obs, const int32_t *shift, const void *tab,
                           const float *const W[4], const float *const b[4], float *fwd_ws, float *acts, void *stream) {
    PgDesc d;
    if (int rc = pg_desc(desc, d, "pixgrad_forward")) return rc;
    if (!obs || !shift || !tab || !W || !b || !fwd_ws || !acts) return fail(TDMPC2_ERR_INVALID, "pixgrad_forward: null argument");
    for (int l = 0; l < PIX_LAYERS; ++l)
        if (!W[l] || !b[l]) return fail(TDMPC2_ERR_INVALID, "pixgrad_forward: null weight or bias of layer %d", l);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pixb_set_lds(pixb_lds(0, PIX_MAX_C, PIX_MAX_CIN))) return rc;
    PgPackParams pk{};
    PixbParams p{};
    for (int l = 0; l < PIX_LAYERS; ++l) {
        pk.W[l] = W[l];
        pk.wp[l] = fwd_ws + pg_wp_off(l, d.cin, d.C);
        p.wp[l] = pk.wp[l];
        p.bias[l] = b[l];
    }
    pk.cin = d.cin; pk.C = d.C;
    const int most = (int)pg_wp_floats(1, d.cin, d.C) > (int)pg_wp_floats(0, d.cin, d.C) ? (int)pg_wp_floats(1, d.cin, d.C)
                                                                                         : (int)pg_wp_floats(0, d.cin, d.C);
    hipLaunchKernelGGL(k_pg_pack, dim3((uint32_t)((most + PG_ROW_THREADS - 1) / PG_ROW_THREADS)), dim3(PG_ROW_THREADS), 0, st, pk);
    LAUNCH_CHECK();
    p.obs = obs; p.cin = d.cin; p.C = d.C; p.n = d.n; p.shift = shift; p.tab = static_cast<const PixTap *>(tab);
    p.ws = acts;
    p.z = acts + pg_z_off(d.n, d.C);
    for (int l = 0; l < PIX_LAYERS; ++l)
        if (int rc = pixb_launch(l, d.obs_dtype == 0, p, pixb_grid(l, d.n, d.C, d.cin), st)) return rc;
    return 0;
}

int tdmpc2_pixgrad_backward(const tdmpc2_pixgrad_desc *desc, const void *obs, const int32_t *shift, const void *tab,
                            const float *const W[4], const float *acts, const float *dz, float *bwd_ws, float *const dW[4],
                            float *const db[4], void *stream) {
    PgDesc d;
    if (int rc = pg_desc(desc, d, "pixgrad_backward")) return rc;
    if (!obs || !shift || !tab || !W || !acts || !dz || !bwd_ws || !dW || !db) return fail(TDMPC2_ERR_INVALID, "pixgrad_backward: null argument");
    int lowest = PIX_LAYERS;  // the lowest layer whose gradients are asked for: nothing below it is computed
    for (int l = PIX_LAYERS - 1; l >= 0; --l) {
        if (!W[l]) return fail(TDMPC2_ERR_INVALID, "pixgrad_backward: null weight of layer %d", l);
        if ((dW[l] == nullptr) != (db[l] == nullptr))
            return fail(TDMPC2_ERR_INVALID, "pixgrad_backward: dW and db of layer %d are given or NULL together", l);
        if (dW[l]) lowest = l;
    }
    if (lowest == PIX_LAYERS) return fail(TDMPC2_ERR_INVALID, "pixgrad_backward: every dW / db pair is null: nothing to compute");
    hipStream_t st = (hipStream_t)stream;
    PgParams p{};
    p.fw.obs = obs; p.fw.cin = d.cin; p.fw.C = d.C; p.fw.n = d.n; p.fw.shift = shift; p.fw.tab = static_cast<const PixTap *>(tab);
    p.acts = acts;
    p.z = acts + pg_z_off(d.n, d.C);
    p.dz = dz;
    p.seed_is_preact = d.seed_is_preact;
    for (int l = 0; l < PIX_LAYERS; ++l) {
        p.W[l] = W[l];
        p.dy[l] = bwd_ws + pg_dy_off(l, d.n, d.C);
        p.dW[l] = dW[l];
        p.db[l] = db[l];
    }
    p.part = bwd_ws + pg_part_base(d.n, d.C);
    const size_t total = pg_dy_floats(3, d.n, d.C);
    hipLaunchKernelGGL(k_pg_seed, dim3((uint32_t)((total + PG_ROW_THREADS - 1) / PG_ROW_THREADS)), dim3(PG_ROW_THREADS), 0, st, p, total);
    LAUNCH_CHECK();
    int rc = 0;
    if (dW[3] && (rc = launch_dw<3, false>(p, st))) return rc;
    if (lowest < 3 && (rc = launch_da<3>(p, st))) return rc;
    if (dW[2] && (rc = launch_dw<2, false>(p, st))) return rc;
    if (lowest < 2 && (rc = launch_da<2>(p, st))) return rc;
    if (dW[1] && (rc = launch_dw<1, false>(p, st))) return rc;
    if (lowest < 1 && (rc = launch_da<1>(p, st))) return rc;
    if (dW[0]) rc = d.obs_dtype == 0 ? launch_dw<0, true>(p, st) : launch_dw<0, false>(p, st);
    return rc;
}

}  // extern "C"
