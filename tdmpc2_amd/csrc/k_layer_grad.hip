// Translation unit of the trainable layer (tdmpc2_layer_*): the kernels of layer_grad_kernels.cuh and their host side.  It shares
// nothing with a planner handle and keeps no state: a call is its descriptor, its pointers and a caller-owned workspace.  Every
// decision (GEMM strides, grids, offsets, workspace layout, refusals on the descriptor) is layer_grad_route.h's; this file checks
// arguments, then launches.  Nothing is allocated, nothing synchronises the host: every call can be captured in a hipGraph.
#include "handle.h"
#include "layer_grad_route.h"

namespace {
using namespace tdk;
#include "layer_grad_kernels.cuh"

static_assert(sizeof(LgDesc) == sizeof(tdmpc2_layer_desc) && sizeof(LgDesc) == 32, "tdmpc2_layer_desc is 32 bytes, no padding");

int lg_desc(const tdmpc2_layer_desc *desc, LgDesc &d, const char *what) {
    if (!desc) return fail(TDMPC2_ERR_INVALID, "%s: null descriptor", what);
    d = LgDesc{desc->kind, desc->groups, desc->rows, desc->in_dim, desc->out_dim, desc->shared_x, desc->simnorm_dim, desc->ln_eps};
    switch (lg_check(d)) {
    case LG_OK: return 0;
    case LG_BAD_KIND: return fail(TDMPC2_ERR_INVALID, "%s: unknown kind %d (0 linear, 1 mish, 2 simnorm)", what, d.kind);
    case LG_BAD_DIMS:
        return fail(TDMPC2_ERR_INVALID, "%s: groups %d, rows %d, in_dim %d, out_dim %d: each must be at least 1", what, d.groups, d.rows,
                    d.in_dim, d.out_dim);
    case LG_BAD_SIMNORM:
        return fail(TDMPC2_ERR_INVALID, "%s: simnorm_dim %d must be at least 1 and divide out_dim %d", what, d.simnorm_dim, d.out_dim);
    case LG_BAD_SHARED: return fail(TDMPC2_ERR_INVALID, "%s: shared_x needs more than one group", what);
    default: return fail(TDMPC2_ERR_UNSUPPORTED, "%s: more than 2^31 workgroups in one launch", what);
    }
}

int lg_launch_gemm(int which, const LgDesc &d, const float *A, const float *B, float *C, const float *bias, const float *mask,
                   hipStream_t st) {
    LgGemmParams p{};
    p.g = lg_gemm(which, d);
    p.A = A; p.B = B; p.C = C; p.bias = bias; p.mask = mask;
    const dim3 grid((uint32_t)p.g.blocks), block(LG_THREADS);
    if (which == LG_FWD) hipLaunchKernelGGL((k_lg_gemm<true, true>), grid, block, 0, st, p);
    else if (which == LG_DX) hipLaunchKernelGGL((k_lg_gemm<true, false>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((k_lg_gemm<false, false>), grid, block, 0, st, p);
    LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" {

int tdmpc2_layer_workspace_bytes(const tdmpc2_layer_desc *desc, size_t *backward_ws_bytes) {
    LgDesc d;
    if (int rc = lg_desc(desc, d, "layer_workspace_bytes")) return rc;
    if (!backward_ws_bytes) return fail(TDMPC2_ERR_INVALID, "layer_workspace_bytes: null argument");
    *backward_ws_bytes = (size_t)lg_ws(d).bytes;
    return 0;
}

int tdmpc2_layer_forward(const tdmpc2_layer_desc *desc, const float *x, const float *w, const float *b, const float *ln_w,
                         const float *ln_b, const float *mask, float *y, float *pre, float *stat, void *stream) {
    LgDesc d;
    if (int rc = lg_desc(desc, d, "layer_forward")) return rc;
    if (!x || !w || !b || !y) return fail(TDMPC2_ERR_INVALID, "layer_forward: null x, w, b or y");
    const bool ln = d.kind != LG_LINEAR;
    if (ln && (!ln_w || !ln_b || !pre || !stat))
        return fail(TDMPC2_ERR_INVALID, "layer_forward: a layer with LayerNorm needs ln_w, ln_b, pre and stat (null given)");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = lg_launch_gemm(LG_FWD, d, x, w, ln ? pre : y, b, mask, st)) return rc;
    if (ln) {
        LgRowParams rp{};
        rp.d = d;
        rp.pre = pre; rp.ln_w = ln_w; rp.ln_b = ln_b; rp.stat = stat; rp.y = y;
        hipLaunchKernelGGL(k_lg_row_fwd, dim3((uint32_t)lg_row_blocks(d)), dim3(64 * LG_ROW_WAVES), 0, st, rp);
        LAUNCH_CHECK();
    }
    return 0;
}

int tdmpc2_layer_backward(const tdmpc2_layer_desc *desc, const float *x, const float *w, const float *ln_w, const float *ln_b,
                          const float *pre, const float *stat, const float *mask, const float *dy, float *dx, float *dw, float *db,
                          float *dln_w, float *dln_b, void *ws, size_t ws_bytes, void *stream) {
    LgDesc d;
    if (int rc = lg_desc(desc, d, "layer_backward")) return rc;
    const bool ln = d.kind != LG_LINEAR;
    const int given = (dw != nullptr) + (db != nullptr) + (ln ? (dln_w != nullptr) + (dln_b != nullptr) : 0), all = ln ? 4 : 2;
    if (given != 0 && given != all)
        return fail(TDMPC2_ERR_INVALID, "layer_backward: %d of the %d parameter gradients given (dw, db%s: all or none)", given, all,
                    ln ? ", dln_w, dln_b" : "");
    const bool params = given != 0;
    if (!dx && !params) return fail(TDMPC2_ERR_INVALID, "layer_backward: dx and every parameter gradient are null: nothing to compute");
    if (!dy) return fail(TDMPC2_ERR_INVALID, "layer_backward: null dy");
    if (dx && !w) return fail(TDMPC2_ERR_INVALID, "layer_backward: dx needs w (null given)");
    if (params && !x) return fail(TDMPC2_ERR_INVALID, "layer_backward: the parameter gradients need x (null given)");
    if (ln && (!ln_w || !ln_b || !pre || !stat))
        return fail(TDMPC2_ERR_INVALID, "layer_backward: a layer with LayerNorm needs ln_w, ln_b, pre and stat (null given)");
    const LgWs lay = lg_ws(d);
    const bool rowk = ln || mask;  // Linear without a mask: dlin IS dy
    if (rowk) {
        if (!ws) return fail(TDMPC2_ERR_INVALID, "layer_backward: null workspace");
        if (ws_bytes < lay.bytes)
            return fail(TDMPC2_ERR_INVALID, "layer_backward: workspace of %llu bytes is too small, %llu needed (tdmpc2_layer_workspace_bytes)",
                        (unsigned long long)ws_bytes, (unsigned long long)lay.bytes);
    }
    hipStream_t st = (hipStream_t)stream;
    float *dlin_ws = rowk ? (float *)((unsigned char *)ws + lay.dlin_off) : nullptr;
    float *du_ws = ln ? (float *)((unsigned char *)ws + lay.du_off) : nullptr;
    const float *dlin = rowk ? dlin_ws : dy;
    if (rowk) {
        LgRowParams rp{};
        rp.d = d;
        rp.pre = pre; rp.ln_w = ln_w; rp.ln_b = ln_b; rp.mask = mask; rp.dy = dy; rp.stat_in = stat; rp.du = du_ws; rp.dlin = dlin_ws;
        hipLaunchKernelGGL(k_lg_row_bwd, dim3((uint32_t)lg_row_blocks(d)), dim3(64 * LG_ROW_WAVES), 0, st, rp);
        LAUNCH_CHECK();
    }
    if (params) {
        LgColParams cp{};
        cp.d = d;
        cp.dlin = dlin; cp.du = du_ws; cp.pre = pre; cp.stat = stat; cp.db = db; cp.dln_w = dln_w; cp.dln_b = dln_b;
        hipLaunchKernelGGL(k_lg_cols, dim3((uint32_t)lg_col_blocks(d)), dim3(LG_COLS * LG_PARTS), 0, st, cp);
        LAUNCH_CHECK();
        if (int rc = lg_launch_gemm(LG_DW, d, dlin, x, dw, nullptr, nullptr, st)) return rc;
    }
    if (dx)
        if (int rc = lg_launch_gemm(LG_DX, d, dlin, w, dx, nullptr, nullptr, st)) return rc;
    return 0;
}

}  // extern "C"
