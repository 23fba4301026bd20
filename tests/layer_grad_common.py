"""The trainable layer (tdmpc2_layer_forward / tdmpc2_layer_backward) restated for the tests:
  - `closed_form`: forward and the closed-form backward of include/tdmpc2_plan.h in numpy, generic in the dtype.  With
    dtype float64 and exact contractions it is the reference; with float32 and `chain_gemm` (per output element serial fmaf
    chains in rising reduction index, what v_mfma_f32_32x32x2_f32 computes, cut every 256 elements as layer_grad_route.h cuts
    them) it is an emulation of the library's arithmetic.
  - `torch_grads`: torch autograd of the same layer in a given dtype (fp64: checks the closed form; fp32: the yardstick of the
    measured gate).
  - the cases of the gates, shared by the CPU and the GPU tests, and the header tdmpc2_amd/csrc/layer_grad_route.h behind a C shim."""
import ctypes
import functools
import os

import numpy as np

from tests import route_shim
from tests.route_shim import rel_err  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINEAR, MISH, SIMNORM = 0, 1, 2
KIND_NAMES = {LINEAR: "linear", MISH: "mish", SIMNORM: "simnorm"}
OUTPUTS = ("y", "dx", "dw", "db", "dln_w", "dln_b")
EPS = 1e-5
U = 2.0 ** -24  # unit roundoff of fp32

# ---------------------------------------------------------------- shapes (the issue's table)
EDGE_R = (1, 31, 32, 33, 65)
EDGE_K = (1, 2, 3, 31, 33, 70)
EDGE_N = {LINEAR: (1, 5, 33, 101), MISH: (2, 24, 40, 72), SIMNORM: (8, 24, 40, 72)}
EDGE_G = ((1, False), (2, False), (2, True), (5, True), (5, False), (1, False))  # (groups, shared_x)
MODEL_SHAPE = (1, False, 96, 518, 512)
LONG_ROW = (1, False, 33, 8, 4096)
LONG_K = (1, False, 33, 4096, 64)


def edge_shapes(kind):
    """(G, shared_x, R, K, N): every value of the table with this kind; a layer call runs all three GEMMs, so every value sits
    on an output-row, an output-column and a reduction dimension of one of them."""
    out = []
    for i in range(6):
        G, sh = EDGE_G[i]
        out.append((G, sh, EDGE_R[(i + kind) % 5], EDGE_K[i], EDGE_N[kind][(i + 2 * kind) % 4]))
    out.append((2, True, EDGE_R[(5 + kind) % 5], EDGE_K[(3 + kind) % 6], EDGE_N[kind][(1 + kind) % 4]))
    return out


def all_shapes(kind):
    return edge_shapes(kind) + [MODEL_SHAPE, LONG_ROW] + ([LONG_K] if kind == LINEAR else [])


def shape_id(s):
    G, sh, R, K, N = s
    return f"G{G}{'s' if sh else ''}-R{R}-K{K}-N{N}"


# ---------------------------------------------------------------- cases
def make_case(kind, shape, style="plain", mask=False, seed=0, integer=False):
    """Inputs of one layer call as fp32 numpy arrays.  style 'trained': LayerNorm gains log-uniform in [0.2, 5], every 7th input
    column of w x 20.  Mish / SimNorm rows reach past the softplus threshold and over +-50 logits through ln_b of columns 0 and 1
    (N >= 8).  integer: x, dy in {-2..2}, w in {-1, 0, 1}, integer b, mask in {0, 2} -- every sum stays far below 2^24."""
    G, sh, R, K, N = shape
    rng = np.random.default_rng([seed, kind, G, int(sh), R, K, N, style == "trained", int(mask)])
    f = np.float32
    c = dict(kind=kind, G=G, R=R, K=K, N=N, shared=bool(sh), sd=8 if kind == SIMNORM else 0, eps=EPS)
    xs = (R, K) if sh else (G, R, K)
    if integer:
        c["x"] = rng.integers(-2, 3, xs).astype(f)
        c["w"] = rng.integers(-1, 2, (G, N, K)).astype(f)
        c["b"] = rng.integers(-3, 4, (G, N)).astype(f)
        c["dy"] = rng.integers(-2, 3, (G, R, N)).astype(f)
        c["mask"] = (2 * rng.integers(0, 2, (G, R, N))).astype(f) if mask else None
    else:
        c["x"] = rng.standard_normal(xs).astype(f)
        c["w"] = (rng.standard_normal((G, N, K)) / np.sqrt(K)).astype(f)
        c["b"] = (0.1 * rng.standard_normal((G, N))).astype(f)
        c["dy"] = rng.standard_normal((G, R, N)).astype(f)
        p = 0.25
        c["mask"] = ((rng.random((G, R, N)) >= p) / (1 - p)).astype(f) if mask else None
    c["ln_w"] = (1 + 0.1 * rng.standard_normal((G, N))).astype(f)
    c["ln_b"] = (0.1 * rng.standard_normal((G, N))).astype(f)
    if style == "trained":
        c["ln_w"] = np.exp(rng.uniform(np.log(0.2), np.log(5.0), (G, N))).astype(f)
        c["w"][:, :, ::7] *= 20
    if kind != LINEAR and N >= 8:
        far = 22.0 if kind == MISH else 50.0
        c["ln_b"][:, 0], c["ln_b"][:, 1] = far, -far
    return c


# ---------------------------------------------------------------- contractions
def exact_gemm(a, b):
    """a [..., M, L] @ b [..., L, N] in the arrays' dtype (fp64: the reference)."""
    return np.matmul(a, b)


SEG = 256  # LG_SEG_TRIPS * LG_KT of layer_grad_route.h: reduction elements per partial chain


def chain_gemm(a, b):
    """fp32, as the library's GEMM sums: one serial chain acc = fmaf(a[m, l], b[l, n], acc) in rising l per SEG reduction elements
    (what v_mfma_f32_32x32x2_f32 computes), the partial chains added in rising order.  The product of two fp32 values is exact in
    fp64; the sum with the fp32 accumulator is rounded to fp64 and then to fp32, which differs from a true fmaf only where the fp64
    sum lands within 2^-29 ulp of a tie: an emulation for error statistics, not for bit equality."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    total = None
    for s0 in range(0, a.shape[-1], SEG):
        acc = np.zeros(a.shape[:-1] + (b.shape[-1],), np.float32)
        for l in range(s0, min(s0 + SEG, a.shape[-1])):
            acc = (a64[..., :, l, None] * b64[..., l, None, :] + acc).astype(np.float32)
        total = acc if total is None else total + acc
    return total


def mish_terms(u):
    """(t, 1 - t^2, sigmoid(u)) with t = tanh(softplus(u)), softplus threshold 20, in u's dtype.  With e = exp(u) and n = e (e + 2):
    t = n / (n + 2) and 1 - t = 2 / (n + 2), so neither tanh(log1p(.)) nor the cancellation of 1 - t * t near t = 1 is evaluated
    (the same functions; in fp32 the difference is several ulp of the derivative).  Past the threshold softplus(u) = u and
    tanh(u) rounds to 1 in either precision."""
    one = u.dtype.type(1)
    big = u > 20
    e = np.exp(np.minimum(u, u.dtype.type(20)))
    n = e * (e + 2)
    t = np.where(big, one, n / (n + 2))
    return t, np.where(big, 0 * one, (2 / (n + 2)) * (one + t)), np.where(big, one, e / (one + e))


def closed_form(c, dtype=np.float64, gemm=exact_gemm, want_abs=False):
    """-> dict of OUTPUTS (those the kind has) in `dtype`, plus 'pre', 'stat'.  want_abs (Linear): also 'abs_y', 'abs_dx', 'abs_dw':
    the same contractions over absolute values (the sum |a| |b| of the a-priori fmaf-chain bound)."""
    t = lambda v: None if v is None else v.astype(dtype)  # noqa: E731
    kind, G, R, K, N, sh = c["kind"], c["G"], c["R"], c["K"], c["N"], c["shared"]
    x, w, b, dy, mask = t(c["x"]), t(c["w"]), t(c["b"]), t(c["dy"]), t(c["mask"])
    xg = np.broadcast_to(x, (G, R, K)) if sh else x
    one = dtype(1)
    lin = gemm(xg, np.swapaxes(w, 1, 2)) + b[:, None, :]
    pre = lin if mask is None else lin * mask
    out = {}
    if kind == LINEAR:
        out["y"] = pre
        dpre = dy
    else:
        lw, lb = t(c["ln_w"])[:, None, :], t(c["ln_b"])[:, None, :]
        mean = pre.mean(-1, keepdims=True, dtype=dtype)
        var = ((pre - mean) ** 2).mean(-1, keepdims=True, dtype=dtype)
        rstd = one / np.sqrt(var + dtype(c["eps"]))
        xh = (pre - mean) * rstd
        u = xh * lw + lb
        if kind == MISH:
            th, omt2, sg = mish_terms(u)
            out["y"] = u * th
            du = dy * (th + u * sg * omt2)
        else:
            ug = u.reshape(G, R, N // c["sd"], c["sd"])
            e = np.exp(ug - ug.max(-1, keepdims=True))
            yg = e / e.sum(-1, keepdims=True, dtype=dtype)
            out["y"] = yg.reshape(G, R, N)
            dyg = dy.reshape(ug.shape)
            du = (yg * (dyg - (dyg * yg).sum(-1, keepdims=True, dtype=dtype))).reshape(G, R, N)
        out["dln_w"] = (du * xh).sum(1, dtype=dtype)
        out["dln_b"] = du.sum(1, dtype=dtype)
        dxh = du * lw
        dpre = rstd * (dxh - dxh.mean(-1, keepdims=True, dtype=dtype) - xh * (dxh * xh).mean(-1, keepdims=True, dtype=dtype))
        out["pre"], out["stat"] = pre, np.concatenate([mean, rstd], -1)
    dlin = dpre if mask is None else dpre * mask
    out["db"] = dlin.sum(1, dtype=dtype)
    out["dw"] = gemm(np.swapaxes(dlin, 1, 2), xg)
    if sh:  # one reduction over (g, n), g outermost, every group padded with zeros to whole trips of 32 (as the kernel stages it)
        pad = (-N) % 32
        dl, wp = np.pad(dlin, ((0, 0), (0, 0), (0, pad))), np.pad(w, ((0, 0), (0, pad), (0, 0)))
        out["dx"] = gemm(np.swapaxes(dl, 0, 1).reshape(R, G * (N + pad)), wp.reshape(G * (N + pad), K))
    else:
        out["dx"] = gemm(dlin, w)
    if want_abs:
        ax, aw, ad = np.abs(xg), np.abs(w), np.abs(dlin)
        out["abs_y"] = exact_gemm(ax, np.swapaxes(aw, 1, 2))
        out["abs_dw"] = exact_gemm(np.swapaxes(ad, 1, 2), ax)
        out["abs_dx"] = exact_gemm(np.swapaxes(ad, 0, 1).reshape(R, G * N), aw.reshape(G * N, K)) if sh else exact_gemm(ad, aw)
    return out


def torch_layer(kind, x, w, b, ln_w, ln_b, mask, sd, eps, shared):
    """The layer in torch ops, as tdmpc2_amd.layers computes it: NormedLinear for one group (F.linear, F.layer_norm with its
    affine), QEnsemble.apply_params for stacked parameters (baddbmm, F.layer_norm without affine, then gain and bias)."""
    import torch
    import torch.nn.functional as F

    G, N = w.shape[0], w.shape[1]
    if G == 1:
        h = F.linear(x[0], w[0], b[0])
        if mask is not None:
            h = h * mask[0]
        if kind != LINEAR:
            h = F.layer_norm(h, (N,), ln_w[0], ln_b[0], eps)
        h = h.unsqueeze(0)
    else:
        xg = x.unsqueeze(0).expand(G, *x.shape) if shared else x
        h = torch.baddbmm(b.unsqueeze(1), xg, w.transpose(1, 2))
        if mask is not None:
            h = h * mask
        if kind != LINEAR:
            h = F.layer_norm(h, (N,), None, None, eps) * ln_w.unsqueeze(1) + ln_b.unsqueeze(1)
    if kind == MISH:
        h = F.mish(h)
    elif kind == SIMNORM:
        h = F.softmax(h.view(*h.shape[:-1], -1, sd), dim=-1).view(h.shape)
    return h


def torch_grads(c, dtype, device="cpu"):
    """torch autograd of `torch_layer` with dy as the seed -> dict of OUTPUTS as numpy arrays."""
    import torch

    mk = lambda v, g=True: None if v is None else torch.tensor(v, dtype=dtype, device=device, requires_grad=g)  # noqa: E731
    ln = c["kind"] != LINEAR
    x, w, b = mk(c["x"]), mk(c["w"]), mk(c["b"])
    lw, lb = (mk(c["ln_w"]), mk(c["ln_b"])) if ln else (None, None)
    y = torch_layer(c["kind"], x, w, b, lw, lb, mk(c["mask"], False), c["sd"], c["eps"], c["shared"])
    y.backward(mk(c["dy"], False))
    out = {"y": y.detach(), "dx": x.grad, "dw": w.grad, "db": b.grad}
    if ln:
        out["dln_w"], out["dln_b"] = lw.grad, lb.grad
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def measured_reference(kind, shape, style, mask):
    """Computed once per case and shared: (case, fp64 closed form, e(T) of torch's CPU fp32 autograd per tensor)."""
    import torch

    c = make_case(kind, shape, style, mask)
    ref = closed_form(c)
    t32 = torch_grads(c, torch.float32)
    return c, ref, {k: rel_err(t32[k], ref[k]) for k in t32}


def measured_cases():
    """(kind, shape, style, mask) of the measured gate: Mish and SimNorm, both weight styles, every edge shape and the two large ones;
    a dropout mask on every other edge shape."""
    out = []
    for kind in (MISH, SIMNORM):
        for style in ("plain", "trained"):
            for i, s in enumerate(all_shapes(kind)):
                out.append((kind, s, style, i % 2 == 1))
    return out


def case_id(k):
    kind, s, style, mask = k
    return f"{KIND_NAMES[kind]}-{style}-{shape_id(s)}{'-mask' if mask else ''}"


# ---------------------------------------------------------------- tdmpc2_amd/csrc/layer_grad_route.h behind a C shim
SHIM = r"""
#include <string.h>
#include "layer_grad_route.h"
static LgDesc mk(const int32_t *v) { return LgDesc{v[0], v[1], v[2], v[3], v[4], v[5], v[6], 1e-5f}; }
extern "C" int check(const int32_t *v) { return lg_check(mk(v)); }
// out: M, Nc, L, batch, gsum, tiles_m, tiles_n, a_m, a_l, a_g, b_n, b_l, b_g, ldc, c_g, blocks
extern "C" void gemm(int which, const int32_t *v, uint64_t *out) {
    const LgGemm g = lg_gemm(which, mk(v));
    const uint64_t o[16] = {(uint64_t)g.M, (uint64_t)g.Nc, (uint64_t)g.L, (uint64_t)g.batch, (uint64_t)g.gsum, (uint64_t)g.tiles_m,
                            (uint64_t)g.tiles_n, g.a_m, g.a_l, g.a_g, g.b_n, g.b_l, g.b_g, g.ldc, g.c_g, g.blocks};
    memcpy(out, o, sizeof o);
}
// every (workgroup, wave, lane, register) of the GEMM's grid that passes the kernel's bounds test adds one to its output element;
// returns the number of writes that fell outside [0, n_out)
extern "C" uint64_t cover(int which, const int32_t *v, uint32_t *count, uint64_t n_out) {
    const LgGemm g = lg_gemm(which, mk(v));
    uint64_t bad = 0;
    for (uint64_t blk = 0; blk < g.blocks; ++blk) {
        const LgTile t = lg_tile(g, blk);
        for (int wave = 0; wave < LG_WAVES; ++wave)
            for (int lane = 0; lane < 64; ++lane)
                for (int i = 0; i < 16; ++i) {
                    const int m = t.m0 + lg_wave_m(wave) + lg_acc_row(lane, i), n = t.n0 + lg_wave_n(wave) + lg_acc_col(lane);
                    if (m >= g.M || n >= g.Nc) continue;
                    const uint64_t off = lg_c_off(g, (uint64_t)t.out, (uint64_t)m, (uint64_t)n);
                    if (off < n_out) ++count[off]; else ++bad;
                }
    }
    return bad;
}
// the reduction indices one accumulator sees, in order: trip by trip, step by step, k = 0 then k = 1 of a step (the MFMA's order)
extern "C" int chain(int L, int32_t *out) {
    int n = 0;
    for (int trip = 0; trip < lg_trips(L); ++trip)
        for (int s = 0; s < LG_KT / LG_KSTEP; ++s)
            for (int half = 0; half < 2; ++half) {
                const int l = trip * LG_KT + lg_step_k(32 * half, s);
                if (l < L) out[n++] = l;
            }
    return n;
}
extern "C" void offsets(int which, const int32_t *v, uint64_t grp, uint64_t m, uint64_t n, uint64_t l, uint64_t *out) {
    const LgGemm g = lg_gemm(which, mk(v));
    out[0] = lg_a_off(g, grp, m, l); out[1] = lg_b_off(g, grp, l, n); out[2] = lg_c_off(g, grp, m, n);
}
extern "C" uint64_t off3(uint64_t g, uint64_t r, uint64_t c, uint64_t R, uint64_t C) { return lg_off3(g, r, c, R, C); }
extern "C" void ws(const int32_t *v, uint64_t *out) { const LgWs w = lg_ws(mk(v)); out[0] = w.dlin_off; out[1] = w.du_off; out[2] = w.bytes; }
extern "C" int col_part(int row) { return lg_col_part(row); }
extern "C" void grids(const int32_t *v, uint64_t *out) { const LgDesc d = mk(v); out[0] = lg_row_blocks(d); out[1] = lg_col_blocks(d); out[2] = (uint64_t)lg_col_tiles(d); }
extern "C" void constants(int32_t *out) {
    const int32_t c[10] = {LG_THREADS, LG_TILE, LG_BM, LG_BN, LG_KT, LG_KSTEP, LG_ROW_WAVES, LG_COLS, LG_PARTS, LG_ALIGN};
    memcpy(out, c, sizeof c);
}
"""
CONSTANT_KEYS = ("THREADS", "TILE", "BM", "BN", "KT", "KSTEP", "ROW_WAVES", "COLS", "PARTS", "ALIGN")
GEMM_KEYS = ("M", "Nc", "L", "batch", "gsum", "tiles_m", "tiles_n", "a_m", "a_l", "a_g", "b_n", "b_l", "b_g", "ldc", "c_g", "blocks")
FWD, DX, DW = 0, 1, 2


def desc_words(kind, G, R, K, N, shared=False, sd=0):
    return (ctypes.c_int32 * 7)(kind, G, R, K, N, int(shared), sd)


def build_route(tmpdir, extra_flags=()):
    i32p, u64, u64p = ctypes.POINTER(ctypes.c_int32), ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)
    return route_shim.build_shim(tmpdir, "layer_grad_route", SHIM, dict(
        check=[i32p], gemm=[ctypes.c_int, i32p, u64p], cover=([ctypes.c_int, i32p, ctypes.POINTER(ctypes.c_uint32), u64], u64),
        chain=[ctypes.c_int, i32p], offsets=[ctypes.c_int, i32p, u64, u64, u64, u64, u64p], off3=([u64] * 5, u64), ws=[i32p, u64p],
        col_part=[ctypes.c_int], grids=[i32p, u64p], constants=[i32p]), ("-O2", *extra_flags))


def route_gemm(lib, which, words):
    out = (ctypes.c_uint64 * 16)()
    lib.gemm(which, words, out)
    return dict(zip(GEMM_KEYS, [int(v) for v in out]))
