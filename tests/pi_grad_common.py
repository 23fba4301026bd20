"""The policy-loss unit (tdmpc2_pigrad_*, include/tdmpc2_pi_grad.h) restated for the tests:
  - `closed_form`: every forward value of the five calls and every gradient seed in numpy, generic in the dtype.  float64 is the
    reference; float32 follows the library's arithmetic (its bins, per-step constants computed in fp64 and rounded once, g as one fp32
    factor, the two cancelling terms of d scaled_entropy / d log_prob taken together) without claiming its bits.
  - `torch_ref`: torch autograd on the CPU of the port's own expression (`world_model._pi_tail`, `world_model.two_hot_inv`, the loss
    line of update_pi): the yardstick of the measured gates in fp32, the reference in fp64.
  - the fixture's inputs, the shape cases shared by the tests, and pi_grad_route.h behind a C shim.

Hyperparameters are fp32 in the C ABI.  `hyper` returns the doubles the library computes with (fp32(1e-4) = 0.0000999999974737875...):
every reference gets those, so the gates measure arithmetic and not the representation of 1e-4 in fp32.

The expression has one discontinuity: symexp'(x) is exp|x| everywhere but 0 at x == 0 exactly.  A logit row whose softmax is symmetric
about the centre of the bins (an all-equal row) sits on it: whether x comes out as 0 or as 1e-17 depends on the order of a sum.  The
fixture carries such a row at 101 bins, where neither torch's fp64 sum nor the library's is exactly 0; the generated shape cases carry
none."""
import ctypes
import os

import numpy as np

from tests import route_shim
from tests.optim_common import FLOOR, MARGIN, rel_err, widen  # noqa: F401  (the measured gate of DESIGN 3.4h)
from tests.route_shim import gate, ordered_sum_model  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pi_grad.npz")
HYPER_KEYS = ("vmin", "vmax", "rho", "entropy_coef", "log_std_min", "log_std_dif")
SYMBOLS = ("tdmpc2_pigrad_head_forward", "tdmpc2_pigrad_head_backward", "tdmpc2_pigrad_value_forward",
           "tdmpc2_pigrad_loss_forward", "tdmpc2_pigrad_loss_backward")
FORWARD = ("action", "entropy", "scaled_entropy", "q", "losses", "step_means")
SEEDS = ("d_scaled_entropy", "d_q_logits", "d_pi_out")
INPUTS = ("pi_out", "eps", "mask", "q_logits", "d_action")
SCALES = (1.0, 37.5)
LOG_2PI_HALF = 0.9189385175704956


def hyper(vmin=-10.0, vmax=10.0, rho=0.5, entropy_coef=1e-4, log_std_min=-10.0, log_std_max=2.0):
    """The reference's defaults (config.yaml), each widened from fp32; log_std_dif as world_model.py:35 forms it (in fp32)."""
    dif = float(np.float32(log_std_max) - np.float32(log_std_min))
    return {k: widen(v) for k, v in zip(HYPER_KEYS, (vmin, vmax, rho, entropy_coef, log_std_min, dif))}


# ---------------------------------------------------------------- inputs
FIXTURE_CASES = {"single": dict(T=3, B=9, A=6, NB=101, live=None), "multi": dict(T=2, B=9, A=6, NB=101, live=(6, 3, 1))}


def mask_of(case):
    if case.get("live") is None:
        return None
    live = case["live"]
    m = np.zeros((case["B"], case["A"]), np.float32)
    for b in range(case["B"]):
        m[b, :live[b % len(live)]] = 1.0
    return m


def fixture_inputs(name):
    """fp32 inputs of a fixture case with the edges of the issue: raw log_std 0, +-6, +-20; means of +-12 with eps 0 (tanh == +-1 in
    fp32); eps 0 and +-4; logit rows all equal, one-hot on the centre bin and on the last bin by a 1e4 logit, every other row with
    a maximum of 1e4."""
    c = FIXTURE_CASES[name]
    T, B, A, NB = c["T"], c["B"], c["A"], c["NB"]
    rng = np.random.default_rng(dict(single=11, multi=20)[name])
    mean = rng.standard_normal((T, B, A))
    raw = 0.7 * rng.standard_normal((T, B, A)) - 1.0  # (log_std near its lower end: log_prob stays well above 1)
    eps = rng.standard_normal((T, B, A))
    raw[0, 0] = [0.0, 6.0, -6.0, 20.0, -20.0, 0.0]
    mean[0, 1] = [12.0, -12.0, 12.0, -12.0, 0.3, -0.2]
    eps[0, 1] = 0.0
    eps[0, 2] = [0.0, 4.0, -4.0, 0.0, 4.0, -4.0]
    raw[1, 3] = [20.0, -20.0, 6.0, -6.0, 0.0, 20.0]
    mean[1, 4] = [-12.0, 12.0, 0.0, 0.0, 12.0, -12.0]
    eps[1, 4] = 0.0
    q = 3.0 * rng.standard_normal((2, T, B, NB))
    q += 1e4 - q.max(-1, keepdims=True)
    rows = q.reshape(-1, NB)
    rows[0] = 1e4
    rows[1] = 0.0
    rows[1, NB // 2] = 1e4
    rows[2] = 0.0
    rows[2, NB - 1] = 1e4
    rows[-1] = 0.0
    rows[-1, NB // 2] = 1e4
    rows[-2] = -3.0
    x = dict(pi_out=np.concatenate([mean, raw], -1), eps=eps, q_logits=q, d_action=rng.standard_normal((T, B, A)))
    x = {k: np.ascontiguousarray(v, np.float32) for k, v in x.items()}
    x["mask"] = mask_of(c)
    return x


def _case(name, T, B, A, NB, live=None):
    return dict(name=name, T=T, B=B, A=A, NB=NB, live=live)


# A in {1, 6, 17, 38, 64}, NB in {2, 64, 65, 101, 129}, (T, B) in {(1, 1), (3, 9), (9, 33), (16, 5)}: not a cross product
CASE_LIST = [
    _case("one", 1, 1, 1, 2),
    _case("small", 3, 9, 6, 101),
    _case("odd", 9, 33, 17, 65),        # 297 rows: not a multiple of a workgroup's rows; a tail past 256 terms
    _case("deep", 16, 5, 38, 64),
    _case("wide", 3, 9, 64, 129),       # columns straddling 64 lanes
    _case("masked", 9, 33, 38, 101, live=(38, 17, 1, 8)),
    _case("mask1", 1, 1, 6, 2, live=(3,)),
]
CASES = {c["name"]: c for c in CASE_LIST}


def make_inputs(case, seed=0):
    """Generic fp32 inputs of a shape case: no row on the x == 0 discontinuity (see the module's docstring)."""
    T, B, A, NB = case["T"], case["B"], case["A"], case["NB"]
    rng = np.random.default_rng(2000 + seed)
    # (log_std near its lower end, as in the fixture: with a wide std the sample saturates tanh, and log(relu(1 - a^2) + 1e-6) then
    # turns the last bit of a into 0.1 of the row's entropy, in torch's fp32 as in the library's: a gate on luck, not on arithmetic)
    x = dict(pi_out=np.concatenate([np.clip(rng.standard_normal((T, B, A)), -3, 3), np.clip(0.7 * rng.standard_normal((T, B, A)) - 1.0, -3, 0)], -1),
             eps=rng.standard_normal((T, B, A)), q_logits=4.0 * rng.standard_normal((2, T, B, NB)),
             d_action=rng.standard_normal((T, B, A)))
    x = {k: np.ascontiguousarray(v, np.float32) for k, v in x.items()}
    x["mask"] = mask_of(case)
    return x


# ---------------------------------------------------------------- the closed form
def bins_of(h, NB, f):
    """torch.linspace(vmin, vmax, NB) in dtype f; float32: as the library forms it (pg_bin: the fp32 step, the rest in fp64, rounded
    once)."""
    k = np.arange(NB)
    if f == np.float32:
        step = float(np.float32((np.float32(h["vmax"]) - np.float32(h["vmin"])) / np.float32(NB - 1)))
    else:
        step = (h["vmax"] - h["vmin"]) / (NB - 1)
    return np.where(k < NB // 2, h["vmin"] + step * k, h["vmax"] - step * (NB - 1 - k)).astype(f)


def _tanh(v, f):
    """tanh in dtype f.  float64: torch's kernel, the fixture's own elementary function -- log(relu(1 - a^2) + 1e-6) turns an ulp of
    a near +-1 (1.1e-16) into 2e-10 of the entropy, 2e-12 of its maximum: two correctly rounded libraries a last bit apart would
    already miss the 1e-12 of tests/test_pi_grad_math.py.  Everything else of the closed form is numpy's."""
    if f == np.float64:
        import torch

        return torch.tanh(torch.from_numpy(np.ascontiguousarray(v, np.float64))).numpy()
    return np.tanh(v).astype(f)


def closed_form(x, case, h, scale, f=np.float64, g=1.0):
    """Every output of the five calls in dtype f.  d_pi_out is head_backward's for the incoming d_action = x['d_action'] and
    d_scaled_entropy = this loss's own seed, as update_pi chains them."""
    T, B, A, NB = case["T"], case["B"], case["A"], case["NB"]
    out = {}
    y, eps = np.asarray(x["pi_out"], f), np.asarray(x["eps"], f)
    m = None if x.get("mask") is None else np.asarray(x["mask"], f)
    lmin, ldif = f(h["log_std_min"]), f(h["log_std_dif"])
    with np.errstate(all="ignore"):
        mean, raw = y[..., :A], y[..., A:]
        th = _tanh(raw, f)
        ls = lmin + f(0.5) * ldif * (th + f(1))
        size = f(A)
        mm = f(1)
        if m is not None:
            mm = m[None]
            mean, ls, eps = mean * mm, ls * mm, eps * mm
            size = m.sum(-1, dtype=f)[None, :]
        sd = np.exp(ls)
        a = _tanh(mean + eps * sd, f)
        om = f(1) - a * a
        lp0 = (f(-0.5) * eps * eps - ls - f(LOG_2PI_HALF)).sum(-1, dtype=f)
        K = np.log(np.maximum(om, 0) + f(1e-6)).sum(-1, dtype=f)
        lp = lp0 - K
        den = lp + f(1e-8)
        S = lp0 * size
        out["action"], out["entropy"] = a.astype(f), (-lp).astype(f)
        out["scaled_entropy"] = se = ((-lp) * (S / den)).astype(f)
        # two_hot_inv of the two heads
        ql = np.asarray(x["q_logits"], f)
        bins = bins_of(h, NB, f)
        e = np.exp(ql - ql.max(-1, keepdims=True)).astype(f)
        es = e.sum(-1, keepdims=True, dtype=f)
        p = (e / es).astype(f)
        xv = (p * bins).sum(-1, dtype=f)
        qh = np.sign(xv) * (np.exp(np.abs(xv)) - f(1))
        out["q"] = q = ((qh[0] + qh[1]) / f(2)).astype(f)
        # the loss
        w = [h["rho"] ** t for t in range(T)]
        sc = f(scale)
        term = (f(h["entropy_coef"]) * se + q / sc).astype(f)
        sm = term.sum(1, dtype=f) / f(B)
        out["step_means"] = sm.astype(f)
        loss = (-(sm) * np.asarray(w, f)).sum(dtype=f) / f(T)
        out["losses"] = np.asarray([loss, out["entropy"].sum(dtype=f) / f(T * B), se.sum(dtype=f) / f(T * B)], f)
        # the seeds
        gf = f(g)
        cse = gf * np.asarray([f(-h["entropy_coef"] * wt / (T * B)) for wt in w], f)
        cq = gf * np.asarray([f(-wt / (2.0 * T * B)) for wt in w], f)
        out["d_scaled_entropy"] = dse = np.broadcast_to(cse[:, None], (T, B)).astype(f)
        # (the library's backward sums exp and exp * bin in fp64 and rounds x once: pi_grad_kernels.cuh)
        xb = ((e.astype(np.float64) * bins.astype(np.float64)).sum(-1) / e.astype(np.float64).sum(-1)).astype(f)
        ds = np.where(xb != 0, np.exp(np.abs(xb)), f(0)).astype(f)
        c = (cq[None, :, None] / sc * ds).astype(f)
        out["d_q_logits"] = (c[..., None] * (p * (bins - xb[..., None]))).astype(f)
        # the head's backward
        ga = np.zeros_like(a) if x.get("d_action") is None else np.asarray(x["d_action"], f)
        g_S = dse * (-(lp / den))
        g_lp = dse * (-(S * f(1e-8)) / (den * den))
        g_lp0 = (g_lp + g_S * size)[..., None]
        g_K = (-g_lp)[..., None]
        dK = np.where(om > 0, (f(-2) * a) / (om + f(1e-6)), f(0))
        g_a = ga + g_K * dK
        g_u = g_a * om
        g_ls = g_u * (eps * sd) - g_lp0
        out["d_pi_out"] = np.concatenate([g_u * mm, g_ls * mm * (f(0.5) * ldif) * (f(1) - th * th)], -1).astype(f)
    return out


# ---------------------------------------------------------------- torch autograd of the port's own expression (CPU)
def torch_ref(x, case, h, scale, dtype, g=1.0):
    """-> the dict of `closed_form` from torch autograd on the CPU in `dtype` (numpy arrays)."""
    import torch

    from tdmpc2_amd import world_model as wm

    T, B, NB = case["T"], case["B"], case["NB"]
    t = {k: None if x.get(k) is None else torch.tensor(np.asarray(x[k]), dtype=dtype) for k in INPUTS}
    y, ql = t["pi_out"].requires_grad_(True), t["q_logits"].requires_grad_(True)
    m = t["mask"]
    dims = None if m is None else m.sum(-1).unsqueeze(-1)
    tt = lambda v: torch.tensor(v, dtype=dtype)  # noqa: E731
    action, info = wm._pi_tail(y, t["eps"], m, dims, tt(h["log_std_min"]), tt(h["log_std_dif"]))
    cfg = type("Cfg", (), dict(num_bins=NB, vmin=h["vmin"], vmax=h["vmax"]))
    qh = wm.two_hot_inv(ql, cfg)
    q = qh.sum(0) / 2
    se = info["scaled_entropy"].detach().requires_grad_(True)
    qs = q / scale
    rho = torch.tensor([h["rho"] ** i for i in range(T)], dtype=dtype)
    pi_loss = (-(h["entropy_coef"] * se + qs).mean(dim=(1, 2)) * rho).mean()
    (pi_loss * g).backward()
    torch.autograd.backward([action, info["scaled_entropy"]], [t["d_action"], se.grad])
    sm = (h["entropy_coef"] * se + qs).mean(dim=(1, 2))
    n = lambda v: v.detach().numpy().copy()  # noqa: E731
    return dict(action=n(action), entropy=n(info["entropy"])[..., 0], scaled_entropy=n(se)[..., 0], q=n(q)[..., 0],
                losses=np.asarray([float(v.detach()) for v in (pi_loss, info["entropy"].mean(), se.mean())]), step_means=n(sm),
                d_scaled_entropy=n(se.grad)[..., 0], d_q_logits=n(ql.grad), d_pi_out=n(y.grad))


# ---------------------------------------------------------------- tdmpc2_amd/csrc/pi_grad_route.h behind a C shim
SHIM = r"""
#include <string.h>
#include <vector>
#include "pi_grad_route.h"
extern "C" void constants(int32_t *out) {
    const int32_t c[10] = {PG_THREADS, PG_ROWS, PG_HEAD_LANES, PG_HEAD_ROWS, PG_MAXT, PG_MAXA, PG_MAXBINS, PG_KINDS, (int32_t)sizeof(PgDesc),
                           (int32_t)sizeof(PgGrid)};
    memcpy(out, c, sizeof c);
}
extern "C" int check(const PgDesc *d) { return pg_check(*d); }
extern "C" uint64_t head_grid(const PgDesc *d) { return pg_head_grid(*d); }
extern "C" uint64_t value_grid(const PgDesc *d) { return pg_value_grid(*d); }
extern "C" void bwd_grid(const PgDesc *d, int want, uint64_t *out) {
    const PgGrid g = pg_bwd_grid(*d, want);
    memcpy(out, g.first, sizeof g.first);
}
extern "C" int step_of(const PgDesc *d, uint64_t unit) { return pg_step_of(*d, unit); }
extern "C" uint64_t mask_row(const PgDesc *d, uint64_t row) { return pg_mask_row(*d, row); }
extern "C" float bin(const PgDesc *d, int k) { return pg_bin(*d, k); }
extern "C" float rho_pow(const PgDesc *d, int t) { return pg_rho_pow(*d, t); }
extern "C" float coef_q(const PgDesc *d, int t) { return pg_coef_q(*d, t); }
extern "C" float coef_se(const PgDesc *d, int t) { return pg_coef_se(*d, t); }
extern "C" float ordered_sum(const float *src, uint64_t n) { return pg_ordered_sum(src, n); }
extern "C" void loss_serial(const PgDesc *d, const float *q, const float *entropy, const float *se, float scale, float *losses,
                            float *step_means) {
    pg_loss_serial(*d, q, entropy, se, scale, losses, step_means);
}
// Every workgroup of the four row launches walked as the kernels walk them: each element a thread (or wavefront) writes after its
// bounds test adds one to its mark.  Returns the number of marks that are not exactly one (zero where loss_backward's output is
// NULL) and of workgroups decoded outside their kind's range.
extern "C" uint64_t cover(const PgDesc *dp) {
    const PgDesc d = *dp;
    const uint64_t TB = pg_tb(d), A = (uint64_t)d.action_dim;
    uint64_t bad = 0;
    {   // the head kernels: action / d_pi_out columns and the row's entropy pair
        std::vector<uint8_t> col(TB * A, 0), row(TB, 0);
        for (uint64_t b = 0; b < pg_head_grid(d); ++b)
            for (int t = 0; t < PG_THREADS; ++t) {
                const uint64_t r = pg_head_row(b, t);
                if (r >= TB) continue;
                for (int j = pg_head_part(t); j < d.action_dim; j += PG_HEAD_LANES) ++col[r * A + (uint64_t)j];
                if (pg_head_part(t) == 0) ++row[r];
                bad += pg_mask_row(d, r) >= (uint64_t)d.batch;
            }
        for (uint8_t m : col) bad += m != 1;
        for (uint8_t m : row) bad += m != 1;
    }
    {   // value_forward: one wavefront per row pair
        std::vector<uint8_t> row(TB, 0);
        for (uint64_t b = 0; b < pg_value_grid(d); ++b)
            for (int t = 0; t < PG_THREADS; t += 64) {
                const uint64_t r = pg_row(b, t);
                if (r < TB) ++row[r];
            }
        for (uint8_t m : row) bad += m != 1;
    }
    for (int want = 1; want < 4; ++want) {  // loss_backward, every subset of outputs that is not empty
        const PgGrid g = pg_bwd_grid(d, want);
        std::vector<uint8_t> qrow(2 * TB, 0), se(TB, 0);
        for (uint64_t b = 0; b < g.first[PG_KINDS]; ++b) {
            int kind;
            uint64_t local;
            pg_decode(g, b, kind, local);
            if (b < g.first[kind] || b >= g.first[kind + 1]) { ++bad; continue; }
            for (int t = 0; t < PG_THREADS; ++t) {
                if (kind == PG_K_SE) {
                    const uint64_t e = pg_se_elem(local, t);
                    if (e < TB) { ++se[e]; bad += pg_step_of(d, e) >= d.steps; }
                } else if ((t & 63) == 0) {
                    const uint64_t r = pg_row(local, t);
                    if (r < 2 * TB) { ++qrow[r]; bad += pg_step_of(d, r) >= d.steps; }
                }
            }
        }
        for (uint8_t m : qrow) bad += m != ((want & PG_WANT_Q) ? 1 : 0);
        for (uint8_t m : se) bad += m != ((want & PG_WANT_SE) ? 1 : 0);
    }
    return bad;
}
"""
# the same walk as a program of its own (build_walk; with sanitize=True under AddressSanitizer and UBSan): argv[1] names a file of
# int32 words: cases, then per case steps, batch, action_dim, num_bins, multitask
MAIN = r"""
#include <stdio.h>
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t ncases = 0;
    if (fread(&ncases, 4, 1, f) != 1) return 2;
    uint64_t bad = 0;
    for (int32_t k = 0; k < ncases; ++k) {
        int32_t w[5];
        if (fread(w, 4, 5, f) != 5) return 2;
        PgDesc d{w[0], w[1], w[2], w[3], w[4], -10.f, 10.f, 0.5f, 1e-4f, -10.f, 12.f};
        if (pg_check(d) != PG_OK) return 2;
        bad += cover(&d);
        std::vector<float> q(pg_tb(d)), e(pg_tb(d)), s(pg_tb(d)), sm(d.steps);
        for (uint64_t i = 0; i < pg_tb(d); ++i) { q[i] = (float)(i % 7) - 3.f; e[i] = 1.f + (float)(i % 5); s[i] = 0.5f * (float)(i % 3); }
        float losses[3];
        pg_loss_serial(d, q.data(), e.data(), s.data(), 2.f, losses, sm.data());
        bad += !(losses[1] > 0.f);
        printf("case %d: head %llu workgroups, value %llu, backward %llu\n", (int)k, (unsigned long long)pg_head_grid(d),
               (unsigned long long)pg_value_grid(d), (unsigned long long)pg_bwd_grid(d, 3).first[PG_KINDS]);
    }
    fclose(f);
    // offsets past 2^32: the last workgroups of a descriptor with more rows than that
    PgDesc big{16, 1 << 29, 64, 101, 0, -10.f, 10.f, 0.5f, 1e-4f, -10.f, 12.f};
    const uint64_t TB = pg_tb(big);
    bad += TB != (1ull << 33);
    bad += pg_head_row(pg_head_grid(big) - 1, PG_THREADS - 1) != TB - 1;
    bad += pg_row(pg_value_grid(big) - 1, PG_THREADS - 1) != TB - 1;
    const PgGrid g = pg_bwd_grid(big, 3);
    int kind;
    uint64_t local;
    pg_decode(g, g.first[PG_K_SE] - 1, kind, local);
    bad += kind != PG_K_Q || pg_row(local, PG_THREADS - 1) != 2 * TB - 1 || pg_step_of(big, 2 * TB - 1) != 15;
    pg_decode(g, g.first[PG_KINDS] - 1, kind, local);
    bad += kind != PG_K_SE || pg_se_elem(local, PG_THREADS - 1) != TB - 1;
    bad += pg_mask_row(big, TB - 1) != (1ull << 29) - 1;
    printf("bad %llu\n", (unsigned long long)bad);
    return bad ? 1 : 0;
}
"""
CONSTANT_KEYS = ("THREADS", "ROWS", "HEAD_LANES", "HEAD_ROWS", "MAXT", "MAXA", "MAXBINS", "KINDS", "DESC_BYTES", "GRID_BYTES")
ROUTE_SIZES = ((1, 1), (3, 9), (9, 33))  # (T, B): B T of 1, 27, 297


class Desc(ctypes.Structure):  # PgDesc = tdmpc2_pigrad_desc
    _fields_ = [(n, ctypes.c_int32) for n in ("steps", "batch", "action_dim", "num_bins", "multitask")] + \
               [(n, ctypes.c_float) for n in HYPER_KEYS]


def desc_of(case, h=None, **over):
    h = h or hyper()
    d = dict(steps=case["T"], batch=case["B"], action_dim=case["A"], num_bins=case["NB"], multitask=int(case.get("live") is not None))
    d.update({k: h[k] for k in HYPER_KEYS})
    d.update(over)
    return Desc(**d)


def build_route(tmpdir):
    dp, u64, i32, fp = ctypes.POINTER(Desc), ctypes.c_uint64, ctypes.c_int32, ctypes.POINTER(ctypes.c_float)
    return route_shim.build_shim(tmpdir, "pi_grad_route", SHIM, dict(
        constants=[ctypes.POINTER(i32)], check=[dp], head_grid=([dp], u64), value_grid=([dp], u64), bwd_grid=[dp, i32, ctypes.POINTER(u64)],
        step_of=[dp, u64], mask_row=([dp, u64], u64), ordered_sum=([fp, u64], ctypes.c_float),
        loss_serial=[dp, fp, fp, fp, ctypes.c_float, fp, fp], cover=([dp], u64),
        **{name: ([dp, i32], ctypes.c_float) for name in ("bin", "rho_pow", "coef_q", "coef_se")}))


def build_walk(tmpdir, sanitize=False):
    return route_shim.build_walk(tmpdir, "pi_grad_route", SHIM + MAIN, sanitize)


def walk_input(path):
    cs = CASE_LIST + [dict(FIXTURE_CASES[k]) for k in FIXTURE_CASES]
    words = [len(cs)]
    for c in cs:
        words += [c["T"], c["B"], c["A"], c["NB"], int(c.get("live") is not None)]
    with open(path, "wb") as f:
        f.write(np.asarray(words, np.int32).tobytes())
    return path


def loss_model(q, entropy, se, h, scale):
    """pg_loss_serial in numpy fp32 -> (losses [3], step_means [T])."""
    f = np.float32
    q, entropy, se = (np.asarray(v, f) for v in (q, entropy, se))
    T, B = q.shape
    term = (f(h["entropy_coef"]) * se).astype(f) + (q / f(scale)).astype(f)
    sm = np.asarray([ordered_sum_model(term[t]) / f(B) for t in range(T)], f)
    loss = f(0)
    for t in range(T):
        loss = f(loss + f((-sm[t]) * f(h["rho"] ** t)))
    rows = f(f(T) * f(B))
    return np.asarray([loss / f(T), ordered_sum_model(entropy.reshape(-1)) / rows, ordered_sum_model(se.reshape(-1)) / rows], f), sm
