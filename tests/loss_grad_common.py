"""The loss unit (tdmpc2_loss_*, include/tdmpc2_plan.h) restated for the tests:
  - `closed_form`: the four losses of TDMPC2._update, their per-step means and the gradient seeds of the total in numpy, generic in
    the dtype.  float64 is the reference; float32 follows the library's arithmetic (symlog through an fp64 log rounded once, the two
    bins picked by index, per-step constants computed in fp64 and rounded once, g as one fp32 factor) without claiming its bits.
  - `torch_ref`: torch autograd on the CPU of the same expression, written out here (log_softmax against a two-hot row built with
    two indexed assignments, mse, binary_cross_entropy_with_logits, the loops over steps and heads): the yardstick of the measured
    gates in fp32, the reference in fp64.  `th` pins the two-hot rows as constant tensors.
  - the case table shared by the CPU and the GPU tests, the fixture's inputs, and loss_grad_route.h behind a C shim.

Hyperparameters are fp32 in the C ABI.  `hyper` returns the doubles the library computes with (fp32(0.1) = 0.100000001490...): every
reference gets those, so the gates measure arithmetic and not the representation of 0.1 in fp32."""
import ctypes
import os

import numpy as np

from tests import route_shim
from tests.optim_common import FLOOR, MARGIN, rel_err, widen  # noqa: F401  (the measured gate of DESIGN 3.4h)
from tests.route_shim import gate, ordered_sum_model  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "loss_seeds.npz")
HYPER_KEYS = ("vmin", "vmax", "bin_size", "rho", "consistency_coef", "reward_coef", "value_coef", "termination_coef")
SEEDS = ("d_z_pred", "d_reward_logits", "d_q_logits", "d_term_logit")
INPUTS = ("z_pred", "next_z", "reward_logits", "reward", "q_logits", "td_target", "term_logit", "terminated")


def hyper(num_bins, vmin=-10.0, vmax=10.0, rho=0.5, coefs=(20.0, 0.1, 0.1, 1.0)):
    """The reference's defaults (config.yaml:17-21, 41-43), each widened from fp32; bin_size as parser.py:59 forms it."""
    vals = (vmin, vmax, (vmax - vmin) / (num_bins - 1), rho, *coefs)
    return {k: widen(v) for k, v in zip(HYPER_KEYS, vals)}


# ---------------------------------------------------------------- cases (not a cross product)
def _case(name, T, B, L, NB, Q, episodic, scale):
    return dict(name=name, T=T, B=B, L=L, NB=NB, Q=Q, episodic=bool(episodic), scale=float(scale))


CASE_LIST = [
    _case("one", 1, 1, 1, 2, 1, False, 1),
    _case("flag", 3, 33, 63, 101, 5, True, 1),
    _case("deep", 8, 1, 65, 63, 2, False, 8),
    _case("wide", 1, 65, 512, 64, 1, True, 30),
    _case("thin", 3, 33, 1, 65, 2, False, 1),
    _case("bins", 1, 33, 63, 257, 5, True, 8),
    _case("long", 8, 65, 65, 101, 1, False, 30),
    _case("two", 3, 1, 512, 2, 5, True, 1),
    _case("mid", 3, 65, 63, 101, 2, True, 8),
    _case("hot", 1, 33, 65, 63, 5, False, 30),
    _case("tall", 8, 33, 1, 257, 2, True, 1),
    _case("five", 3, 33, 512, 101, 5, False, 8),  # the 5M model's T, L, NB and Q at a small batch
    _case("loud", 3, 33, 63, 101, 5, True, 30),   # "flag" with logits of scale 30
]
CASES = {c["name"]: c for c in CASE_LIST}
FIXTURE_CASE = _case("fixture", 2, 9, 16, 101, 3, True, 4)


def target_edges(h, num_bins):
    """0, +-1e5 (beyond the clamp), 1e-30 (symlog rounds to 0), and bin boundaries +-expm1(k bin_size)."""
    ks = sorted({1, 2, max(1, (num_bins - 1) // 4), max(1, (num_bins - 1) // 2 - 1)})
    edges = [0.0, 1e5, -1e5, 1e-30]
    for k in ks:
        edges += [np.expm1(k * h["bin_size"]), -np.expm1(k * h["bin_size"])]
    return np.asarray(edges, np.float32)


def make_inputs(case, seed=0):
    """fp32 inputs of a case with the edge rows: one-hot logits of +-30, all-equal logits, termination logits 0 and +-100, and the
    target edges in the leading elements of reward and (in reverse order) td_target."""
    T, B, L, NB, Q, s = case["T"], case["B"], case["L"], case["NB"], case["Q"], case["scale"]
    h = hyper(NB)
    rng = np.random.default_rng(1000 + seed)
    n = T * B
    x = dict(z_pred=rng.random((T, B, L)), next_z=rng.random((T, B, L)), reward_logits=s * rng.standard_normal((T, B, NB)),
             q_logits=s * rng.standard_normal((Q, T, B, NB)), reward=np.sinh(rng.uniform(-6, 6, (T, B))),
             td_target=np.sinh(rng.uniform(-9.5, 9.5, (T, B))))
    x = {k: v.astype(np.float32) for k, v in x.items()}
    edges = target_edges(h, NB)
    k = min(n, edges.size)
    x["reward"].reshape(-1)[:k] = edges[:k]
    x["td_target"].reshape(-1)[:k] = edges[::-1][:k]
    for name in ("reward_logits", "q_logits"):
        rows = x[name].reshape(-1, NB)
        rows[0] = -30.0
        rows[0, NB // 3] = 30.0
        if rows.shape[0] > 1:
            rows[-1] = 30.0
            rows[-1, NB - 1] = -30.0
        if rows.shape[0] > 2:
            rows[1] = 1.25
    if case["episodic"]:
        tl = (s * rng.standard_normal((T, B))).astype(np.float32)
        tl.reshape(-1)[:min(n, 3)] = np.asarray([0.0, 100.0, -100.0], np.float32)[:min(n, 3)]
        x["term_logit"] = tl
        x["terminated"] = (rng.random((T, B)) < 0.3).astype(np.float32)
    return x


# ---------------------------------------------------------------- the closed form
def two_hot(target, h, num_bins, f):
    """-> (i0, i1, off, rows [..., num_bins]) of math.two_hot in dtype f; a NaN target gives off = NaN at bins 0 and 1."""
    t = np.asarray(target, f)
    with np.errstate(all="ignore"):
        if f == np.float32:
            m = np.log((np.float32(1) + np.abs(t)).astype(np.float64)).astype(np.float32)
        else:
            m = np.log(1.0 + np.abs(t))
        s = np.where(t > 0, m, np.where(t < 0, -m, t)).astype(f)
        x = np.where(np.isnan(s), s, np.minimum(np.maximum(s, f(h["vmin"])), f(h["vmax"]))).astype(f)
        u = ((x - f(h["vmin"])) / f(h["bin_size"])).astype(f)
        fl = np.floor(u)
        off = (u - fl).astype(f)
        i0 = np.clip(np.where(np.isnan(fl), 0, fl), 0, num_bins - 1).astype(np.int64)
        i1 = (i0 + 1) % num_bins
        rows = np.zeros(t.shape + (num_bins,), f)
        np.put_along_axis(rows, i0[..., None], (f(1) - off)[..., None], -1)
        np.put_along_axis(rows, i1[..., None], off[..., None], -1)
    return i0, i1, off, rows


def _softmax_parts(x, f):
    m = x.max(-1, keepdims=True)
    e = np.exp(x - m).astype(f)
    es = e.sum(-1, keepdims=True, dtype=f)
    return (e / es).astype(f), (m + np.log(es)).astype(f)


def closed_form(x, case, h, f=np.float64, g=1.0, th=None):
    """losses [5], step_means [4, T] and the four seeds in dtype f.  th: dict(reward=[T, B, NB], td_target=[T, B, NB]) of pinned
    two-hot rows (the restatement -(th log_softmax).sum()), else the rows of `two_hot` with the two bins picked by index."""
    T, B, L, NB, Q = case["T"], case["B"], case["L"], case["NB"], case["Q"]
    a = {k: np.asarray(v, f) for k, v in x.items()}
    w = [h["rho"] ** t for t in range(T)]
    out = {}
    with np.errstate(all="ignore"):
        d = a["z_pred"] - a["next_z"]
        cons_t = (d * d).sum((1, 2), dtype=f) / f(B * L)

        def head(logits, target, key):
            p, lse = _softmax_parts(logits, f)
            if th is not None:
                rows = np.asarray(th[key], f)
                rows = np.broadcast_to(rows, logits.shape)
                ce = -(rows * (logits - lse)).sum(-1, dtype=f)
                S = rows.sum(-1, dtype=f)
            else:
                i0, i1, off, rows = two_hot(target, h, NB, f)
                i0, i1, off, rows = (np.broadcast_to(v, logits.shape[:-1] + v.shape[target.ndim:]) for v in (i0, i1, off, rows))
                l0 = np.take_along_axis(logits, i0[..., None], -1)[..., 0] - lse[..., 0]
                l1 = np.take_along_axis(logits, i1[..., None], -1)[..., 0] - lse[..., 0]
                ce = -((f(1) - off) * l0 + off * l1)
                S = (f(1) - off) + off
            return ce.astype(f), (p * S[..., None] - rows).astype(f)

        ce_r, seed_r = head(a["reward_logits"], a["reward"], "reward")
        ce_q, seed_q = head(a["q_logits"], a["td_target"], "td_target")
        rew_t = ce_r.sum(1, dtype=f) / f(B)
        val_t = (ce_q.sum(2, dtype=f) / f(B)).sum(0, dtype=f)  # over the heads
        if case["episodic"]:
            xl, y = a["term_logit"], a["terminated"]
            bce = np.maximum(xl, 0) - xl * y + np.log1p(np.exp(-np.abs(xl)))
            term_t = bce.sum(1, dtype=f) / f(B)
            sig = f(1) / (f(1) + np.exp(-xl))
        else:
            term_t = np.zeros(T, f)
        wf = np.asarray(w, f)
        cons = (cons_t * wf).sum(dtype=f) / f(T)
        rew = (rew_t * wf).sum(dtype=f) / f(T)
        val = (val_t * wf).sum(dtype=f) / f(T * Q)
        term = term_t.sum(dtype=f) / f(T)
        total = f(h["consistency_coef"]) * cons + f(h["reward_coef"]) * rew + f(h["termination_coef"]) * term + f(h["value_coef"]) * val
        out["losses"] = np.asarray([cons, rew, val, term, total], f)
        out["step_means"] = np.stack([cons_t, rew_t, val_t / f(Q), term_t]).astype(f)
        gf = f(g)
        cz = gf * np.asarray([f(h["consistency_coef"] * 2.0 * wt / (T * B * L)) for wt in w], f)
        cr = gf * np.asarray([f(h["reward_coef"] * wt / (T * B)) for wt in w], f)
        cq = gf * np.asarray([f(h["value_coef"] * wt / (T * Q * B)) for wt in w], f)
        out["d_z_pred"] = (cz[:, None, None] * d).astype(f)
        out["d_reward_logits"] = (cr[:, None, None] * seed_r).astype(f)
        out["d_q_logits"] = (cq[None, :, None, None] * seed_q).astype(f)
        if case["episodic"]:
            out["d_term_logit"] = ((gf * f(h["termination_coef"] / (T * B))) * (sig - y)).astype(f)
    return out


def pinned_rows(x, case, h):
    """The fp32 two-hot rows both sides of the pinned-target gate are given."""
    return dict(reward=two_hot(x["reward"], h, case["NB"], np.float32)[3], td_target=two_hot(x["td_target"], h, case["NB"], np.float32)[3])


# ---------------------------------------------------------------- torch autograd of the same expression (CPU)
def torch_two_hot(t, h, num_bins):
    import torch

    s = torch.sign(t) * torch.log(1 + torch.abs(t))
    s = torch.clamp(s, h["vmin"], h["vmax"]).reshape(-1)
    u = (s - h["vmin"]) / h["bin_size"]
    idx = torch.floor(u)
    off = u - idx
    idx = idx.long()
    rows = torch.zeros(s.shape[0], num_bins, dtype=t.dtype, device=t.device)
    ar = torch.arange(s.shape[0], device=t.device)
    rows[ar, idx] = 1 - off
    rows[ar, (idx + 1) % num_bins] = off
    return rows


def torch_total(z_pred, next_z, reward_logits, reward, q_logits, td_target, term_logit, terminated, case, h, th=None):
    """The loss expression of TDMPC2._update on torch tensors of one dtype -> (losses [5], step_means [4][T] as python lists)."""
    import torch
    import torch.nn.functional as F

    T, NB, Q = case["T"], case["NB"], case["Q"]

    def soft_ce(logits, target, rows):
        rows = torch_two_hot(target, h, NB) if rows is None else rows
        return -(rows * F.log_softmax(logits, dim=-1)).sum(-1, keepdim=True)

    cons = rew = val = 0
    steps = [[], [], [], []]
    for t in range(T):
        wt = h["rho"] ** t
        c_t = F.mse_loss(z_pred[t], next_z[t])
        r_t = soft_ce(reward_logits[t], reward[t], None if th is None else th["reward"][t]).mean()
        cons, rew = cons + c_t * wt, rew + r_t * wt
        v_t = 0
        for q in range(Q):
            v_q = soft_ce(q_logits[q, t], td_target[t], None if th is None else th["td_target"][t]).mean()
            val, v_t = val + v_q * wt, v_t + v_q
        steps[0].append(c_t)
        steps[1].append(r_t)
        steps[2].append(v_t / Q)
    cons, rew, val = cons / T, rew / T, val / (T * Q)
    if case["episodic"]:
        term = F.binary_cross_entropy_with_logits(term_logit, terminated)
        steps[3] = [F.binary_cross_entropy_with_logits(term_logit[t], terminated[t]) for t in range(T)]
    else:
        term = torch.zeros((), dtype=z_pred.dtype, device=z_pred.device)
        steps[3] = [term] * T
    total = h["consistency_coef"] * cons + h["reward_coef"] * rew + h["termination_coef"] * term + h["value_coef"] * val
    return [cons, rew, val, term, total], steps


def torch_ref(x, case, h, dtype, th=None):
    """-> the dict of `closed_form` from torch autograd on the CPU in `dtype` (numpy arrays)."""
    import torch

    t = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in x.items()}
    leaves = ["z_pred", "reward_logits", "q_logits"] + (["term_logit"] if case["episodic"] else [])
    for k in leaves:
        t[k].requires_grad_(True)
    tht = None if th is None else {k: torch.tensor(v, dtype=dtype) for k, v in th.items()}
    losses, steps = torch_total(t["z_pred"], t["next_z"], t["reward_logits"], t["reward"], t["q_logits"], t["td_target"],
                                t.get("term_logit"), t.get("terminated"), case, h, tht)
    losses[4].backward()
    out = dict(losses=np.asarray([float(v.detach()) for v in losses]),
               step_means=np.asarray([[float(v.detach()) for v in row] for row in steps]))
    for k in leaves:
        out["d_" + k] = t[k].grad.numpy().copy()
    return out


# ---------------------------------------------------------------- tdmpc2_amd/csrc/loss_grad_route.h behind a C shim
SHIM = r"""
#include <string.h>
#include <vector>
#include "loss_grad_route.h"
extern "C" void constants(int32_t *out) {
    const int32_t c[12] = {LS_THREADS, LS_WAVES, LS_ROWS, LS_ELEMS, LS_MAXT, LS_CONS, LS_REW, LS_TERM, LS_Q0, LS_KINDS, (int32_t)sizeof(LsDesc),
                           (int32_t)sizeof(LsGrid)};
    memcpy(out, c, sizeof c);
}
extern "C" int check(const LsDesc *d) { return ls_check(*d); }
extern "C" uint64_t ws_floats(const LsDesc *d) { return ls_ws_floats(*d); }
extern "C" uint64_t ws_index(const LsDesc *d, int slot, uint64_t row) { return ls_ws_index(*d, slot, row); }
extern "C" void grid(const LsDesc *d, int backward, int want, uint64_t *out) {
    const LsGrid g = ls_grid(*d, backward != 0, want);
    memcpy(out, g.first, sizeof g.first);
}
extern "C" void decode(const LsDesc *d, int backward, int want, uint64_t block, int32_t *kind, uint64_t *local) {
    const LsGrid g = ls_grid(*d, backward != 0, want);
    int k;
    ls_decode(g, block, k, *local);
    *kind = k;
}
extern "C" void unit_info(const LsDesc *d, int kind, int backward, uint64_t unit, int32_t *step, uint64_t *target) {
    *step = ls_step_of(*d, kind, backward != 0, unit);
    *target = ls_target_of(*d, unit);
}
extern "C" float coef(const LsDesc *d, int kind, int t) { return ls_coef(*d, kind, t); }
extern "C" float rho_pow(const LsDesc *d, int t) { return ls_rho_pow(*d, t); }
extern "C" float ordered_sum(const float *src, uint64_t n) { return ls_ordered_sum(src, n); }
extern "C" uint64_t elem(uint64_t local, int thread, int j) { return ls_elem(local, thread, j); }
// Every workgroup of a launch walked as the kernels walk it: each unit a thread (or wavefront) passes the bounds test with adds one
// to its mark, each forward unit also to the workspace float it writes.  Returns the number of units outside their kind's range,
// marks that are not exactly one where the kind takes part (zero where it does not) and workspace floats written twice.
extern "C" uint64_t cover(const LsDesc *dp, int backward, int want) {
    const LsDesc d = *dp;
    const bool bw = backward != 0;
    const LsGrid g = ls_grid(d, bw, want);
    uint64_t bad = 0;
    std::vector<std::vector<uint8_t>> marks(LS_KINDS);
    for (int k = 0; k < LS_KINDS; ++k) marks[k].assign(ls_units(d, k, bw), 0);
    std::vector<uint8_t> ws(ls_ws_floats(d), 0);
    for (uint64_t b = 0; b < g.first[LS_KINDS]; ++b) {
        int kind;
        uint64_t local;
        ls_decode(g, b, kind, local);
        if (b < g.first[kind] || b >= g.first[kind + 1]) { ++bad; continue; }
        const uint64_t n = ls_units(d, kind, bw);
        for (int t = 0; t < LS_THREADS; ++t) {
            if (kind == LS_K_CONS && bw) {
                for (int j = 0; j < LS_ELEMS / LS_THREADS; ++j) {
                    const uint64_t e = ls_elem(local, t, j);
                    if (e < n) ++marks[kind][e];
                }
            } else if (kind == LS_K_TERM) {
                const uint64_t e = ls_term_elem(local, t);
                if (e < n) {
                    ++marks[kind][e];
                    if (!bw) ++ws[ls_ws_index(d, LS_TERM, e)];
                }
            } else if ((t & 63) == 0) {  // one wavefront per row
                const uint64_t r = ls_row(local, t);
                if (r < n) {
                    ++marks[kind][r];
                    if (!bw) ++ws[ls_ws_index(d, kind == LS_K_CONS ? LS_CONS : (kind == LS_K_REW ? LS_REW : LS_Q0), r)];
                }
            }
        }
    }
    for (int k = 0; k < LS_KINDS; ++k) {
        const uint8_t expect = (!bw || ((want >> k) & 1)) ? 1 : 0;
        for (uint8_t m : marks[k]) bad += m != expect;
    }
    if (!bw) {
        const uint64_t tb = ls_tb(d);
        for (uint64_t i = 0; i < ws.size(); ++i) {
            const bool term_slot = i / tb == (uint64_t)LS_TERM;
            bad += ws[i] != ((term_slot && !d.episodic) ? 0 : 1);
        }
    }
    return bad;
}
"""
# the same walk as a program of its own (build_walk; with sanitize=True under AddressSanitizer and UBSan): argv[1] names a file of
# int32 words: cases, then per case steps, batch, latent_dim, num_q, num_bins, episodic
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
        int32_t w[6];
        if (fread(w, 4, 6, f) != 6) return 2;
        LsDesc d{w[0], w[1], w[2], w[3], w[4], w[5], -10.f, 10.f, 20.f / (float)(w[4] - 1), 0.5f, 20.f, 0.1f, 0.1f, 1.f};
        if (ls_check(d) != LS_OK) return 2;
        bad += cover(&d, 0, 0);
        for (int want = 1; want < 16; ++want)
            if (d.episodic || !(want & LS_WANT_TERM)) bad += cover(&d, 1, want);
        printf("case %d: ws %llu floats, forward %llu workgroups, backward %llu\n", (int)k, (unsigned long long)ls_ws_floats(d),
               (unsigned long long)ls_grid(d, false, 0).first[LS_KINDS], (unsigned long long)ls_grid(d, true, 15).first[LS_KINDS]);
    }
    fclose(f);
    // offsets past 2^32: the last workgroups of a descriptor whose tensors are longer than that
    LsDesc big{8, 1 << 24, 512, 5, 101, 1, -10.f, 10.f, 0.2f, 0.5f, 20.f, 0.1f, 0.1f, 1.f};
    const LsGrid g = ls_grid(big, true, 15);
    const uint64_t n = ls_units(big, LS_K_CONS, true);
    int kind;
    uint64_t local;
    ls_decode(g, g.first[LS_K_REW] - 1, kind, local);
    bad += kind != LS_K_CONS || ls_elem(local, 255, 3) != n - 1 || n != (1ull << 36);
    bad += ls_step_of(big, LS_K_CONS, true, n - 1) != 7;
    ls_decode(g, g.first[LS_KINDS] - 1, kind, local);
    bad += kind != LS_K_TERM || ls_term_elem(local, 255) != ls_tb(big) - 1;
    bad += ls_ws_index(big, LS_Q0 + 4, ls_tb(big) - 1) != ls_ws_floats(big) - 1;
    printf("bad %llu\n", (unsigned long long)bad);
    return bad ? 1 : 0;
}
"""
CONSTANT_KEYS = ("THREADS", "WAVES", "ROWS", "ELEMS", "MAXT", "CONS", "REW", "TERM", "Q0", "KINDS", "DESC_BYTES", "GRID_BYTES")


class Desc(ctypes.Structure):  # LsDesc = tdmpc2_loss_desc
    _fields_ = [(n, ctypes.c_int32) for n in ("steps", "batch", "latent_dim", "num_q", "num_bins", "episodic")] + \
               [(n, ctypes.c_float) for n in HYPER_KEYS]


def desc_of(case, h=None, **over):
    h = h or hyper(case["NB"])
    d = dict(steps=case["T"], batch=case["B"], latent_dim=case["L"], num_q=case["Q"], num_bins=case["NB"], episodic=int(case["episodic"]))
    d.update({k: h[k] for k in HYPER_KEYS})
    d.update(over)
    return Desc(**d)


def build_route(tmpdir):
    dp, u64, i32 = ctypes.POINTER(Desc), ctypes.c_uint64, ctypes.c_int32
    return route_shim.build_shim(tmpdir, "loss_grad_route", SHIM, dict(
        constants=[ctypes.POINTER(i32)], check=[dp], ws_floats=([dp], u64), ws_index=([dp, i32, u64], u64),
        grid=[dp, i32, i32, ctypes.POINTER(u64)], decode=[dp, i32, i32, u64, ctypes.POINTER(i32), ctypes.POINTER(u64)],
        unit_info=[dp, i32, i32, u64, ctypes.POINTER(i32), ctypes.POINTER(u64)], coef=([dp, i32, i32], ctypes.c_float),
        rho_pow=([dp, i32], ctypes.c_float), ordered_sum=([ctypes.POINTER(ctypes.c_float), u64], ctypes.c_float),
        elem=([u64, i32, i32], u64), cover=([dp, i32, i32], u64)))


def build_walk(tmpdir, sanitize=False):
    return route_shim.build_walk(tmpdir, "loss_grad_route", SHIM + MAIN, sanitize)


def walk_input(path):
    words = [len(CASE_LIST) + 1]
    for c in CASE_LIST + [FIXTURE_CASE]:
        words += [c["T"], c["B"], c["L"], c["Q"], c["NB"], int(c["episodic"])]
    with open(path, "wb") as f:
        f.write(np.asarray(words, np.int32).tobytes())
    return path
