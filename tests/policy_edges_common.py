"""Shared by tests/test_policy_edges.py (CPU) and tests/test_gpu_policy_edges.py (-m gpu): the policy prior's edge cases
(tdmpc2_plan_pi: policy_kernels.cuh, policy_route.h, launch_pi), their fp64 reference, the measured gate and a numpy emulation of
the kernels' summation order.

A case is (L, T, M, A, n, max_envs, kind) with seeded `_pi.*` weights, z (a SimNorm output: softmax over groups of 8), eps, and for
T > 0 per-row tasks whose masks differ (column 0 always live; the saturated probe's all-zero row is the one exception).
Reference: `ref64` = tests/policy_common.fp64_pi in float64, `ref32` = the same formula in torch float32 on the CPU.
Gate, per case and output (action, mean, log_std, entropy, scaled_entropy):
    max|HIP - ref64| <= 4 max(max|ref32 - ref64|, 2^-23 max(1, max|ref64|))
(encoder_common.FACTOR / FLOOR; the floor scales with magnitude because log_std reaches -10 and the entropies
thousands).  `ref32`'s matrix products are the CPU BLAS's, whose blocking differs between machines: the same emulation output
stood at 0.47 of the gate on one CPU and at 0.71 on another (s_32_4096_A17, `mean` on the row route, whose four chains of 1024
terms are the longest sums here).  Every gated case has at least 512 elements of action, so the row counts of the shape table are raised where A is
small, keeping the edge each shape is there for: the handle's max_envs is chosen so that the spread route's LAST chunk has the row
count the table names (n = 16 q + 9, 16 + 3, 16 + 7, 16 + 2, 6 x 16 + 5; n = 512 rows at A = 1).  The multitask row family
(32, 1, 96, 5) is ONE case of 257 rows and max_envs = 16: its reference and gate are computed once on all 257 rows (1285 elements)
and the calls with n = 1, 2, 9, 19, 49 run prefixes of those rows against the same reference rows and the same gate (`ROWS`).
Value probes (`head_*`: A = 64, M = 32, `_pi.2.weight` = 0 and `_pi.2.bias` = the chosen pre-activations on a 1/16 grid, so the
head's inputs are exact in any summation order on both routes; rows differ by eps and mask):
  head_inside     |mean + eps exp(log_std)| <= 3; log_std pre-activations sweep [-40, 40]; two rows of eps = 0 (action bits = mean
                  bits).  The eps rows are 0, +-1 and mixed TIMES a per-lane power of two s_j <= 1 with exp(log_std_j) s_j <= 1:
                  with the squash's upper end reached (exp(2) = 7.4) no lane can hold |mean +- exp(log_std)| <= 3 at eps = +-1 and
                  at eps = 0 at once, so the lanes of large log_std take eps = +-1/8 (re-chosen input, not a wider gate).
  head_saturated  every live |mean + eps exp(log_std)| >= 20 (tanh = +-1 exactly in fp32 and fp64, the squash term is log(1e-6) in
                  both), |eps| = 30 among the rows, multitask with mask rows all ones / lane 0 / alternating / first 63 / all zeros.
  head_band       values in (3, 20), where log(relu(1 - a^2) + 1e-6) amplifies one ulp of tanhf: gated per value in
                  policy_common.entropy_bound's form, the only case gated that way.
Every probe row keeps |log_prob| >= 1 (lp + 1e-8 never near zero).

`emulate` follows the published order.  Row route: encoder_common's narrow chains (four chains over k % 4, tail on chain 0,
((a0 + a1) + (a2 + a3)) + bias) and block sums.  k_pol_gemv: eight waves take shares of ceil(in / 8), two chains a / b over even
and odd k of the share, the single tail on a, a wave's partial a + b, the partials added in wave order, then the bias; k_enc_norm
as in encoder_common.  Head: every __f*_rn operation rounded separately, the xor butterfly 32..1 over the 64 lanes.  fp32, not
claimed bit-exact (libm's tanhf / expf / logf, the compiler's contraction choices)."""
import dataclasses
from typing import Optional

import numpy as np
import torch

from tdmpc2_amd import synth
from tdmpc2_amd.config import named_config
from tests import encoder_common as ec
from tests import policy_common as pc

FACTOR, FLOOR, MIN_ELEMENTS, N_TASKS = ec.FACTOR, ec.FLOOR, ec.MIN_ELEMENTS, ec.N_TASKS
POL_MAX_WIDTH, POL_THREADS, POL_GEMV_WAVES, POL_ROW_MAX_MLP, POL_ROW_MAX_ROWS = 4096, 512, 8, 1024, 256
OUTPUTS = ("action", "mean", "log_std", "entropy", "scaled_entropy")
f32, f64 = np.float32, np.float64


@dataclasses.dataclass
class Case:
    name: str
    L: int
    T: int
    M: int
    A: int
    n: int
    max_envs: int
    kind: str = "shape"          # shape | head_inside | head_saturated | head_band
    big: bool = False            # hundreds of MB on the device: one such handle at a time
    cfg: object = None
    sd: dict = None
    z: np.ndarray = None
    eps: np.ndarray = None
    tasks: Optional[np.ndarray] = None

    @property
    def in0(self):
        return self.L + self.T

    @property
    def emb(self):
        return None if self.tasks is None else pc.task_rows(self.sd, self.tasks)[0]

    @property
    def mask(self):
        return None if self.tasks is None else pc.task_rows(self.sd, self.tasks)[1]

    def chunks(self, n=None):
        """rows of the spread route's chunks for a call of n rows (launch_pi)"""
        n = self.n if n is None else n
        return [min(self.max_envs, n - r0) for r0 in range(0, n, self.max_envs)]


def make_cfg(L, T, M, A):
    cfg = named_config("small", task="mt30" if T else "walker-run", latent_dim=L, mlp_dim=M, action_dim=A)
    cfg.task_dim = T
    return cfg


def specs():
    """Every case, unfilled: (name, L, T, M, A, n, max_envs).  Row counts: module docstring."""
    C = Case
    return [
        C("s_32_32_A1", 32, 0, 32, 1, 512, 16),              # 2A = 2 columns, one live head lane; both routes chunk / take any n
        C("s_32_32_A64", 32, 0, 32, 64, 8, 8),               # 2A = 128 > M: the head sets the y row and maxw; full wave
        C("mt_33_96_A5", 32, 1, 96, 5, 257, 16),             # in0 = 33, M = 96; run at n in ROWS
        C("mt_67_544_A63", 64, 3, 544, 63, 19, 16),          # in0 = 67, kq = 68, two features per thread; last chunk 3 rows: R = 4
        C("mt_101_480_A33", 96, 5, 480, 33, 23, 16),         # in0 = 101 (kq = 13), idle threads in the block sums, 2A = 66
        C("s_32_512_A64", 32, 0, 512, 64, 18, 16),           # one feature per thread exactly; last chunk 2 rows: R = 2
        C("mt_128_1056_A6", 32, 96, 1056, 6, 101, 16),       # auto -> spread by width; forced row: three features per thread
        C("s_32_4096_A17", 32, 0, 4096, 17, 32, 8, big=True),    # POL_MAX_WIDTH: eight features per thread, R = 8 LDS at its largest
        C("s_4096_32_A2", 4096, 0, 32, 2, 256, 8, big=True),     # in0 at POL_MAX_WIDTH
        C("head_inside", 32, 0, 32, 64, 8, 8, kind="head_inside"),
        C("head_saturated", 32, 1, 32, 64, 10, 8, kind="head_saturated"),
        C("head_band", 32, 0, 32, 64, 8, 8, kind="head_band"),
    ]


ROW_FAMILY = "mt_33_96_A5"
ROWS = (1, 2, 9, 19, 49, 105, 257)   # calls on prefixes of the row family; 105 = 6 x 16 + 9, 257 leaves the row route on auto
REFUSED_BIND = (4096, 1)             # in0 = 4097: tdmpc2_plan_bind_policy -> TDMPC2_ERR_UNSUPPORTED
NAMES = [c.name for c in specs()]
SHAPE_NAMES = [c.name for c in specs() if c.kind == "shape"]
PROBE_NAMES = [c.name for c in specs() if c.kind != "shape"]


def runs():
    """(case name, rows of the call) of every gated GPU run"""
    return [(n, r) for n in NAMES for r in (ROWS if n == ROW_FAMILY else (case_spec(n).n,))]


def case_spec(name):
    return next(c for c in specs() if c.name == name)


def _grid16(a):
    return (np.round(np.asarray(a, f64) * 16) / 16).astype(f32)


def _fill(c: Case, seed):
    rng = np.random.default_rng(seed)
    c.cfg = make_cfg(c.L, c.T, c.M, c.A)
    sd, fin = {}, c.in0
    for l, out in enumerate((c.M, c.M, 2 * c.A)):
        # the output layer's spread is set by its fan-in so that the head sees O(1) pre-activations at every width (a 4096-wide
        # trunk under a fixed 0.1 would saturate every tanh and leave log(relu(1 - a^2) + 1e-6) ill-conditioned everywhere)
        w_std = 0.3 if l == 0 else 0.1 if l == 1 else 0.3 / np.sqrt(fin)
        sd[f"_pi.{l}.weight"], sd[f"_pi.{l}.bias"] = synth._linear(rng, out, fin, w_std=w_std)
        if l < 2:
            sd[f"_pi.{l}.ln.weight"], sd[f"_pi.{l}.ln.bias"] = synth._ln(rng, out)
        fin = out
    sd["_pi.2.bias"][c.A:] += f32(0.25)   # log_std around -2.5: eps moves the action by tenths, |mean + eps exp(log_std)| stays below 3
    c.z = synth.simnorm_np(rng.standard_normal((c.n, c.L)).astype(f32), 8)
    c.eps = rng.standard_normal((c.n, c.A)).astype(f32)
    if c.T:
        tab = rng.standard_normal((N_TASKS, c.T))
        # rows of norm 0.3 .. 0.9 on a 2^-10 grid: nn.Embedding(max_norm=1) leaves them alone in every precision
        tab = tab / np.linalg.norm(tab, axis=-1, keepdims=True) * rng.uniform(0.3, 0.9, (N_TASKS, 1))
        sd["_task_emb.weight"] = (np.round(tab * 1024) / 1024).astype(f32)
        assert (np.linalg.norm(sd["_task_emb.weight"].astype(f64), axis=-1) < 1.0).all()
        sd["_action_masks"] = (rng.random((N_TASKS, c.A)) < 0.7).astype(f32)
        sd["_action_masks"][:, 0] = 1.0
        c.tasks = ((np.arange(c.n) * 7 + 2) % N_TASKS).astype(np.int64)
    c.sd = sd
    if c.kind != "shape":
        _pin(c, rng)
    return c


def probe_pre(c: Case):
    """(mean, log_std) pre-activations [A] of a value probe = the two halves of `_pi.2.bias`"""
    b = np.asarray(c.sd["_pi.2.bias"], f64)
    return b[:c.A], b[c.A:]


def _pin(c: Case, rng):
    """Value probes: the output layer is its bias alone; every row sees the same pre-activations and differs by eps and mask."""
    A, n, sd = c.A, c.n, c.sd
    assert A == 64 and c.M == 32
    sd["_pi.2.weight"] = np.zeros((2 * A, c.M), f32)
    lane = np.arange(A)
    sign = np.where(lane % 2 == 0, 1.0, -1.0)
    ends = np.asarray([-40.0, -20.0, -10.0, -5.0, 5.0, 10.0, 20.0, 40.0])
    if c.kind == "head_inside":
        mu = _grid16(rng.uniform(-2.0, 2.0, A))
        lr = _grid16(np.concatenate([ends, np.linspace(-3.0, 3.0, A - len(ends))]))
        lr = lr[rng.permutation(A)]
        sigma = np.exp(-10.0 + 6.0 * (np.tanh(lr.astype(f64)) + 1.0))
        s = np.where(sigma <= 1.0, 1.0, 0.125)          # exp(2) / 8 < 1
        assert (sigma * s <= 1.0).all()
        pat = np.zeros((n, A))
        pat[1], pat[2], pat[3] = 1.0, -1.0, sign         # rows 0 and 4: eps = 0
        pat[5] = -sign
        pat[6:] = rng.integers(-2, 3, (n - 6, A)) / 2.0   # mixed: 0, +-1/2, +-1
        c.eps = (pat * s).astype(f32)
    elif c.kind == "head_saturated":
        mu = _grid16(sign * rng.uniform(21.0, 40.0, A))
        lr = _grid16(np.concatenate([ends, np.linspace(-3.0, 3.0, A - len(ends))]))
        lr = lr[rng.permutation(A)]
        mag = np.zeros((n, A))
        mag[0], mag[1], mag[2] = 0.0, 1.0, 30.0
        mag[3:] = rng.choice([0.0, 0.5, 1.0, 3.0, 30.0], (n - 3, A))
        # eps pushes the way of the mean: |mean + eps exp(log_std)| >= |mean| >= 21; where exp(log_std) is tiny (30 exp < 1)
        # the sign is free
        free = lr <= -2.0
        sg = np.where(free[None] & (rng.random((n, A)) < 0.5), -1.0, 1.0) * np.sign(mu)[None]
        c.eps = (mag * sg).astype(f32)
        masks = (rng.random((N_TASKS, A)) < 0.7).astype(f32)
        masks[:, 0] = 1.0
        masks[0] = 1.0                                  # all ones
        masks[1] = 0.0
        masks[1, 0] = 1.0                               # lane 0 only
        masks[2] = (lane % 2 == 0)                      # alternating
        masks[3] = (lane < 63)                          # the first 63 lanes
        masks[4] = 0.0                                  # none: size = 0
        sd["_action_masks"] = masks
        c.tasks = (np.arange(n) % 5).astype(np.int64)   # every pattern twice, with different eps
    elif c.kind == "head_band":
        mu = _grid16(sign * np.linspace(4.5, 18.0, A)[rng.permutation(A)])
        lr = _grid16(np.concatenate([[-40.0, -20.0, -10.0, -5.0], np.linspace(-3.0, 0.5, A - 4)]))
        lr = lr[rng.permutation(A)]                      # exp(log_std) <= 0.31
        c.eps = _grid16(rng.uniform(-3.5, 3.5, (n, A)))
        c.eps[0] = 0.0
    else:
        raise KeyError(c.kind)
    sd["_pi.2.bias"] = np.concatenate([mu, lr]).astype(f32)


_built, _refs = {}, {}


def case(name) -> Case:
    if name not in _built:
        i = NAMES.index(name)
        c = _fill(specs()[i], seed=300 + i)
        assert c.n * c.A >= MIN_ELEMENTS and c.L % 32 == 0 and c.M % 32 == 0 and 1 <= c.A <= 64
        _built[name] = c
    return _built[name]


# ---------------------------------------------------------------------------------------------------------- references
def refs(c: Case):
    """(ref64, ref32, gate): dicts over OUTPUTS, computed once per case and left unchanged."""
    if c.name not in _refs:
        a = pc.fp64_pi(c.cfg, c.sd, c.z, c.tasks, c.eps)
        b = pc.fp64_pi(c.cfg, c.sd, c.z, c.tasks, c.eps, dtype=torch.float32)
        for v in list(a.values()) + list(b.values()):
            v.setflags(write=False)
        _refs[c.name] = (a, b, {k: gate(a[k], b[k]) for k in OUTPUTS})
    return _refs[c.name]


def ref_err(a64, b32):
    a64 = np.asarray(a64, f64)
    return max(float(np.abs(np.asarray(b32, f64) - a64).max()), FLOOR * max(1.0, float(np.abs(a64).max())))


def gate(a64, b32):
    return FACTOR * ref_err(a64, b32)


def band_bound(c: Case, key, rows=slice(None)):
    """head_band's per-value gate, policy_common.entropy_bound's form: max(1e-5 max(1, |v64|), 2 |ref32 - v64|)"""
    a, b, _ = refs(c)
    return pc.entropy_bound({key: a[key][rows]}, {key: b[key][rows]}, key).reshape(a[key][rows].shape)


def ratios(c: Case, got, rows=None):
    """{output: worst err / gate} of `got` (dict over OUTPUTS on the first `rows` rows); head_band: worst err / per-value bound."""
    r = slice(0, c.n if rows is None else rows)
    a, _, g = refs(c)
    out = {}
    for k in OUTPUTS:
        err = np.abs(np.asarray(got[k], f64).reshape(a[k][r].shape) - a[k][r])
        out[k] = float((err / band_bound(c, k, r)).max()) if c.kind == "head_band" else float(err.max() / g[k])
    return out


# ---------------------------------------------------------------------------------------------------------- order emulation
def _wave_sum(v):
    """[n, <= 64] -> [n]: idle lanes add 0, xor butterfly 32..1"""
    w = np.zeros((v.shape[0], 64), f32)
    w[:, :v.shape[1]] = v
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    return w[:, 0]


def _gemv(x, wt, bias):
    """k_pol_gemv: x [n, in], wt [in, out]"""
    fin = wt.shape[0]
    kq = (fin + POL_GEMV_WAVES - 1) // POL_GEMV_WAVES
    s = np.zeros((x.shape[0], wt.shape[1]), f32)
    for w in range(POL_GEMV_WAVES):
        k0 = min(fin, w * kq)
        k1 = min(fin, k0 + kq)
        a = np.zeros_like(s)
        b = np.zeros_like(s)
        k = k0
        while k + 2 <= k1:
            a = ec._fma(x[:, k, None], wt[None, k], a)
            b = ec._fma(x[:, k + 1, None], wt[None, k + 1], b)
            k += 2
        if k < k1:
            a = ec._fma(x[:, k, None], wt[None, k], a)
        s = s + (a + b)
    return s + bias


def head(y, A, eps, mask, lmin, ldif):
    """pol_head on pre-activations y [n, 2A] in fp32, one rounding per operation -> dict over OUTPUTS"""
    r = ec._r
    y, eps = np.asarray(y, f32), np.asarray(eps, f32)
    mu, lr = y[:, :A], y[:, A:]
    ls = f32(lmin) + (f32(0.5) * f32(ldif)) * (r(np.tanh(lr.astype(f64))) + f32(1.0))
    size = np.full(y.shape[0], f32(A))
    if mask is not None:
        m = np.asarray(mask, f32)
        mu, ls, eps = mu * m, ls * m, eps * m
        size = _wave_sum(m)
    res = f32(-0.5) * (eps * eps) - ls
    lp = _wave_sum(res - f32(0.9189385175704956))
    slp = lp * size
    act = r(np.tanh((mu + eps * r(np.exp(ls.astype(f64)))).astype(f64)))
    mt = r(np.tanh(mu.astype(f64)))
    sq = r(np.log((np.maximum(f32(1.0) - act * act, f32(0.0)) + f32(1e-6)).astype(f64)))
    lp = lp - _wave_sum(sq)
    with np.errstate(divide="ignore", invalid="ignore"):
        se = (-lp) * (slp / (lp + f32(1e-8)))
    return {"action": act, "mean": mt, "log_std": ls, "entropy": (-lp)[:, None], "scaled_entropy": se[:, None]}


def emulate(c: Case, route, rows=None):
    """dict over OUTPUTS, fp32, in the kernels' summation order on `route` ("row": k_pol_row; "spread": k_pol_gemv + k_enc_norm + k_pol_head)."""
    n = c.n if rows is None else rows
    x = c.z[:n] if c.tasks is None else np.concatenate([c.z[:n], c.emb[:n]], -1)
    x = np.ascontiguousarray(x, f32)
    for l in range(3):
        p = f"_pi.{l}."
        wt = np.ascontiguousarray(np.asarray(c.sd[p + "weight"], f32).T)
        bias = np.asarray(c.sd[p + "bias"], f32)[None]
        y = ec._chains(x, wt, 0, wt.shape[0]) + bias if route == "row" else _gemv(x, wt, bias)
        if l < 2:
            x = ec._norm_act(y, np.asarray(c.sd[p + "ln.weight"], f32), np.asarray(c.sd[p + "ln.bias"], f32), False, 8)
    mask = None if c.tasks is None else c.mask[:n]
    lmin = f32(c.cfg.log_std_min)
    return head(y, c.A, c.eps[:n], mask, lmin, f32(c.cfg.log_std_max) - lmin)
