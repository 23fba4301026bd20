"""Shared by tests/test_encoder_edges.py (CPU) and tests/test_gpu_encoder_edges.py (-m gpu): the state encoder's edge cases, its
fp64 reference, the measured gate and a numpy emulation of the kernels' summation order.

Reference: `z64` = tests/policy_common.fp64_encode (the CPU test pins it against oracle.planner_oracle.OracleModel in float64);
`z_ref32` = the same oracle in float32 on the CPU, the reference's own arithmetic.
Gate, per case: max|z - z64| <= 4 max(max|z_ref32 - z64|, 2^-23) (the measured-gate form of DESIGN 3.4h / 5); every gated case has
at least 512 output elements.

`emulate` follows the published order of encoder_kernels.cuh / policy_kernels.cuh: products in fp64 rounded to fp32 after every
add, four chains over k (k % 4) with the tail on chain 0, ((a0 + a1) + (a2 + a3)) + bias; on the wide route the four waves split
k in shares of ceil(in / 4) and their partials add as ((p0 + p1) + (p2 + p3)) + bias; block sums = per-thread sums over
f = tid + u 512, a xor butterfly 32..1 over the 64 lanes, then the eight waves in order.  pol_layer's sixteen-step loop feeds the
same four chains in the same order as k_encode's four-step loop, so the row copy shares the narrow emulation.  Not claimed bit-exact
(libm's expf, the compiler's contraction choices)."""
import dataclasses
from typing import Optional, Tuple

import numpy as np
import torch

from oracle import planner_oracle as po
from tdmpc2_amd import synth
from tdmpc2_amd.config import named_config
from tests import policy_common as pc

FACTOR, FLOOR = 4.0, 2.0 ** -23
MIN_ELEMENTS = 512
MAX_ENVS = 16
ENC_WIDE, ENC_MAX_WIDTH, ENC_MAX_LAYERS = 1024, 4096, 6
ENC_GEMV_LDS_MAX = 64 * 1024
ENC_MAX_IN = ENC_GEMV_LDS_MAX // 4 - 256   # encoder_kernels.cuh: k_enc_gemv's (in + 256) floats of LDS
THREADS = 512
N_TASKS = 30
f32, f64 = np.float32, np.float64


@dataclasses.dataclass
class Case:
    name: str
    obs_dim: int
    T: int
    widths: Tuple[int, ...]
    E: int
    kind: str = "shape"          # shape | mish | ln_const | ln_offset | ln_outlier | simnorm | task
    max_envs: int = MAX_ENVS
    pi: bool = False             # also runs through act_pi (narrow encoders)
    cfg: object = None
    sd: dict = None
    obs: np.ndarray = None
    tasks: Optional[np.ndarray] = None

    @property
    def route(self):
        return "wide" if max((self.obs_dim + self.T,) + self.widths) > ENC_WIDE else "narrow"

    @property
    def emb(self):
        return None if self.tasks is None else pc.task_rows(self.sd, self.tasks)[0]

    @property
    def mask(self):
        return None if self.tasks is None else pc.task_rows(self.sd, self.tasks)[1]


def make_cfg(latent, T, simnorm_dim=8):
    cfg = named_config("small", task="mt30" if T else "walker-run", latent_dim=latent, simnorm_dim=simnorm_dim)
    cfg.task_dim = T
    return cfg


def _selection(out_f, in_f, rng, signs=True):
    """Every output feature reads one input with weight +-1: pre-activations of integer inputs are exact in any order."""
    w = np.zeros((out_f, in_f), f32)
    sel = (np.arange(out_f) * 7 + 3) % in_f
    w[np.arange(out_f), sel] = np.where(rng.random(out_f) < 0.5, -1.0, 1.0) if signs else 1.0
    return w


def _fill(c: Case, seed):
    """Synth-style seeded weights of the encoder and a small policy prior, observations, per-row tasks; value probes pin theirs."""
    rng = np.random.default_rng(seed)
    c.cfg = cfg = make_cfg(c.widths[-1], c.T)
    sd, fin = {}, c.obs_dim + c.T
    for l, out in enumerate(c.widths):
        w, b = synth._linear(rng, out, fin)
        g, beta = synth._ln(rng, out)
        sd.update({f"_encoder.state.{l}.weight": w, f"_encoder.state.{l}.bias": b, f"_encoder.state.{l}.ln.weight": g,
                   f"_encoder.state.{l}.ln.bias": beta})
        fin = out
    M, A, fin = cfg.mlp_dim, cfg.action_dim, c.widths[-1] + c.T
    for l, out in enumerate((M, M, 2 * A)):
        sd[f"_pi.{l}.weight"], sd[f"_pi.{l}.bias"] = synth._linear(rng, out, fin, w_std=0.3 if l == 0 else 0.1)
        if l < 2:
            sd[f"_pi.{l}.ln.weight"], sd[f"_pi.{l}.ln.bias"] = synth._ln(rng, out)
        fin = out
    c.obs = rng.standard_normal((c.E, c.obs_dim)).astype(f32)
    if c.T:
        tab = rng.standard_normal((N_TASKS, c.T))
        # rows of norm 0.3 .. 0.9 on a 2^-10 grid: nn.Embedding(max_norm=1) leaves them alone in every precision
        tab = tab / np.linalg.norm(tab, axis=-1, keepdims=True) * rng.uniform(0.3, 0.9, (N_TASKS, 1))
        sd["_task_emb.weight"] = (np.round(tab * 1024) / 1024).astype(f32)
        sd["_action_masks"] = (rng.random((N_TASKS, A)) < 0.7).astype(f32)
        sd["_action_masks"][:, 0] = 1.0
        c.tasks = ((np.arange(c.E) * 7 + 2) % N_TASKS).astype(np.int64)  # distinct per row up to 30 rows
    c.sd = sd
    if c.kind != "shape":
        _pin(c, rng)
    return c


def _pin(c: Case, rng):
    """Value probes: depth 2, selection weights, zero bias, integer observations (module docstring of the GPU test)."""
    assert len(c.widths) == 2
    sd, E, H, L, D = c.sd, c.E, c.widths[0], c.widths[1], c.obs_dim
    p = "_encoder.state"
    sd[f"{p}.0.weight"] = _selection(H, D + c.T, rng, signs=c.kind not in ("ln_const", "ln_offset"))
    sd[f"{p}.1.weight"] = _selection(L, H, rng)
    for l, n in ((0, H), (1, L)):
        sd[f"{p}.{l}.bias"] = np.zeros(n, f32)
        sd[f"{p}.{l}.ln.weight"] = np.ones(n, f32)
        sd[f"{p}.{l}.ln.bias"] = np.zeros(n, f32)
    c.obs = rng.integers(-6, 7, (E, D)).astype(f32)
    if c.kind == "mish":
        # v = 0.01 LN(y) + bias: [-40, 40], the clamp's neighbourhood, below -30, and beyond where exp(v)^2 leaves fp32 (44.4)
        # and where expf itself does (88.8) -- without the clamp those are inf / inf
        pts = [-40.0, -35.0, -30.5, -30.0, -20.0, 19.9, 19.95, 19.99, 20.0, 20.01, 20.05, 20.1, 40.0, 44.0, 45.0, 60.0, 89.0, 100.0]
        v = np.concatenate([np.asarray(pts), np.linspace(-40.0, 40.0, H - len(pts))])
        sd[f"{p}.0.ln.weight"] = np.full(H, 0.01, f32)
        sd[f"{p}.0.ln.bias"] = v.astype(f32)
    elif c.kind == "ln_const":      # every feature of a row reads the same value with weight +1: variance 0
        c.obs = np.repeat(rng.integers(-6, 7, (E, 1)), D, axis=1).astype(f32)
        c.obs[0] = 0.0
        sd[f"{p}.0.ln.bias"] = (0.5 * rng.standard_normal(H)).astype(f32)   # the hidden row is then Mish(bias), not all equal
    elif c.kind == "ln_offset":
        c.obs = (1e4 + rng.integers(-3, 4, (E, D))).astype(f32)
    elif c.kind == "ln_outlier":
        c.obs[np.arange(E), np.arange(E) % D] = 60000.0
    elif c.kind == "simnorm":
        # gain 60 on the last LayerNorm: groups spread over 100; group 0 reads one hidden feature eight times (all equal),
        # group 1 reads two features four times each (exact ties at the maximum)
        w = sd[f"{p}.1.weight"]
        w[:16] = 0.0
        w[:8, 1] = 1.0
        w[8:12, 2] = 1.0
        w[12:16, 3] = -1.0
        sd[f"{p}.1.ln.weight"] = np.full(L, 60.0, f32)
    elif c.kind == "task":
        # the task columns carry row-distinct sixteenths; hidden feature f reads column (7 f + 3) % (D + T) of obs | task_emb
        tab = (rng.integers(-7, 8, (N_TASKS, c.T)) / 16.0).astype(f32)
        tab[np.arange(N_TASKS), np.arange(N_TASKS) % c.T] += (np.arange(N_TASKS) % 5 + 1) / 32.0
        assert (np.linalg.norm(tab, axis=-1) < 1.0).all()
        sd["_task_emb.weight"] = tab
    else:
        raise KeyError(c.kind)


def _shape(name, obs, T, widths, E, **kw):
    return Case(name, obs, T, tuple(widths), E, **kw)


def specs():
    """Every case, unfilled.  Latents are multiples of 32: creation refuses the others (the GPU test pins that), so the issue's
    `1 -> 8`, `.. -> 513 -> 72`, `1024 -> 16 -> 8`, `1025 -> 16 -> 8` and `7 -> 32 x5 -> 16` end in the nearest latent a handle can have."""
    S = _shape
    out = [
        S("n_1_32", 1, 0, (32,), 16, pi=True),
        S("n_3_63_64", 3, 0, (63, 64), 8, pi=True),
        S("n_5_65_513_96", 5, 0, (65, 513, 96), 8, pi=True),
        S("n_mt_17p2_1024_1023_1024", 17, 2, (1024, 1023, 1024), 2, pi=True),
        S("n_1024_16_32", 1024, 0, (16, 32), 16, pi=True),
        S("n_depth6", 7, 0, (32,) * 6, 16, pi=True),
        S("n_3_63_64_E49", 3, 0, (63, 64), 3 * MAX_ENVS + 1),
        S("w_1025_16_32", 1025, 0, (16, 32), 16),
        S("w_5_1025_64", 5, 0, (1025, 64), 8),
        S("w_37_4096_512_E1", 37, 0, (4096, 512), 1),
        S("w_mt_39p96_4095_1376", 39, 96, (4095, 1376), MAX_ENVS),
        S("w_depth6", 9, 0, (1100, 31, 1100, 31, 1100, 64), 8),
        S("w_511_1025_512_4096_64", 6, 0, (511, 1025, 512, 4096, 64), 8),
        S("n_6_511_512_64", 6, 0, (511, 512, 64), 8, pi=True),
        S("w_maxin_32", ENC_MAX_IN, 0, (32,), 16),   # the widest input a handle accepts: k_enc_gemv's LDS request at its limit
    ]
    out += [S(f"n_{k}_48_64", k, 0, (48, 64), 8, pi=True) for k in (15, 16, 17, 19)]
    out += [S("n_mt_11p5_48_64", 11, 5, (48, 64), 8, pi=True)]
    for kind in ("mish", "ln_const", "ln_offset", "ln_outlier", "simnorm"):
        out += [S(f"n_{kind}", 12, 0, (48, 64), 8, kind=kind, pi=True), S(f"w_{kind}", 12, 0, (48, 1088), 8, kind=kind)]
    out += [S("n_task", 5, 4, (48, 64), 8, kind="task", pi=True), S("w_task", 5, 4, (48, 1088), 8, kind="task")]
    return out


_built = {}


def case(name) -> Case:
    if name not in _built:
        all_ = specs()
        i = [c.name for c in all_].index(name)
        c = _fill(all_[i], seed=100 + i)
        assert c.E * c.widths[-1] >= MIN_ELEMENTS and (c.route == "narrow" or c.E <= c.max_envs)
        _built[name] = c
    return _built[name]


NAMES = [c.name for c in specs()]
PI_NAMES = [c.name for c in specs() if c.pi]
PI_SPREAD = "n_17_48_64_rows257"   # enough rows that launch_pi leaves the row route: the encoder then runs by its own launch


def pi_spread_case() -> Case:
    if PI_SPREAD not in _built:
        _built[PI_SPREAD] = _fill(_shape(PI_SPREAD, 17, 0, (48, 64), 257, max_envs=257, pi=True), seed=99)
    return _built[PI_SPREAD]


# ---------------------------------------------------------------------------------------------------------- references
_refs = {}


def _oracle(c: Case, dtype):
    sd = {k: torch.as_tensor(v) for k, v in c.sd.items()}
    tasks = None if c.tasks is None else torch.as_tensor(c.tasks)
    with torch.no_grad():
        return po.OracleModel(c.cfg, sd, dtype=dtype).encode(torch.as_tensor(c.obs).to(dtype), tasks).numpy()


def z64(c: Case):
    return refs(c)[0]


def z64_oracle(c: Case):
    return _oracle(c, torch.float64)


def z_ref32(c: Case):
    return refs(c)[1]


def refs(c: Case):
    """(z64, z_ref32, gate), computed once per case and left unchanged."""
    if c.name not in _refs:
        a = pc.fp64_encode(c.cfg, c.sd, c.obs, c.tasks)
        b = _oracle(c, torch.float32)
        a.setflags(write=False)
        b.setflags(write=False)
        _refs[c.name] = (a, b, gate(a, b))
    return _refs[c.name]


def ref_err(a64, b32):
    return max(float(np.abs(np.asarray(b32, f64) - a64).max()), FLOOR)


def gate(a64, b32):
    return FACTOR * ref_err(a64, b32)


def pi_refs(c: Case, eps):
    """fp64_encode -> fp64_pi, and the same chain in torch fp32 on the CPU: ({mean, log_std} fp64, the same in fp32)."""
    if ("pi", c.name) not in _refs:
        g64 = pc.fp64_pi(c.cfg, c.sd, z64(c), c.tasks, eps)
        sd = {k: torch.as_tensor(v) for k, v in c.sd.items()}
        m = po.OracleModel(c.cfg, sd)
        with torch.no_grad():
            x = torch.as_tensor(z_ref32(c))
            mask = None
            if c.tasks is not None:
                x = torch.cat([x, torch.as_tensor(c.emb)], -1)
                mask = torch.as_tensor(c.mask)
            out = po.mlp_forward(m.sd, "_pi", x)
            mean, ls = out.chunk(2, -1)
            ls = po.log_std_fn(ls, float(c.cfg.log_std_min), float(c.cfg.log_std_max) - float(c.cfg.log_std_min))
            if mask is not None:
                mean, ls = mean * mask, ls * mask
            g32 = {"mean": torch.tanh(mean).numpy(), "log_std": ls.numpy()}
        _refs[("pi", c.name)] = ({k: g64[k] for k in g32}, g32)
    return _refs[("pi", c.name)]


# ---------------------------------------------------------------------------------------------------------- order emulation
def _r(x):
    return np.asarray(x, f64).astype(f32)


def _fma(x, w, a):
    return _r(x.astype(f64) * w.astype(f64) + a.astype(f64))


def _chains(x, wt, k0, k1):
    """x [E, in], wt [in, out] -> the four chains of k0 <= k < k1, summed (a0 + a1) + (a2 + a3)"""
    a = [np.zeros((x.shape[0], wt.shape[1]), f32) for _ in range(4)]
    k = k0
    while k + 4 <= k1:
        for j in range(4):
            a[j] = _fma(x[:, k + j, None], wt[None, k + j], a[j])
        k += 4
    while k < k1:
        a[0] = _fma(x[:, k, None], wt[None, k], a[0])
        k += 1
    return (a[0] + a[1]) + (a[2] + a[3])


def _block_sum(per_thread):
    """[E, 512] per-thread values -> [E, 1]: xor butterfly over each wave's 64 lanes, then the eight waves in order"""
    v = per_thread.reshape(per_thread.shape[0], THREADS // 64, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    s = np.zeros(v.shape[0], f32)
    for w in range(THREADS // 64):
        s = s + v[:, w, 0]
    return s[:, None]


def _per_thread(y, fold):
    """y [E, out] -> [E, 512]: thread tid folds its features tid + u 512 in order of u"""
    E, out = y.shape
    pad = np.zeros((E, 8 * THREADS), f32)
    pad[:, :out] = y
    pad = pad.reshape(E, 8, THREADS)
    part = np.zeros((E, THREADS), f32)
    for u in range(8):
        part = fold(part, pad[:, u])
    return part


def _norm_act(y, g, b, last, sg):
    out = f32(y.shape[1])
    mean = _block_sum(_per_thread(y, lambda p, v: p + v)) / out
    d = y - mean
    var = _block_sum(_per_thread(d, lambda p, v: _fma(v, v, p))) / out
    rstd = f32(1.0) / np.sqrt(var + f32(1e-5), dtype=f32)
    v = _fma(d * rstd, g[None], b[None])
    with np.errstate(over="ignore", invalid="ignore"):
        if not last:
            ex = _r(np.exp(np.minimum(v, f32(20.0)).astype(f64)))
            n = ex * (ex + f32(2.0))
            return v * (n / (n + f32(2.0)))
        E, L = v.shape
        grp = v.reshape(E, L // sg, sg)
        ex = _r(np.exp((grp - grp.max(-1, keepdims=True)).astype(f64)))
        s, lane, o = ex, np.arange(sg), 1
        while o < sg:
            s = s + s[:, :, lane ^ o]
            o <<= 1
        return (ex / s).reshape(E, L)


def emulate(c: Case, route=None):
    """z [E, L] fp32 in the kernels' summation order on `route` ("narrow": k_encode and the row copy; "wide": k_enc_gemv + k_enc_norm)."""
    route = route or c.route
    x = c.obs if c.tasks is None else np.concatenate([c.obs, c.emb], -1)
    x = np.ascontiguousarray(x, f32)
    n = len(c.widths)
    for l in range(n):
        p = f"_encoder.state.{l}."
        wt = np.ascontiguousarray(np.asarray(c.sd[p + "weight"], f32).T)
        fin = wt.shape[0]
        bias = np.asarray(c.sd[p + "bias"], f32)[None]
        with np.errstate(over="ignore", invalid="ignore"):
            if route == "narrow":
                y = _chains(x, wt, 0, fin) + bias
            else:
                kq = (fin + 3) // 4
                q = [_chains(x, wt, w * kq, min(fin, w * kq + kq)) for w in range(4)]
                y = ((q[0] + q[1]) + (q[2] + q[3])) + bias
            x = _norm_act(y, np.asarray(c.sd[p + "ln.weight"], f32), np.asarray(c.sd[p + "ln.bias"], f32), l == n - 1, c.cfg.simnorm_dim)
    return x
