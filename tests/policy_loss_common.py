"""Shared by the policy-loss tests and tools/make_policy_loss_golden.py: the case table, the seeded inputs, the fixture reader and
an fp32 / fp64 numpy restatement of RunningScale.update (reference tdmpc2/common/scale.py:21-42), the loss assembly of update_pi
(tdmpc2/tdmpc2.py:223-228) and math.termination_statistics (common/math.py:97-109)."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("tiny", "tiny_mt", "c1_ep", "c2", "mt5", "c3")
# kernel families a case runs on (tdmpc2_path: 1 fused, 2 layered; 0 auto for the 64-wide models, which only the layered family takes)
PATHS = {"tiny": (0,), "tiny_mt": (0,), "c1_ep": (1, 2), "c2": (1, 2), "mt5": (1, 2), "c3": (2,)}
B_FULL, B_SMALL = 12, 130                     # per-row fields at B_FULL; scalars at both
SCALES0 = (1.0, 7.5)                          # RunningScale.value before the call
ROW_FIELDS = ("action", "q", "entropy", "scaled_entropy")
SCALAR_FIELDS = ("loss", "step_means", "percentiles")
SCALE_NS = (1, 2, 3, 20, 21, 41, 130, 256, 257, 4096)
SCALE_KINDS = ("normal", "ties", "x300")
SCALE_CASE = "tiny"                           # the fixture that carries the scale table
TERM_CASE = "c1_ep"                           # the fixture that carries termination statistics of seeded logits
TAU = 0.01


def path(name):
    return os.path.join(GOLDEN_DIR, f"policy_loss_{name}.npz")


def golden(name):
    with np.load(path(name)) as f:
        return {k: f[k] for k in f.files}


def inputs(cfg, B):
    """Seeded inputs of one case at batch B (never stored): zs [H+1, B, L], pi_eps [H+1, B, A], qidx, tasks [B]."""
    from oracle import cases
    from tdmpc2_amd import synth

    T = cfg.horizon + 1
    tb = cases.td_batch(cfg, B)
    zs = synth.make_latents(cfg, T * B, seed=13).reshape(T, B, cfg.latent_dim)
    pi_eps = np.random.default_rng(17).standard_normal((T, B, cfg.action_dim)).astype(np.float32)
    return dict(zs=zs, pi_eps=pi_eps, qidx=tb["qidx"], tasks=tb["tasks"])


def scale_input(n, kind):
    x = (np.random.default_rng(100 + n).standard_normal(n) * 3).astype(np.float32)
    if kind == "ties":
        x = (np.round(x * 2) / 2).astype(np.float32)
    elif kind == "x300":
        x = (x * np.float32(300)).astype(np.float32)
    return x


def nan_input(n):
    x = scale_input(n, "normal").copy()
    x[n // 3] = np.nan
    return x


def term_input(n=B_SMALL):
    rng = np.random.default_rng(23)
    return (rng.standard_normal(n) * 2).astype(np.float32), (rng.random(n) < 0.3).astype(np.float32)


def tol(v, d64):
    """Per element: max(1e-4 max(1, |v|), 2 x the reference's own fp32-vs-fp64 distance) -- tests/model_common.py: tol."""
    return np.maximum(1e-4 * np.maximum(1.0, np.abs(v)), 2.0 * float(d64))


def edge_gate(v64, v32):
    """max(1e-5 max(1, |v|), 2 x |restatement fp32 - restatement fp64|) -- tests/model_common.py: edge_gate."""
    v64 = np.asarray(v64, np.float64)
    return np.maximum(1e-5 * np.maximum(1.0, np.abs(v64)), 2.0 * np.abs(np.asarray(v32, np.float64) - v64))


def ulp_diff(a, b):
    """Distance in fp32 units in the last place (both NaN: 0)."""
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) and np.isnan(b):
        return 0
    if np.isnan(a) or np.isnan(b):
        return 2**31
    key = lambda v: (lambda i: i if i >= 0 else -(i & 0x7FFFFFFF))(int(np.array(v, np.float32).view(np.int32)))
    return abs(key(a) - key(b))


# ---------------------------------------------------------------- restatements
def percentiles(x, dtype=np.float32):
    """RunningScale._percentile of n values: positions and weights in fp32 as scale.py:21-28 forms them, products in `dtype`."""
    f = np.float32
    xs = np.sort(np.asarray(x, dtype).reshape(-1))   # NaN last, as torch.sort
    n = len(xs)
    out = []
    for pct in (f(5), f(95)):
        pos = f(f(pct * f(n - 1)) / f(100))
        fl = np.floor(pos)
        ce = min(f(fl + f(1)), f(n - 1))
        wc = f(pos - fl)
        wf = f(f(1) - wc)
        out.append(dtype(dtype(xs[int(fl)] * dtype(wf)) + dtype(xs[int(ce)] * dtype(wc))))
    return np.array(out, dtype)


def scale_update(x, s0, tau=TAU, dtype=np.float32):
    """RunningScale.update -> (percentiles [2], value after the lerp): clamp(p95 - p5, min = 1) keeps a NaN; s + tau (v - s)."""
    p = percentiles(x, dtype)
    d = dtype(p[1] - p[0])
    v = d if np.isnan(d) else max(d, dtype(1))
    s0 = dtype(s0)
    return p, dtype(s0 + dtype(dtype(tau) * dtype(v - s0)))


def loss_from(q, ent, sent, scale, rho, entropy_coef, dtype=np.float32):
    """tdmpc2.py:224-228 from per-row terms [T, B]: (loss [4] = pi_loss, mean entropy, mean scaled_entropy, scale; step_means [3, T])."""
    q, ent, sent = (np.asarray(a, dtype).reshape(a.shape[0], -1) for a in (q, ent, sent))
    scale = dtype(scale)
    qs = q / scale
    T = q.shape[0]
    w = np.array([dtype(np.float32(rho)) ** t for t in range(T)], dtype)
    pi_loss = (-(dtype(np.float32(entropy_coef)) * sent + qs).mean(1) * w).mean()
    sm = np.stack([qs.mean(1), sent.mean(1), ent.mean(1)])
    return np.array([pi_loss, ent.mean(), sent.mean(), scale], dtype), sm.astype(dtype)


def sigmoid32(x):
    """1 / (1 + exp(-x)) in fp32 with a correctly rounded exp (numpy's own fp32 exp is a 1-ulp SIMD routine: at x = 1e-7 it
    returns 1 - 2^-24 where the rounded value is 1 - 2^-23, which moves the knife edge sigmoid > 0.5)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        e = np.exp(-x.astype(np.float64)).astype(np.float32)
    return (np.float32(1) / (np.float32(1) + e)).astype(np.float32)


def term_counts(x, y):
    """tp, fn, fp of math.py:102-104 with pred = fp32 sigmoid(x) > 0.5."""
    pred = sigmoid32(x) > np.float32(0.5)
    y = np.asarray(y, np.float32)
    return int((pred & (y == 1)).sum()), int((~pred & (y == 1)).sum()), int((pred & (y == 0)).sum())


def term_stats(tp, fn, fp, ysum, n):
    """math.py:101-107 in fp32 from the counts: (rate, f1)."""
    f = np.float32
    eps = f(1e-9)
    recall = f(f(tp) / f(f(tp + fn) + eps))
    precision = f(f(tp) / f(f(tp + fp) + eps))
    f1 = f(f(f(2) * f(precision * recall)) / f(f(precision + recall) + eps))
    return f(f(ysum) / f(n)), f1


TERM_EDGE_XS = (0.0, -0.0, 1e-8, 1e-7, 3e-7, 20.0, -20.0)
TERM_EDGE_YS = (0.0, 1.0)
