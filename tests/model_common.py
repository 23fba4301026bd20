"""Shared by the model rollout / loss tests and tools/make_model_golden.py: the case table, the seeded inputs, the fixture
reader, and a numpy restatement of the loss row math (reference tdmpc2/common/math.py:5-9, 42-47, 58-71; tdmpc2/tdmpc2.py:285-304)."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# case -> (batch of the full entry, batch of the small entry or None)
CASES = {"tiny": (12, 130), "tiny_mt": (12, 130), "small_ep_fire": (12, 130), "c1_ep": (12, 130), "c2": (12, 130),
         "mt5": (12, 130), "c3": (12, 130), "c4": (8, None)}
TARGET_CASES = ("tiny_mt", "c1_ep", "c3")   # fixtures with the target ensemble's heads on the same rollout ("tq.q_logits", "tq.q")
OBS_CASES = ("tiny", "c2", "tiny_mt")   # fixtures that also carry the reference's encode output of seeded observations
FULL = ("zs", "reward_logits", "reward", "q_logits", "q", "term_logit", "losses", "step_means")
SMALL = ("reward", "q", "term_logit", "losses", "step_means")
RTOL = 1e-4   # the project's gate for this layer code (TD_RTOL, tests/test_gpu_td_target.py)


def path(name):
    return os.path.join(GOLDEN_DIR, f"model_{name}.npz")


def golden(name):
    with np.load(path(name)) as f:
        return {k: f[k] for k in f.files}


def inputs(cfg, B):
    """Seeded inputs of one case at batch B (nothing of this is stored): z0, actions [H, B, A] and cases.td_batch."""
    from oracle import cases
    from tdmpc2_amd import synth

    tb = cases.td_batch(cfg, B)
    z0 = synth.make_latents(cfg, B, seed=9)
    actions = np.random.default_rng(31).uniform(-1, 1, (cfg.horizon, B, cfg.action_dim)).astype(np.float32)
    return dict(tb, z0=z0, actions=actions)


def obs_inputs(cfg, B):
    rng = np.random.default_rng(41)
    return rng.standard_normal((cfg.horizon + 1, B, cfg.obs_shape["state"][0])).astype(np.float32)


def tol(v, d64):
    """Per element: max(1e-4 max(1, |v|), 2 x the reference's own fp32-vs-fp64 distance of the field)."""
    return np.maximum(RTOL * np.maximum(1.0, np.abs(v)), 2.0 * float(d64))


# ---------------------------------------------------------------- loss row math, dtype of the inputs (fp64 in the tests)
def symlog(x):
    return np.sign(x) * np.log(1 + np.abs(x))


def soft_ce_rows(logits, target, cfg):
    """soft_ce of rows: logits [R, bins], target [R] -> [R]; the two target bins picked by index."""
    nb = cfg.num_bins
    m = logits.max(-1, keepdims=True)
    lse = (m + np.log(np.exp(logits - m).sum(-1, keepdims=True)))[:, 0]
    x = np.clip(symlog(target), cfg.vmin, cfg.vmax)
    bin_size = (cfg.vmax - cfg.vmin) / (nb - 1)
    u = (x - cfg.vmin) / bin_size
    i0 = np.clip(np.floor(u).astype(np.int64), 0, nb - 1)
    off = u - np.floor(u)
    i1 = (i0 + 1) % nb
    r = np.arange(len(target))
    return -((1 - off) * (logits[r, i0] - lse) + off * (logits[r, i1] - lse))


def bce_logits(x, y):
    return np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))


def losses_from(cfg, zs, reward_logits, q_logits, term_logit, next_z, reward, td, terminated):
    """tdmpc2.py:285-304 from predictions and targets ([H, B] targets) -> (losses [5], step_means [4, H])."""
    H, B = reward.shape
    sm = np.zeros((4, H), zs.dtype)
    for t in range(H):
        sm[0, t] = ((zs[t + 1] - next_z[t]) ** 2).mean()
        sm[1, t] = soft_ce_rows(reward_logits[t], reward[t], cfg).mean()
        sm[2, t] = np.mean([soft_ce_rows(q_logits[i, t], td[t], cfg).mean() for i in range(q_logits.shape[0])])
        if cfg.episodic:
            sm[3, t] = bce_logits(term_logit[t + 1], terminated[t]).mean()
    w = np.array([cfg.rho ** t for t in range(H)], zs.dtype)
    cons, rew, val = (sm[0] * w).sum() / H, (sm[1] * w).sum() / H, (sm[2] * w).sum() / H
    term = sm[3].mean() if cfg.episodic else 0.0
    total = cfg.consistency_coef * cons + cfg.reward_coef * rew + cfg.termination_coef * term + cfg.value_coef * val
    return np.array([cons, rew, val, term, total], zs.dtype), sm


# ---------------------------------------------------------------- pinned logits and edge inputs (tests/test_model_edges.py,
# tests/test_gpu_model_edges.py).  A head whose last layer has weight 0 and bias l gives the logits l on every row, exactly
# (0 x + b = b for finite x in either arithmetic): known logits reach the loss kernels through the public entry points.
EDGE_FLOOR = 1e-5   # the project's loss-stage floor (tests/test_gpu_model.py, "the loss stage alone")


def symexp(x):
    return np.sign(x) * (np.exp(np.abs(x)) - 1)


def two_hot_inv_rows(logits, cfg):
    """two_hot_inv of rows (math.py:74-83): logits [..., bins] -> [...], in the dtype of the logits."""
    b = np.linspace(cfg.vmin, cfg.vmax, cfg.num_bins).astype(logits.dtype)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    return symexp((p * b).sum(-1))


def pin_heads(sd, cfg, reward_row=None, q_rows=None, term_x=None):
    """A copy of a state dict (torch tensors) with the named heads' last layers pinned: weight 0, bias the given fp32 logits.
    reward_row [bins]; q_rows [num_q, bins], written to the online and the target ensemble; term_x a scalar."""
    import torch

    out = {k: torch.as_tensor(v).clone() for k, v in sd.items()}

    def pin(key, bias):
        b = torch.as_tensor(np.asarray(bias, np.float32)).reshape(out[f"{key}.bias"].shape)
        out[f"{key}.weight"] = torch.zeros_like(out[f"{key}.weight"])
        out[f"{key}.bias"] = b.to(out[f"{key}.bias"].dtype)

    if reward_row is not None:
        pin("_reward.2", reward_row)
    if q_rows is not None:
        for key in ("_Qs.params.2", "_target_Qs_params.2", "_detach_Qs_params.2"):
            if f"{key}.weight" in out:
                pin(key, q_rows)
    if term_x is not None:
        pin("_termination.2", [term_x])
    return out


def edge_gate(v64, v32):
    """Per element: max(1e-5 max(1, |v|), 2 x |restatement in fp32 - restatement in fp64|), both restatements evaluated on the
    host from the exact fp32 logits and targets; nothing in it comes from a HIP result."""
    v64 = np.asarray(v64, np.float64)
    return np.maximum(EDGE_FLOOR * np.maximum(1.0, np.abs(v64)), 2.0 * np.abs(np.asarray(v32, np.float64) - v64))


EDGE_KS = (0, 1, 2, 49, 50, 51, 98, 99, 100)


def edge_targets(cfg):
    """fp32 targets at the edges of symlog / the clamp / the bins: 45 values, padded with three ordinary ones to 6 x 8."""
    t = [0.0, -0.0, 1e-8, -1e-8, 1e-30, -1e-30]
    bin_size = (cfg.vmax - cfg.vmin) / (cfg.num_bins - 1)
    for k in EDGE_KS:
        c = np.float32(symexp(np.float64(cfg.vmin + k * bin_size)))
        t += [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    t += [22025.4, -22025.4, 22026.5, -22026.5, 22027.0, -22027.0]   # symexp(10) = 22025.47: both sides of the clamp
    t += [1e6, -1e6, 3e38, -3e38, np.inf, -np.inf]
    t += [1.0, -2.5, 123.0]
    return np.array(t, np.float32)


EDGE_OFFSETS = (0.0, 30.0, -30.0, 300.0, -300.0)
UNGATED_ROW = "off+10000"   # lse = m + log(sum) loses the digits of log(sum) at m = 1e4: printed, not gated


def edge_logit_rows(cfg):
    """name -> fp32 logits row [bins] (seeded or literal)."""
    nb = cfg.num_bins
    rng = np.random.default_rng(20)
    rows = {"zero": np.zeros(nb)}
    for s in (1, 10, 30, 100):
        rows[f"n{s}"] = rng.standard_normal(nb) * s
    for j in (0, nb // 2, nb - 1):
        r = np.full(nb, -1e4)
        r[j] = 0.0
        rows[f"hot{j}"] = r
    r = rng.standard_normal(nb) * 3
    r[40] = r[41] = r.max() + 1.0
    rows["twomax"] = r
    base = rng.standard_normal(nb) * 3
    for c in EDGE_OFFSETS:
        rows[f"off{c:+.0f}"] = base.astype(np.float32) + np.float32(c)
    rows[UNGATED_ROW] = base.astype(np.float32) + np.float32(1e4)
    return {k: np.asarray(v, np.float32) for k, v in rows.items()}


# (row, target) pairs at which the REFERENCE's own fp32 soft_ce leaves the gate (tests/test_model_edges.py measures it): not
# asked of the library either.  Filled from that test's output; each entry names the measured err / gate.
EDGE_REMOVED = {}


def edge_pairs(cfg):
    """Every gated (row name, target index) of the edge table."""
    t = edge_targets(cfg)
    return [(name, i) for name in edge_logit_rows(cfg) if name != UNGATED_ROW for i in range(len(t))
            if (name, i) not in EDGE_REMOVED]


TERM_XS = (0.0, -0.0, 1e-8, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4)
TERM_YS = (0.0, 1.0, 0.3)
