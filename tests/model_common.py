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
