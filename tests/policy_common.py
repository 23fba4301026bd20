"""Shared by the policy-prior tests: tests/golden/policy.npz (tools/make_policy_golden.py) and an fp64 evaluation of the reference's
WorldModel.pi (tdmpc2/common/world_model.py:144-184, common/math.py:12-29) on the fixture's inputs, from which the entropy gates are
derived (a quantity is gated against fp32's own distance from fp64)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.helpers import GOLDEN_DIR

CASES = ("tiny", "c2", "m19_mt30", "c3", "c4")
FIELDS = ("obs", "tasks", "eps", "z", "action", "mean", "log_std", "entropy", "scaled_entropy")
GATE = 1e-5  # mean, action, log_std, z: the encoder's Z_GATE


def golden(name):
    g = np.load(os.path.join(GOLDEN_DIR, "policy.npz"))
    out = {f: g[f"{name}.{f}"] for f in FIELDS}
    out["tasks"] = None if (out["tasks"] < 0).all() else out["tasks"]
    return out


def task_rows(sd, tasks):
    """(task_emb [n, T] with nn.Embedding(max_norm=1)'s renorm, act_mask [n, A]) of the rows' tasks, fp32 numpy."""
    w = np.asarray(sd["_task_emb.weight"], np.float32)[tasks]
    n = np.linalg.norm(w.astype(np.float32), axis=-1, keepdims=True)
    emb = np.where(n > 1.0, w * (1.0 / (n + 1e-7)), w).astype(np.float32)
    return emb, np.asarray(sd["_action_masks"], np.float32)[tasks]


def fp64_encode(cfg, sd, obs, tasks):
    """The reference's state encoder (layers.enc: NormedLinear + Mish, the last with SimNorm) in float64 -> z [n, L]."""
    d = lambda a: torch.as_tensor(np.asarray(a)).double()  # noqa: E731
    x = d(obs)
    if tasks is not None:
        x = torch.cat([x, d(task_rows(sd, tasks)[0])], -1)
    n = 0
    while f"_encoder.state.{n}.weight" in sd:
        n += 1
    for l in range(n):
        x = x @ d(sd[f"_encoder.state.{l}.weight"]).T + d(sd[f"_encoder.state.{l}.bias"])
        x = F.layer_norm(x, (x.shape[-1],), d(sd[f"_encoder.state.{l}.ln.weight"]), d(sd[f"_encoder.state.{l}.ln.bias"]), 1e-5)
        if l < n - 1:
            x = x * torch.tanh(F.softplus(x))
        else:
            x = torch.softmax(x.view(x.shape[0], -1, cfg.simnorm_dim), -1).view(x.shape[0], -1)
    return x.numpy()


def fp64_pi(cfg, sd, z, tasks, eps, dtype=torch.float64):
    """The reference's pi in float64 on z (fp32 inputs promoted): {mean, log_std, action, entropy, scaled_entropy}.  `dtype`
    torch.float32: the same formula in the reference's own arithmetic on the CPU (tests/policy_edges_common.py's ref32)."""
    d = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
    x = d(z)
    mask = None
    if tasks is not None:
        emb, mask = task_rows(sd, tasks)
        x = torch.cat([x, d(emb)], -1)
        mask = d(mask)
    for l in range(3):
        x = x @ d(sd[f"_pi.{l}.weight"]).T + d(sd[f"_pi.{l}.bias"])
        if l < 2:
            x = F.layer_norm(x, (x.shape[-1],), d(sd[f"_pi.{l}.ln.weight"]), d(sd[f"_pi.{l}.ln.bias"]), 1e-5)
            x = x * torch.tanh(F.softplus(x))
    mean, ls = x.chunk(2, -1)
    lmin = float(np.float32(cfg.log_std_min))
    ldif = float(np.float32(cfg.log_std_max) - np.float32(cfg.log_std_min))
    ls = lmin + 0.5 * ldif * (torch.tanh(ls) + 1)
    e = d(eps)
    if mask is not None:
        mean, ls, e = mean * mask, ls * mask, e * mask
    lp = (-0.5 * e.pow(2) - ls - 0.9189385175704956).sum(-1, keepdim=True)
    slp = lp * (e.shape[-1] if mask is None else mask.sum(-1, keepdim=True))
    act = torch.tanh(mean + e * ls.exp())
    lp = lp - torch.log(F.relu(1 - act.pow(2)) + 1e-6).sum(-1, keepdim=True)
    return {"mean": torch.tanh(mean).numpy(), "log_std": ls.numpy(), "action": act.numpy(), "entropy": (-lp).numpy(),
            "scaled_entropy": (-lp * (slp / (lp + 1e-8))).numpy()}


def entropy_bound(g64, gold, key):
    """Per-value gate: max(1e-5 relative to max(1, |value|), 2 x |reference fp32 - fp64|) -- entropy / scaled_entropy per row,
    and the GPU tests' mean / action / log_std per element."""
    v64 = g64[key].reshape(-1)
    ref = np.asarray(gold[key], np.float64).reshape(-1)
    return np.maximum(GATE * np.maximum(1.0, np.abs(v64)), 2.0 * np.abs(ref - v64))
