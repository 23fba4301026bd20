"""CPU: the fixtures tests/golden/model_<case>.npz (tools/make_model_golden.py) -- shapes, a `_d64` beside every field, size --,
regenerated bit for bit where the reference tree is present; and the numpy restatement of the loss row math
(tests/model_common.py) that the GPU test's error attribution leans on: against the reference's own soft_ce / BCE in fp64 to
1e-12 (reference tree present), and against every fixture's stored losses computed from its stored fp32 predictions."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import model_common as mc



def _cfg(name):
    from oracle import cases

    return cases.build_case(name)["cfg"]


@pytest.mark.parametrize("name", mc.CASES)
def test_fixture_layout(name):
    assert os.path.getsize(mc.path(name)) <= 400 * 1024
    g = mc.golden(name)
    cfg = _cfg(name)
    H, L, A, nq, nb = cfg.horizon, cfg.latent_dim, cfg.action_dim, cfg.num_q, max(cfg.num_bins, 1)
    b_full, b_small = mc.CASES[name]
    for B, fields in ((b_full, mc.FULL), (b_small, mc.SMALL)):
        if not B:
            assert not any(k.startswith("b130.") for k in g)
            continue
        shapes = {"zs": (H + 1, B, L), "reward_logits": (H, B, nb), "reward": (H, B, 1), "q_logits": (nq, H, B, nb),
                  "q": (nq, H, B, 1), "term_logit": (H + 1, B, 1), "losses": (5,), "step_means": (4, H)}
        for k in fields:
            if k == "term_logit" and not cfg.episodic:
                assert f"b{B}.{k}" not in g
                continue
            assert g[f"b{B}.{k}"].shape == shapes[k] and g[f"b{B}.{k}"].dtype == np.float32, (k, B)
            assert np.isfinite(g[f"b{B}.{k}"]).all()
            assert 0 <= float(g[f"b{B}.{k}_d64"]) < 1e-4, (k, B)   # the reference's own round-off: well inside the 1e-4 gate
        assert g[f"b{B}.td"].shape == (H, B)
        if fields is mc.SMALL:
            assert not any(f"b{B}.{k}" in g for k in ("zs", "reward_logits", "q_logits"))
    if name in mc.TARGET_CASES:
        assert g["tq.q_logits"].shape == (nq, H, b_full, nb) and g["tq.q"].shape == (nq, H, b_full, 1)
        assert 0 <= float(g["tq.q_logits_d64"]) < 1e-4 and 0 <= float(g["tq.q_d64"]) < 1e-4
        assert np.abs(g["tq.q_logits"] - g[f"b{b_full}.q_logits"]).max() > 1e-2   # another parameter set than the online heads
    if name in mc.OBS_CASES:
        assert g["obs.z"].shape == (H + 1, b_full, L) and g["obs.losses"].shape == (5,) and "obs.losses_d64" in g


@pytest.mark.parametrize("name", mc.CASES)
def test_fixture_regenerates_bit_for_bit(name):
    from oracle import ref_runner

    if not ref_runner.available():
        pytest.skip("reference tree not present")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_model_golden", os.path.join(os.path.dirname(mc.GOLDEN_DIR), "..", "tools", "make_model_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res, g = mod.generate(name), mc.golden(name)
    assert sorted(res) == sorted(g)
    for k in g:
        assert np.array_equal(np.asarray(res[k]), g[k]), k


@pytest.mark.parametrize("name", mc.CASES)
def test_loss_restatement_reproduces_the_stored_losses(name):
    """From the fixture's own fp32 predictions, in fp64: the stored losses within the reference's stored fp32-vs-fp64 distance
    (+ 1e-6 for the predictions themselves being fp32 roundings of what the fp64 run saw)."""
    cfg = _cfg(name)
    g = mc.golden(name)
    B = mc.CASES[name][0]
    inp = mc.inputs(cfg, B)
    f = lambda k: g[f"b{B}.{k}"].astype(np.float64)
    tl = f("term_logit")[..., 0] if cfg.episodic else None
    ls, sm = mc.losses_from(cfg, f("zs"), f("reward_logits"), f("q_logits"), tl, inp["next_z"].astype(np.float64),
                            inp["reward"][..., 0].astype(np.float64), f("td"), inp["terminated"][..., 0].astype(np.float64))
    for k, v in (("losses", ls), ("step_means", sm)):
        err = np.abs(v - g[f"b{B}.{k}"])
        assert (err <= 2 * float(g[f"b{B}.{k}_d64"]) + 1e-6 * np.maximum(1, np.abs(v))).all(), (k, err.max())


def _edge_targets(cfg):
    top = np.expm1(cfg.vmax)
    return np.array([0.0, top, -top, top * 1.5, -top * 3, np.nextafter(top, 0), 1e-9, -2.5, 7.0, 0.2, 123.0])


def test_loss_row_math_edges():
    """vmax / vmin edge rows: targets at exactly symexp(vmax), beyond it, and 0 -- the weights stay a two-hot (sum 1, the
    wrapped upper bin has weight 0) and the value is the cross entropy against it."""
    cfg = SimpleNamespace(num_bins=101, vmin=-10.0, vmax=10.0)
    rng = np.random.default_rng(0)
    t = _edge_targets(cfg)
    lg = rng.standard_normal((len(t), 101)) * 3
    got = mc.soft_ce_rows(lg, t, cfg)
    logp = lg - np.log(np.exp(lg).sum(-1, keepdims=True))
    x = np.clip(mc.symlog(t), -10, 10)
    for i in range(len(t)):   # dense two-hot, built the slow way
        w = np.zeros(101)
        u = (x[i] + 10) / 0.2
        j = min(int(np.floor(u + 1e-12)) if abs(u - round(u)) < 1e-9 else int(np.floor(u)), 100)
        w[j] += 1 - (u - j)
        w[(j + 1) % 101] += u - j
        assert abs(w.sum() - 1) < 1e-12
        assert abs(got[i] + (w * logp[i]).sum()) < 1e-9, (i, t[i])
    assert abs(got[1] + logp[1, 100]) < 1e-9 and abs(got[2] + logp[2, 0]) < 1e-9 and abs(got[0] + logp[0, 50]) < 1e-9


def test_loss_row_math_against_the_reference():
    from oracle import ref_runner

    if not ref_runner.available():
        pytest.skip("reference tree not present")
    import torch
    import torch.nn.functional as F
    ref_runner._import_reference()
    from common import math as rmath

    cfg = SimpleNamespace(num_bins=101, vmin=-10.0, vmax=10.0, bin_size=20.0 / 100)
    rng = np.random.default_rng(1)
    t = np.concatenate([_edge_targets(cfg), rng.standard_normal(200) * 50])
    lg = rng.standard_normal((len(t), 101)) * 4
    want = rmath.soft_ce(torch.as_tensor(lg), torch.as_tensor(t)[:, None], cfg)[:, 0].numpy()
    assert np.abs(mc.soft_ce_rows(lg, t, cfg) - want).max() <= 1e-12 * np.maximum(1, np.abs(want)).max()
    x, y = rng.standard_normal(500) * 8, (rng.random(500) < 0.3).astype(np.float64)
    wb = F.binary_cross_entropy_with_logits(torch.as_tensor(x), torch.as_tensor(y), reduction="none").numpy()
    assert np.abs(mc.bce_logits(x, y) - wb).max() <= 1e-12
