"""CPU: the fixture tests/golden/update_steps.npz (tools/make_update_golden.py: K iterations of the reference's own `_update` per
case, fp64 and fp32, and one fp64 run per deliberately wrong control) -- its layout and size, regenerated bit for bit where the
reference tree is present, the conditions on its inputs without which tests/test_gpu_update.py could pass vacuously, and the
sensitivity of its gates: every control lies at least 10 bounds away from the verbatim run."""
import os

import numpy as np
import pytest

from tests import update_common as uc


@pytest.fixture(scope="module")
def g():
    return uc.golden()


@pytest.fixture(scope="module")
def cfgs():
    return {c: uc.build(c)[0] for c in uc.CASES}


def _col(g, cfgs, case_id, key, name="info64"):
    return g[f"{case_id}.{name}"][:, uc.info_keys(cfgs[case_id]).index(key)]


def test_layout_and_size(g, cfgs):
    assert os.path.getsize(uc.GOLDEN) <= uc.SIZE_CAP
    assert float(g["scale0"]) == uc.SCALE0
    expected = {"scale0"}
    for case_id, spec in uc.CASES.items():
        cfg = cfgs[case_id]
        K, H, B, A, od, n = uc.K, cfg.horizon, spec["B"], cfg.action_dim, cfg.obs_shape["state"][0], len(uc.info_keys(cfg))
        shapes = {"obs": ((H + 1, B, od), np.float32), "action": ((H, B, A), np.float32), "reward": ((H, B, 1), np.float32),
                  "td_pi_eps": ((K, H, B, A), np.float32), "td_qidx": ((K, 2), np.int32), "pi_eps": ((K, H + 1, B, A), np.float32),
                  "qidx": ((K, 2), np.int32), "info64": ((K, n), np.float64), "info32": ((K, n), np.float64),
                  "td64": ((K, H, B, 1), np.float64), "td32": ((K, H, B, 1), np.float32)}
        if cfg.episodic:
            shapes["terminated"] = ((H, B, 1), np.float32)
            shapes["term_logit64"] = ((K, B, 1), np.float64)
        if cfg.multitask:
            shapes["task"] = ((B,), np.int64)
        for control in uc.controls_of(cfg):
            shapes[f"{control}.info64"] = ((K, n), np.float64)
            shapes[f"{control}.td64"] = ((K, H, B, 1), np.float64)
        for k, (shape, dtype) in shapes.items():
            a = g[f"{case_id}.{k}"]
            assert a.shape == shape and a.dtype == dtype and np.isfinite(a).all(), (case_id, k, a.shape, a.dtype)
        expected |= {f"{case_id}.{k}" for k in shapes}
        assert (H, B) == {"tiny-B33": (2, 33), "tiny_mt-B12": (2, 12), "small_ep-B9": (3, 9), "tiny_wideq-B12": (2, 12),
                          "tiny-H1-B1": (1, 1)}[case_id]
        # the stored inputs are the seeded ones
        batch, pins = uc.inputs(case_id, cfg)
        for k, v in {**batch, **pins}.items():
            assert np.array_equal(g[f"{case_id}.{k}"], v), (case_id, k)
    assert set(g) == expected


def test_generator_reproduces_the_fixture(g):
    from oracle import ref_runner

    if not ref_runner.available():
        pytest.skip("reference tree not available")
    import sys

    sys.path.insert(0, os.path.join(uc.ROOT, "tools"))
    import make_update_golden as gen

    new = gen.generate()
    assert set(g) == set(new)
    for k in g:
        assert np.asarray(new[k]).dtype == g[k].dtype and np.array_equal(g[k], new[k]), k


# ---------------------------------------------------------------- conditions on the inputs
def test_head_pairs(g, cfgs):
    for case_id in uc.CASES:
        nq = cfgs[case_id].num_q
        for name in ("td_qidx", "qidx"):
            q = g[f"{case_id}.{name}"]
            assert (q[:, 0] != q[:, 1]).all() and q.min() >= 0 and q.max() == nq - 1        # two heads; some pair uses num_q - 1
            assert len({tuple(p) for p in q.tolist()}) == uc.K                               # the pairs differ between iterations
            assert (q[:, 0] > q[:, 1]).any() and (q[:, 0] < q[:, 1]).any()                   # some pair has its first index above


def test_multitask_case_uses_a_mask_and_two_discounts(g, cfgs):
    from tdmpc2_amd.config import get_discount

    cfg = cfgs["tiny_mt-B12"]
    task = g["tiny_mt-B12.task"]
    assert np.array_equal(task, np.arange(12) % len(cfg.tasks))
    assert any(cfg.action_dims[t] < cfg.action_dim for t in task)
    assert len({get_discount(cfg, cfg.episode_lengths[t]) for t in task}) >= 2
    _, sd = uc.build("tiny_mt-B12")
    assert (sd["_action_masks"][task].sum(-1) < cfg.action_dim).any()


def test_episodic_case_has_terminations_and_decided_logits(g, cfgs):
    last = g["small_ep-B9.terminated"][-1]
    assert (last == 1).any() and (last == 0).any()
    assert float(np.abs(g["small_ep-B9.term_logit64"]).min()) >= 1e-4
    logit, keys = g["small_ep-B9.term_logit64"], uc.info_keys(cfgs["small_ep-B9"])
    assert (logit > 0).any() and (logit < 0).any()   # both predictions occur
    # the stored statistics are those of the stored logits (math.termination_statistics: sigmoid(.) > 0.5 terminates)
    for it in range(uc.K):
        pred, y = logit[it, :, 0] > 0, last[:, 0] == 1
        tp, fn, fp = (pred & y).sum(), (~pred & y).sum(), (pred & ~y).sum()
        rec, prec = tp / (tp + fn + 1e-9), tp / (tp + fp + 1e-9)
        f1 = 2 * prec * rec / (prec + rec + 1e-9)
        assert abs(g["small_ep-B9.info64"][it, keys.index("termination_rate")] - y.mean()) <= 1e-6
        assert abs(g["small_ep-B9.info64"][it, keys.index("termination_f1")] - f1) <= 1e-6


def test_percentile_path_is_live_only_where_it_is_meant_to_be(g, cfgs):
    tau = uc.oc.widen(cfgs["tiny-B33"].tau)
    for case_id in uc.CASES:
        s = np.concatenate([[uc.SCALE0], _col(g, cfgs, case_id, "pi_scale")])
        clamped = s[:-1] + tau * (1.0 - s[:-1])  # lerp(previous, 1, tau): clamp(min=1) won
        if case_id == "tiny_wideq-B12":
            assert (np.abs(s[1:] - clamped) > 1e-3 * s[1:]).all(), s
        else:
            assert np.allclose(s[1:], clamped, rtol=1e-12), (case_id, s)


def test_gated_scalars_have_a_relative_error(g, cfgs):
    for case_id in uc.CASES:
        cfg = cfgs[case_id]
        keys = uc.info_keys(cfg)
        bounds = uc.info_bounds(g, case_id, keys)
        for k in keys:
            col = _col(g, cfgs, case_id, k)
            if k == "termination_loss" and not cfg.episodic:
                assert bounds[k] is None and not col.any() and not _col(g, cfgs, case_id, k, "info32").any()
            elif k in uc.STAT_KEYS:
                assert bounds[k] is None
                assert np.allclose(col, _col(g, cfgs, case_id, k, "info32"), atol=1e-6, rtol=0)  # decided: both runs agree
            else:
                assert (col != 0).all() and bounds[k] is not None and uc.MARGIN * uc.FLOOR <= bounds[k] < 1e-3, (case_id, k, bounds[k])
        # the TD gate is positive and the fp32 run is inside its own floor term
        gate = uc.td_gate(g, case_id)
        assert (gate >= uc.vc.CHAIN_FLOOR).all()
        assert (np.abs(g[f"{case_id}.td32"] - g[f"{case_id}.td64"]) <= 0.5 * gate).all()


# ---------------------------------------------------------------- sensitivity
# `soft_update_first` is no error: `update_pi` writes `_pi` alone and reads the online Q parameters, the lerp reads the online Q
# parameters and writes the target ones, so the two commute and the run is the verbatim one bit for bit.  The fixture
# keeps it as the control of the controls: a variant that changes nothing must measure exactly 0.
COMMUTES = ("soft_update_first",)


def test_every_control_is_far_from_the_verbatim_run(g, cfgs):
    best = {}
    for case_id in uc.CASES:
        cfg = cfgs[case_id]
        keys = uc.info_keys(cfg)
        for control in uc.controls_of(cfg):
            r, where = uc.control_margin(g, case_id, control, keys)
            print(f"{control:18s} {case_id:15s} {r:12.4g} bounds at {where}")
            if r > best.get(control, (-1.0,))[0]:
                best[control] = (r, case_id, where)
    assert set(best) == set(uc.CONTROLS)
    for control, (r, case_id, where) in best.items():
        print(f"{control}: {r:.4g} bounds ({case_id}, {where})")
        if control in COMMUTES:
            for c in uc.CASES:
                assert np.array_equal(g[f"{c}.{control}.info64"], g[f"{c}.info64"]) and np.array_equal(g[f"{c}.{control}.td64"], g[f"{c}.td64"])
        else:
            assert r >= uc.SENSITIVITY, (control, r, case_id, where)
    # the remainder on the task embedding shows where the issue expects it: the model step of the iteration after
    keys = uc.info_keys(cfgs["tiny_mt-B12"])
    d = np.abs(g["tiny_mt-B12.no_emb_leak.info64"] - g["tiny_mt-B12.info64"])
    assert not d[0].any() and d[1, keys.index("grad_norm")] > 0
