"""CPU: the fixtures tests/golden/policy_loss_<case>.npz (tools/make_policy_loss_golden.py), regenerated bit for bit where the
reference tree is present, and the numpy restatement of tests/policy_loss_common.py that the GPU test leans on: percentiles bit
for bit and the lerped scale within 2 fp32 ulp of the reference's own RunningScale (torch's lerp_ and s + tau (v - s) can differ by
one ulp), the loss assembly against the stored scalars, NaN placement, and termination_statistics at the edges of sigmoid > 0.5."""
import os

import numpy as np
import pytest

from tests import policy_loss_common as pc


def _cfg(name):
    from oracle import cases

    return cases.build_case(name)["cfg"]


@pytest.mark.parametrize("name", pc.CASES)
def test_fixture_layout(name):
    assert os.path.getsize(pc.path(name)) <= 400 * 1024
    g = pc.golden(name)
    cfg = _cfg(name)
    T, A = cfg.horizon + 1, cfg.action_dim
    shapes = {"action": (T, pc.B_FULL, A), "q": (T, pc.B_FULL, 1), "entropy": (T, pc.B_FULL, 1), "scaled_entropy": (T, pc.B_FULL, 1)}
    for k, shp in shapes.items():
        assert g[f"b{pc.B_FULL}.{k}"].shape == shp and g[f"b{pc.B_FULL}.{k}"].dtype == np.float32
        # the reference's own round-off: 1 - a^2 cancels in fp32 where the squashed action saturates (c2, A = 38: 0.035 on
        # entropies of -150), so it is only required to be a small fraction of the field
        assert 0 <= float(g[f"b{pc.B_FULL}.{k}_d64"]) < 1e-3 * max(1.0, float(np.abs(g[f"b{pc.B_FULL}.{k}"]).max()))
    for B in (pc.B_FULL, pc.B_SMALL):
        for s0 in pc.SCALES0:
            assert g[f"b{B}.s{s0}.loss"].shape == (4,) and g[f"b{B}.s{s0}.step_means"].shape == (3, T)
            assert g[f"b{B}.s{s0}.percentiles"].shape == (2,)
            for k in pc.SCALAR_FIELDS:
                v = g[f"b{B}.s{s0}.{k}"]
                assert np.isfinite(v).all() and 0 <= float(g[f"b{B}.s{s0}.{k}_d64"]) < 1e-3 * max(1.0, float(np.abs(v).max()))


@pytest.mark.parametrize("name", pc.CASES)
def test_generator_reproduces_the_fixture(name):
    from oracle import ref_runner

    if not ref_runner.available():
        pytest.skip("reference tree not available")
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_policy_loss_golden as gen

    g, new = pc.golden(name), gen.generate(name)
    assert set(g) == set(new)
    for k in g:
        assert np.array_equal(g[k], new[k], equal_nan=True), k


def test_scale_restatement_matches_the_reference_table():
    g = pc.golden(pc.SCALE_CASE)
    worst = 0
    for kind in pc.SCALE_KINDS:
        for n in pc.SCALE_NS:
            ref = g[f"scale.{kind}.{n}"]
            p, s = pc.scale_update(pc.scale_input(n, kind), 1.0)
            assert p[0].tobytes() == ref[0].tobytes() and p[1].tobytes() == ref[1].tobytes(), (kind, n, p, ref)
            worst = max(worst, pc.ulp_diff(s, ref[2]))
            assert pc.ulp_diff(s, ref[2]) <= 2, (kind, n, s, ref[2])
    print(f"scale after the lerp: worst {worst} ulp over {len(pc.SCALE_KINDS) * len(pc.SCALE_NS)} combinations")


def test_scale_edges():
    assert pc.scale_update(np.array([3.25], np.float32), 1.0)[1] == np.float32(1.0)   # n = 1: both percentiles x[0], v = 1
    p, s = pc.scale_update(np.array([-4.0, 6.0], np.float32), 1.0)                    # n = 2: 0.05 and 0.95 of the way
    assert np.allclose(p, [-3.5, 5.5], rtol=1e-6) and s == np.float32(1.0 + 0.01 * 8.0)


def test_nan_placement():
    g = pc.golden(pc.SCALE_CASE)
    p, s = pc.scale_update(pc.nan_input(16), 1.0)    # position 0.95 x 15 = 14.25: its ceiling is the NaN sorted last
    assert np.isnan(s) and np.isnan(g["scale.nan.16"][2])
    p, s = pc.scale_update(pc.nan_input(256), 1.0)   # 0.95 x 255 = 242.25: the NaN at sorted index 255 is never touched
    assert np.isfinite(s) and p.tobytes() == g["scale.nan.256"][:2].tobytes() and pc.ulp_diff(s, g["scale.nan.256"][2]) <= 2


@pytest.mark.parametrize("name", pc.CASES)
def test_loss_restatement_matches_the_stored_scalars(name):
    g, cfg = pc.golden(name), _cfg(name)
    B = pc.B_FULL
    q, ent, sent = (g[f"b{B}.{k}"] for k in ("q", "entropy", "scaled_entropy"))
    for s0 in pc.SCALES0:
        p, s = pc.scale_update(q[0], s0)
        assert p.tobytes() == g[f"b{B}.s{s0}.percentiles"].tobytes()
        assert pc.ulp_diff(s, g[f"b{B}.s{s0}.loss"][3]) <= 2
        loss, sm = pc.loss_from(q, ent, sent, g[f"b{B}.s{s0}.loss"][3], cfg.rho, cfg.entropy_coef, np.float64)
        assert (np.abs(loss - g[f"b{B}.s{s0}.loss"]) <= pc.tol(loss, g[f"b{B}.s{s0}.loss_d64"])).all()
        assert (np.abs(sm - g[f"b{B}.s{s0}.step_means"]) <= pc.tol(sm, g[f"b{B}.s{s0}.step_means_d64"])).all()


def test_termination_restatement():
    # fp32 sigmoid(1e-8) == 0.5: not a predicted termination, although x > 0
    assert pc.sigmoid32(1e-8) == np.float32(0.5) and pc.sigmoid32(3e-7) > np.float32(0.5)
    for x in pc.TERM_EDGE_XS:
        for y in pc.TERM_EDGE_YS:
            tp, fn, fp = pc.term_counts([x], [y])
            pred = bool(pc.sigmoid32(x) > np.float32(0.5))
            assert (tp, fn, fp) == (int(pred and y == 1), int(not pred and y == 1), int(pred and y == 0))
            rate, f1 = pc.term_stats(tp, fn, fp, y, 1)
            assert rate == np.float32(y) and (f1 == np.float32(1.0) if tp else f1 == 0)
    x, y = pc.term_input()
    tp, fn, fp = pc.term_counts(x, y)
    rate, f1 = pc.term_stats(tp, fn, fp, y.sum(), len(y))
    ref = pc.golden(pc.TERM_CASE)["term.stats"]
    assert pc.ulp_diff(rate, ref[0]) <= 1 and pc.ulp_diff(f1, ref[1]) <= 1
