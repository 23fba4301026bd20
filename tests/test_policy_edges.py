"""CPU: what tests/test_gpu_policy_edges.py stands on (tests/policy_edges_common.py) -- policy_common.fp64_pi agrees with
tdmpc2_amd.world_model.WorldModel.pi in double (1e-12) and in float (pc.GATE), the value probes hold the conditions they are named
for, the case list reaches the route edges its table claims (policy_route.h itself under g++: tests/policy_route_model.py), and the
numpy emulation of the kernels' summation order meets every case's gate on both routes (measured before any GPU run: DESIGN 3.4c)."""
import numpy as np
import pytest
import torch

from tests import encoder_common as ec
from tests import policy_common as pc
from tests import policy_edges_common as pe
from tests import policy_route_model as pr


@pytest.fixture(scope="module")
def route_lib(tmp_path_factory):
    return pr.build(tmp_path_factory.mktemp("policy_route"))


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("T", [0, 3])
def test_fp64_pi_agrees_with_world_model(T, monkeypatch):
    from tdmpc2_amd import checkpoint, synth
    from tdmpc2_amd.world_model import WorldModel

    cfg = pe.make_cfg(64, T, 96, 5)
    sd = synth.make_state_dict(cfg, seed=11)
    rng = np.random.default_rng(12)
    n, tasks = 6, None
    if T:  # a table nn.Embedding(max_norm=1) leaves alone in every precision; masks that differ by task
        tab = rng.standard_normal((pe.N_TASKS, T))
        tab = tab / np.linalg.norm(tab, axis=-1, keepdims=True) * rng.uniform(0.3, 0.9, (pe.N_TASKS, 1))
        sd["_task_emb.weight"] = (np.round(tab * 1024) / 1024).astype(np.float32)
        sd["_action_masks"] = (rng.random((pe.N_TASKS, cfg.action_dim)) < 0.7).astype(np.float32)
        sd["_action_masks"][:, 0] = 1.0
        tasks = np.asarray([2, 9, 16, 23, 0, 7])
    z = synth.make_latents(cfg, n, seed=13)
    eps = rng.standard_normal((n, cfg.action_dim)).astype(np.float32)
    wm = WorldModel(cfg).eval()
    wm.load_state_dict(checkpoint.convert_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}))
    monkeypatch.setattr(torch, "randn_like", lambda x, **kw: torch.as_tensor(eps).to(x.dtype).clone())
    task = None if tasks is None else torch.as_tensor(tasks)
    for dtype, tol in ((torch.float32, pc.GATE), (torch.float64, 1e-12)):
        wm = wm.to(dtype)
        with torch.no_grad():
            action, info = wm.pi(torch.as_tensor(z).to(dtype), task)
        got = dict(info, action=action)
        ref = pc.fp64_pi(cfg, sd, z, tasks, eps, dtype=dtype)
        for k in pe.OUTPUTS:
            assert got[k].dtype == dtype and ref[k].dtype == (np.float32 if dtype == torch.float32 else np.float64)
            err = np.abs(got[k].numpy().astype(np.float64) - ref[k])
            assert (err <= tol * np.maximum(1.0, np.abs(ref[k]))).all(), (k, dtype, err.max())
    if T:
        assert len({int(m.sum()) for m in sd["_action_masks"][tasks]}) > 1


# ------------------------------------------------------------------------------------------------ the cases
def test_cases_are_well_formed():
    assert len(set(pe.NAMES)) == len(pe.NAMES)
    for name in pe.NAMES:
        c = pe.case(name)
        assert c.n * c.A >= pe.MIN_ELEMENTS and c.L % 32 == 0 and c.M % 32 == 0 and 1 <= c.A <= 64
        assert max(c.in0, c.M) <= pe.POL_MAX_WIDTH and c.z.shape == (c.n, c.L) and c.eps.shape == (c.n, c.A)
        np.testing.assert_allclose(c.z.astype(np.float64).reshape(c.n, -1, 8).sum(-1), 1.0, atol=1e-6)   # a SimNorm output
        assert (c.z >= 0).all()
        if c.T:
            assert (c.mask[:, 0] == 1).sum() >= c.n - 2 and len({tuple(m) for m in c.mask}) > 1
            assert (np.linalg.norm(c.emb.astype(np.float64), axis=-1) < 1).all()
        a, b, g = pe.refs(c)
        for k in pe.OUTPUTS:
            assert np.isfinite(a[k]).all() and np.isfinite(b[k]).all() and g[k] >= pe.FACTOR * pe.FLOOR
    assert pe.REFUSED_BIND[0] + pe.REFUSED_BIND[1] == pe.POL_MAX_WIDTH + 1
    assert {9, 19, 49} <= set(pe.ROWS) and max(pe.ROWS) == pe.case(pe.ROW_FAMILY).n


def test_value_probes():
    for name in pe.PROBE_NAMES:
        c = pe.case(name)
        mu, lr = pe.probe_pre(c)
        assert not c.sd["_pi.2.weight"].any()
        assert np.array_equal(mu * 16, np.round(mu * 16)) and np.array_equal(lr * 16, np.round(lr * 16))   # exact in any order
        a, b, _ = pe.refs(c)
        ls = -10.0 + 6.0 * (np.tanh(lr) + 1.0)
        mask = np.ones((c.n, c.A)) if c.tasks is None else c.mask.astype(np.float64)
        x = mu[None] * mask + c.eps.astype(np.float64) * mask * np.exp(ls[None] * mask)
        live = mask > 0
        np.testing.assert_allclose(np.tanh(x), a["action"], atol=1e-15)
        assert (np.abs(a["entropy"]) >= 1.0).all(), name          # entropy = -log_prob
        assert lr.min() == -40.0
        if name == "head_inside":
            assert lr.max() == 40.0 and ls.max() == 2.0 and ls.min() == -10.0 and (np.abs(x) <= 3.0).all()
            zero = [r for r in range(c.n) if not c.eps[r].any()]
            assert len(zero) == 2 and np.array_equal(a["action"][zero], a["mean"][zero])
            assert {-1.0, 1.0, 0.5, -0.5, 0.125, -0.125} <= set(np.unique(c.eps).tolist())
        elif name == "head_saturated":
            assert lr.max() == 40.0 and (np.abs(x[live]) >= 20.0).all() and (np.abs(a["action"][live]) == 1.0).all()
            assert (np.abs(b["action"][live]) == 1.0).all() and (np.abs(c.eps) == 30.0).any()
            pats = {tuple(m) for m in mask.astype(int)}
            lane = np.arange(c.A)
            for want in (lane >= 0, lane == 0, lane % 2 == 0, lane < 63, lane < 0):
                assert tuple(want.astype(int)) in pats
            none = ~live.any(-1)
            assert none.sum() == 2 and (a["scaled_entropy"][none] == 0).all() and (b["scaled_entropy"][none] == 0).all()
            for k in ("action", "mean", "log_std"):
                assert (a[k][none] == 0).all()
        else:
            assert (np.abs(x) > 3.0).all() and (np.abs(x) < 20.0).all()
            assert (np.abs(x) < 5).any() and (np.abs(x) > 9.1).any() and ((np.abs(x) > 5) & (np.abs(x) < 9)).any()


def test_cases_reach_their_route_edges(route_lib):
    """The case list as a whole reaches what the issue's table claims: a later edit to it cannot quietly drop an edge."""
    R, idle, partial, empty, odd_share, per_thread, auto, lasts, head_wide, col_tail = set(), 0, 0, 0, 0, set(), set(), set(), 0, set()
    for name, rows in pe.runs():
        c = pe.case_spec(name)
        maxw = max(c.in0, c.M, 2 * c.A)
        kind = pr.route(route_lib, rows, c.in0, c.M, c.A, maxw, pr.AUTO)["kind"]
        auto.add((kind, "wide" if c.M > pe.POL_ROW_MAX_MLP else "narrow", "many" if rows > pe.POL_ROW_MAX_ROWS else "few"))
        assert pr.route(route_lib, rows, c.in0, c.M, c.A, maxw, pr.FORCE_ROW)["kind"] == pr.POL_ROW      # forced row runs every case
        per_thread.add(-(-c.M // pe.POL_THREADS))
        head_wide += 2 * c.A > c.M
        col_tail.add(2 * c.A % 64)
        ch = c.chunks(rows)
        if len(ch) > 1:
            lasts.add(ch[-1])
        for m in ch:
            r = pr.route(route_lib, m, c.in0, c.M, c.A, maxw, pr.FORCE_SPREAD)
            assert r["kind"] == pr.POL_SPREAD and r["launches"] == 6
            for g in (r["grids"][0], r["grids"][2], r["grids"][4]):
                R.add(g["R"])
                idle += g["R"] > m                              # a workgroup row wider than the rows there are
                partial += m > g["R"] and m % g["R"] != 0       # the last workgroup row holds fewer than R rows
                kq = -(-g["in"] // pe.POL_GEMV_WAVES)
                shares = [max(0, min(g["in"], w * kq + kq) - min(g["in"], w * kq)) for w in range(pe.POL_GEMV_WAVES)]
                assert sum(shares) == g["in"]
                empty += 0 in shares
                odd_share += any(s % 2 for s in shares)
    assert R == {1, 2, 4, 8} and idle and partial and empty and odd_share
    assert per_thread >= {1, 2, 3, 8} and head_wide and {2, 0, 10 % 64, 62, 66 % 64} <= col_tail
    assert {(pr.POL_ROW, "narrow", "few"), (pr.POL_SPREAD, "wide", "few"), (pr.POL_SPREAD, "narrow", "many")} <= auto
    assert {1, 3} <= lasts
    # the single cases the table names
    c = pe.case_spec("mt_33_96_A5")
    assert c.in0 == 33 and -(-33 // 8) == 5 and 7 * 5 >= 33 and c.chunks(19)[-1] == 3 and c.chunks(49)[-1] == 1 and c.chunks(257)[-1] == 1
    assert c.chunks(105)[-1] == 9 and c.chunks(9) == [9]
    assert pe.case_spec("mt_67_544_A63").chunks()[-1] == 3 and pe.case_spec("mt_101_480_A33").chunks()[-1] == 7
    assert pe.case_spec("s_32_512_A64").chunks()[-1] == 2 and pe.case_spec("mt_128_1056_A6").chunks()[-1] == 5
    assert -(-101 // 8) == 13 and -(-544 // 8) == 68 and 480 % 64 != 0


# ------------------------------------------------------------------------------------------------ the emulation
@pytest.mark.parametrize("name,rows", pe.runs())
def test_emulation_meets_every_gate(name, rows):
    c = pe.case(name)
    for route in ("row", "spread"):
        r = pe.ratios(c, pe.emulate(c, route, rows), rows)
        print(f"[{name} n={rows}] {route}: emulation err / gate " + " ".join(f"{k}={v:.2f}" for k, v in r.items()))
        assert max(r.values()) <= 1.0, (route, r)


def test_emulation_sees_a_dropped_tail():
    """The emulation is of the ORDER: with pol_layer's single tail dropped it leaves the gate by far (in0 = 33)."""
    c = pe.case(pe.ROW_FAMILY)
    real = ec._chains
    try:
        ec._chains = lambda x, wt, k0, k1: real(x, wt, k0, k0 + (k1 - k0) // 4 * 4)
        assert max(pe.ratios(c, pe.emulate(c, "row", 9), 9).values()) > 100
    finally:
        ec._chains = real
    assert max(pe.ratios(c, pe.emulate(c, "row", 9), 9).values()) <= 1.0
