"""-m gpu: tdmpc2_plan_policy_loss / running_scale / termination_stats (the forward of TDMPC2.update_pi, reference
tdmpc2/tdmpc2.py:208-239) against the reference-minted fixtures tests/golden/policy_loss_<case>.npz
(tools/make_policy_loss_golden.py) and the numpy restatement of tests/policy_loss_common.py.

Gates.  Fixture fields: max(1e-4 max(1, |v|), 2 x <field>_d64), the layer code's gate (tests/model_common.py: tol).  Percentiles
and scale: against the restatement fed the library's own q[0], bit for bit / 2 fp32 ulp.  The tail alone: against the fp64
restatement fed the library's own per-row outputs, max(1e-5 max(1, |v|), 2 x |restatement fp32 - fp64|).  Termination statistics:
1 fp32 ulp of the restatement.  The worst err / gate per item goes to profiles/policy_loss_parity.json.

Every case runs on the kernel families of policy_loss_common.PATHS (the fused cases on both) and in both arithmetics."""
import json
import os

import numpy as np
import pytest
import torch

from tests import policy_loss_common as pc
from tests.gpu_common import case_on_gpu, dev

pytestmark = pytest.mark.gpu

PRECS = [1, 2]  # exact-fp32 MFMA, f16x2 split
ERR_INVALID, ERR_UNSUPPORTED = 1, 2
_planners, _record = {}, {}


def _planner(name, prec, path=1):
    key = (name, prec, path)
    if key not in _planners:
        _planners[key] = case_on_gpu(name, path, prec)
    return _planners[key]


def d(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev())


def _kw(c, model, inp):
    cfg = c["cfg"]
    if not cfg.multitask:
        return {}
    emb = model.sd["_task_emb.weight"]
    norm = emb.norm(2, dim=-1, keepdim=True)
    emb = torch.where(norm > 1.0, emb * (1.0 / (norm + 1e-7)), emb)  # nn.Embedding(max_norm=1)
    return dict(task_emb_table=emb.to(dev()).contiguous(), act_mask_table=model.sd["_action_masks"].to(torch.float32).to(dev()).contiguous(),
                task_ids=d(inp["tasks"].astype(np.int32)))


def _call(name, prec, B, s0, want=pc.ROW_FIELDS + ("step_means", "percentiles"), update=True, T=None, eps=True, path=None):
    c, model, planner = _planner(name, prec, pc.PATHS[name][0] if path is None else path)
    cfg = c["cfg"]
    inp = pc.inputs(cfg, B)
    T = cfg.horizon + 1 if T is None else T
    scale = torch.full((1,), s0, device=dev())
    res = planner.policy_loss(d(inp["zs"][:T]), scale, rho=cfg.rho, entropy_coef=cfg.entropy_coef, tau=cfg.tau, update_scale=update,
                              pi_eps=d(inp["pi_eps"][:T]) if eps else None, qidx=d(inp["qidx"]), want=want, **_kw(c, model, inp))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}, float(scale.item())


def _note(item, prec, ratio):
    key = f"{item}/prec{prec}"
    _record[key] = max(_record.get(key, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    if _record:
        out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "policy_loss_parity.json")
        with open(out, "w") as f:
            json.dump({"worst_err_over_gate": dict(sorted(_record.items()))}, f, indent=1)
            f.write("\n")


def _check_scale(q0, s0, got_pct, got_scale):
    p, s = pc.scale_update(q0, s0)
    assert got_pct.tobytes() == p.tobytes(), (got_pct, p)
    assert pc.ulp_diff(got_scale, s) <= 2, (got_scale, s)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,path", [(n, p) for n in pc.CASES for p in pc.PATHS[n]])
def test_parity_with_the_reference(name, path, prec):
    g = pc.golden(name)
    for B in (pc.B_FULL, pc.B_SMALL):
        for s0 in pc.SCALES0:
            res, scale = _call(name, prec, B, s0, path=path)
            fields = [(k, f"b{B}.s{s0}.{k}") for k in ("loss", "step_means")]
            if B == pc.B_FULL:
                fields += [(k, f"b{B}.{k}") for k in pc.ROW_FIELDS]
            for k, gk in fields:
                err, gate = np.abs(res[k] - g[gk]), pc.tol(g[gk], g[gk + "_d64"])
                print(f"[{name} path {path} prec {prec} B {B} s0 {s0}] {k}: worst err / gate {(err / gate).max():.3f}")
                _note(f"parity/{name}/path{path}/{k}", prec, (err / gate).max())
                assert (err <= gate).all(), (k, float(err.max()), float(gate.min()))
            assert scale == res["loss"][3]
            _check_scale(res["q"][0], s0, res["percentiles"], res["loss"][3])


SHAPES = [(1, 0), (1, 8), (2, 3), (21, 2), (16, 3), (13, 4), (130, 3)]  # 63 / 64 / 65 rows around the 64-row tile among them


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("prec", PRECS)
def test_tail_alone(prec, path):
    c, model, planner = _planner("c1_ep", prec, path)
    cfg = c["cfg"]
    from tdmpc2_amd import synth

    for B, steps in SHAPES:
        T = steps + 1
        zs = synth.make_latents(cfg, T * B, seed=50 + B).reshape(T, B, cfg.latent_dim)
        scale = torch.full((1,), 7.5, device=dev())
        res = planner.policy_loss(d(zs), scale, rho=cfg.rho, entropy_coef=cfg.entropy_coef, tau=cfg.tau, seed=3,
                                  want=("q", "entropy", "scaled_entropy", "step_means", "percentiles"))
        torch.cuda.synchronize()
        res = {k: v.cpu().numpy() for k, v in res.items()}
        assert np.isfinite(res["q"]).all() and np.isfinite(res["entropy"]).all()
        _check_scale(res["q"][0], 7.5, res["percentiles"], res["loss"][3])
        args = (res["q"], res["entropy"], res["scaled_entropy"], res["loss"][3], cfg.rho, cfg.entropy_coef)
        l64, s64 = pc.loss_from(*args, np.float64)
        l32, s32 = pc.loss_from(*args, np.float32)
        for k, got, v64, v32 in (("loss", res["loss"], l64, l32), ("step_means", res["step_means"], s64, s32)):
            err, gate = np.abs(got - v64), pc.edge_gate(v64, v32)
            print(f"[tail prec {prec} B {B} steps {steps}] {k}: worst err / gate {(err / gate).max():.3f}")
            _note(f"tail/path{path}/{k}", prec, (err / gate).max())
            assert (err <= gate).all(), (B, steps, k, got, v64)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["tiny", "tiny_mt", "c1_ep", "mt5"])
def test_consistency_with_the_sibling_calls(name, prec):
    """action / q carry policy_value's bits (B = 12, and B = 21: 84 rows, a full 64-row tile and a tail); fewer outputs change no
    bit of the loss; entropy / scaled_entropy agree with tdmpc2_plan_pi (plain fp32 FMAs) within tests/policy_common.py's
    entropy_bound with its floor widened to 1e-4: max(1e-4 max(1, |v|), 2 x the reference's fp32-vs-fp64 distance) -- that distance
    is the fixture's <field>_d64 here (the policy fixture's per-row one belongs to other rows), hence at the fixture's B = 12."""
    c, model, planner = _planner(name, prec, pc.PATHS[name][0])
    cfg = c["cfg"]
    T = cfg.horizon + 1
    for B in (pc.B_FULL, 21):
        inp = pc.inputs(cfg, B)
        res, _ = _call(name, prec, B, 1.0)
        kw = _kw(c, model, inp)
        if cfg.multitask:
            kw["task_ids"] = kw["task_ids"].repeat(T)
        a, q = planner.policy_value(d(inp["zs"].reshape(T * B, -1)), pi_eps=d(inp["pi_eps"].reshape(T * B, -1)), qidx=d(inp["qidx"]), **kw)
        assert a.cpu().numpy().tobytes() == res["action"].tobytes() and q.cpu().numpy().tobytes() == res["q"].tobytes()
        few, _ = _call(name, prec, B, 1.0, want=())
        assert few["loss"].tobytes() == res["loss"].tobytes()
    B = pc.B_FULL
    inp = pc.inputs(cfg, B)
    res, _ = _call(name, prec, B, 1.0)
    kw = _kw(c, model, inp)
    planner.bind_policy({k: v for k, v in model.sd.items() if k.startswith("_pi.")})
    pkw = {}
    if cfg.multitask:
        ids = kw["task_ids"].repeat(T).long()
        pkw = dict(task_emb=kw["task_emb_table"][ids].contiguous(), act_mask=kw["act_mask_table"][ids].contiguous())
    _, info = planner.pi(d(inp["zs"].reshape(T * B, -1)), eps=d(inp["pi_eps"].reshape(T * B, -1)), **pkw)
    g = pc.golden(name)
    for k in ("entropy", "scaled_entropy"):
        ref = info[k].cpu().numpy().reshape(-1)
        err = np.abs(res[k].reshape(-1) - ref)
        assert (err <= pc.tol(ref, g[f"b{B}.{k}_d64"])).all(), (k, float(err.max()))


@pytest.mark.parametrize("prec", PRECS)
def test_pieces_of_the_layered_family(prec):
    """A c3 handle whose workspace holds 512 rows runs the 4 x 130 = 520 rows of a call as 512 + 8 -- a split inside step 3 -- and
    equals the handle that holds them all, bit for bit: with a tape, and with Philox (same seed, same call counter)."""
    from tdmpc2_amd.native import NativePlanner

    c, model, whole = _planner("c3", prec, 2)
    cfg = c["cfg"]
    assert cfg.num_samples == 512   # (`whole`: tests/gpu_common.py builds it with max_envs >= 2, 1 024 rows)
    pieces = NativePlanner(cfg, c["iterations"], dev(), max_envs=1, path=2, precision=prec)
    pieces.bind_state_dict(model.sd)
    B = pc.B_SMALL
    inp = pc.inputs(cfg, B)
    kw = _kw(c, model, inp)
    want = pc.ROW_FIELDS + ("step_means", "percentiles")
    for eps in (d(inp["pi_eps"]), None):
        for qidx in (d(inp["qidx"]), None):
            out = []
            for pl in (whole, pieces):
                pl.set_call_counter(77)
                scale = torch.full((1,), 7.5, device=dev())
                r = pl.policy_loss(d(inp["zs"]), scale, tau=cfg.tau, pi_eps=eps, qidx=qidx, seed=11, want=want, **kw)
                torch.cuda.synchronize()
                out.append({k: v.cpu().numpy() for k, v in r.items()})
            for k in out[0]:
                assert np.isfinite(out[0][k]).all() and out[0][k].tobytes() == out[1][k].tobytes(), (k, eps is None, qidx is None)
    pieces.close()


def test_scale_state_and_graph_replay():
    c, model, planner = _planner("c1_ep", 1)
    cfg = c["cfg"]
    B = pc.B_FULL
    kept, s_after = _call("c1_ep", 1, B, 7.5, update=False)
    assert s_after == 7.5 and kept["loss"][3] == np.float32(7.5)
    l64, _ = pc.loss_from(kept["q"], kept["entropy"], kept["scaled_entropy"], 7.5, cfg.rho, cfg.entropy_coef, np.float64)
    assert abs(kept["loss"][0] - l64[0]) <= 1e-5 * max(1.0, abs(l64[0]))
    # two eager calls against two replays of one captured call: the scale advances twice, the bits are equal
    inp = pc.inputs(cfg, B)
    zs, eps, qidx = d(inp["zs"]), d(inp["pi_eps"]), d(inp["qidx"])
    run = lambda scale: planner.policy_loss(zs, scale, tau=cfg.tau, pi_eps=eps, qidx=qidx, want=("percentiles",))
    s_e = torch.ones(1, device=dev())
    run(s_e)
    eager = run(s_e)
    torch.cuda.synchronize()
    s_g = torch.ones(1, device=dev())
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            captured = run(s_g)
        s_g.fill_(1.0)
        graph.replay()
        graph.replay()
    torch.cuda.synchronize()
    assert s_g.cpu().numpy().tobytes() == s_e.cpu().numpy().tobytes() and float(s_e) != 1.0
    assert captured["loss"].cpu().numpy().tobytes() == eager["loss"].cpu().numpy().tobytes()


def test_running_scale_table():
    _, _, planner = _planner("c1_ep", 1)
    g = pc.golden(pc.SCALE_CASE)
    table = [(f"scale.{kind}.{n}", pc.scale_input(n, kind)) for kind in pc.SCALE_KINDS for n in pc.SCALE_NS]
    table += [(f"scale.nan.{n}", pc.nan_input(n)) for n in (16, 256)]
    table += [("n16384", pc.scale_input(16384, "normal"))]
    for key, x in table:
        scale, pct = torch.ones(1, device=dev()), torch.zeros(2, device=dev())
        planner.running_scale(d(x), scale, tau=pc.TAU, percentiles=pct)
        torch.cuda.synchronize()
        p, s = pc.scale_update(x, 1.0)
        got_p, got_s = pct.cpu().numpy(), scale.cpu().numpy()[0]
        assert got_p.tobytes() == p.tobytes() or (np.isnan(p) == np.isnan(got_p)).all() and np.array_equal(p, got_p, equal_nan=True), (key, got_p, p)
        assert pc.ulp_diff(got_s, s) <= 2, (key, got_s, s)
        if key in g:
            assert np.array_equal(got_p, g[key][:2], equal_nan=True) and pc.ulp_diff(got_s, g[key][2]) <= 2, (key, got_s, g[key])
    assert np.isnan(pc.scale_update(pc.nan_input(16), 1.0)[1]) and np.isfinite(pc.scale_update(pc.nan_input(256), 1.0)[1])
    # the edges, stated directly: n = 1 gives both percentiles x[0], so v = 1 and a scale of 1 stays 1; n = 2 interpolates
    scale, pct = torch.ones(1, device=dev()), torch.zeros(2, device=dev())
    planner.running_scale(d(np.array([3.25], np.float32)), scale, tau=pc.TAU, percentiles=pct)
    assert scale.item() == 1.0 and pct.tolist() == [3.25, 3.25]
    planner.running_scale(d(np.array([6.0, -4.0], np.float32)), scale, tau=pc.TAU, percentiles=pct)
    assert np.allclose(pct.cpu().numpy(), [-3.5, 5.5], rtol=1e-6) and scale.item() == np.float32(np.float32(1) + np.float32(0.01) * np.float32(8))


def test_termination_stats():
    _, _, planner = _planner("c1_ep", 1)
    xs = np.array([x for x in pc.TERM_EDGE_XS for _ in pc.TERM_EDGE_YS], np.float32)
    ys = np.array([y for _ in pc.TERM_EDGE_XS for y in pc.TERM_EDGE_YS], np.float32)
    rows = [(xs[i:i + 1], ys[i:i + 1]) for i in range(len(xs))] + [(xs, ys), pc.term_input(), pc.term_input(257), pc.term_input(4097)]
    for x, y in rows:
        st = planner.termination_stats(d(x), d(y)).cpu().numpy()
        tp, fn, fp = pc.term_counts(x, y)
        rate, f1 = pc.term_stats(tp, fn, fp, y.sum(), len(y))
        assert pc.ulp_diff(st[0], rate) <= 1 and pc.ulp_diff(st[1], f1) <= 1, (x[:4], y[:4], st, rate, f1)
    x, y = pc.term_input()
    st = planner.termination_stats(d(x), d(y)).cpu().numpy()
    ref = pc.golden(pc.TERM_CASE)["term.stats"]
    assert pc.ulp_diff(st[0], ref[0]) <= 1 and pc.ulp_diff(st[1], ref[1]) <= 1


def test_refusals():
    import ctypes as C

    from tdmpc2_amd import native

    c, model, planner = _planner("c1_ep", 1)
    cfg = c["cfg"]
    lib, h = planner.lib, planner._h
    zs, scale, loss = torch.zeros(2, 4, cfg.latent_dim, device=dev()), torch.ones(1, device=dev()), torch.zeros(4, device=dev())
    pin = native.PolicyLossIn(rho=0.5, entropy_coef=1e-4, tau=0.01, update_scale=1)
    P = lambda t: C.c_void_p(t.data_ptr())
    call = lambda B, steps, z=P(zs), i=C.byref(pin), s=P(scale), l=P(loss), tt=None: lib.tdmpc2_plan_policy_loss_mt(
        h, B, steps, z, tt, None, None, 0, i, s, None, l, None)
    with torch.cuda.device(dev()):
        assert call(4, 1) == 0
        assert call(4, 1, z=None) == ERR_INVALID and call(4, 1, i=None) == ERR_INVALID
        assert call(4, 1, s=None) == ERR_INVALID and call(4, 1, l=None) == ERR_INVALID
        assert call(0, 1) == ERR_INVALID and call(4, -1) == ERR_INVALID and call(4, 9) == ERR_INVALID
        tt = native.TaskTables(task_ids=zs.data_ptr(), task_emb=zs.data_ptr(), act_mask=zs.data_ptr(), discount=None, n_tasks=1)
        assert call(4, 1, tt=C.byref(tt)) == ERR_INVALID   # tables on a single-task handle
        assert call(16385, 0) == ERR_UNSUPPORTED           # update_scale beyond the percentile kernel's n (refused before any read)
        x = torch.zeros(4, device=dev())
        rs = lambda n, xx=P(x), s=P(scale): lib.tdmpc2_plan_running_scale(h, n, xx, C.c_float(0.01), s, None, None)
        assert rs(4) == 0 and rs(0) == ERR_INVALID and rs(4, xx=None) == ERR_INVALID and rs(4, s=None) == ERR_INVALID
        assert rs(16385) == ERR_UNSUPPORTED
        ts = lambda n, a=P(x), b=P(x), o=P(loss): lib.tdmpc2_plan_termination_stats(h, n, a, b, o, None)
        assert ts(4) == 0 and ts(0) == ERR_INVALID and ts(4, a=None) == ERR_INVALID and ts(4, b=None) == ERR_INVALID and ts(4, o=None) == ERR_INVALID
        # multitask handle without tables (fused and layered)
        for nm in ("mt5", "tiny_mt"):
            _, _, pm = _planner(nm, 1, pc.PATHS[nm][0])
            zm = torch.zeros(2, 4, pm.cfg.latent_dim, device=dev())
            assert lib.tdmpc2_plan_policy_loss(pm._h, 4, 1, P(zm), None, None, 0, C.byref(pin), P(scale), None, P(loss), None) == ERR_INVALID
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["tiny", "tiny_mt", "c1_ep", "mt5"])
def test_python_boundary(name):
    from tdmpc2_amd.tdmpc2 import TDMPC2

    c, model, _ = _planner(name, 1, pc.PATHS[name][0])
    cfg = c["cfg"]
    agent = TDMPC2(cfg, device=dev())
    agent.load({k: torch.as_tensor(v) for k, v in c["sd"].items()})
    B = pc.B_FULL
    inp = pc.inputs(cfg, B)
    task = None if inp["tasks"] is None else torch.as_tensor(inp["tasks"])
    g = pc.golden(name)
    res = agent.policy_loss(torch.as_tensor(inp["zs"]), task, pi_eps=torch.as_tensor(inp["pi_eps"]), qidx=d(inp["qidx"]), want=("q",))
    got = np.array([float(res[k]) for k in ("pi_loss", "pi_entropy", "pi_scaled_entropy", "pi_scale")])
    ref = g[f"b{B}.s1.0.loss"]
    assert (np.abs(got - ref) <= pc.tol(ref, g[f"b{B}.s1.0.loss_d64"])).all()
    # (the tiny models' Q spread is below 1: clamp(min = 1) leaves their scale at 1)
    assert float(agent.scale.value) == float(res["pi_scale"])
    assert pc.ulp_diff(float(agent.scale.value), pc.scale_update(res["q"][0].cpu().numpy(), 1.0)[1]) <= 2
    # state_dict round trip with the reference's keys
    sd = agent.scale.state_dict()
    assert set(sd) == {"value", "percentiles"} and sd["percentiles"].tolist() == [5.0, 95.0]
    other = TDMPC2(cfg, device=dev())
    other.scale.load_state_dict({k: v.clone() for k, v in sd.items()})
    assert float(other.scale.value) == float(agent.scale.value)
    with pytest.raises(ValueError):
        other.scale.load_state_dict(dict(value=sd["value"], percentiles=torch.tensor([10.0, 90.0])))
    x = d(pc.scale_input(41, "normal"))
    before = float(other.scale.value)
    y = other.scale(x.reshape(-1, 1), update=True)
    _, s = pc.scale_update(pc.scale_input(41, "normal"), before)
    assert pc.ulp_diff(float(other.scale.value), s) <= 2 and torch.equal(y, x.reshape(-1, 1) / other.scale.value)
    # update_info: every key of the reference's _update dict except the two gradient norms
    rng = np.random.default_rng(3)
    H = cfg.horizon
    obs = torch.as_tensor(rng.standard_normal((H + 1, B, cfg.obs_shape["state"][0])).astype(np.float32))
    act = torch.as_tensor(rng.uniform(-1, 1, (H, B, cfg.action_dim)).astype(np.float32))
    rew = torch.as_tensor(rng.standard_normal((H, B, 1)).astype(np.float32))
    term = torch.as_tensor((rng.random((H, B, 1)) < 0.2).astype(np.float32)).to(dev())
    info = agent.update_info(obs, act, rew, term if cfg.episodic else None, task)
    keys = {"consistency_loss", "reward_loss", "value_loss", "termination_loss", "total_loss", "pi_loss", "pi_entropy",
            "pi_scaled_entropy", "pi_scale"}
    if cfg.episodic:
        keys |= {"termination_rate", "termination_f1"}
    assert set(info) == keys
    assert all(v.dim() == 0 and np.isfinite(float(v)) for v in info.values())
