"""GPU: the loss unit (tdmpc2_loss_forward / tdmpc2_loss_backward, autograd.model_loss, TDMPC2.update_model) against fp64.

Gates (tests/loss_grad_common.py: gate): e <= MARGIN * max(e_torch32, FLOOR) per tensor, e = max |T - T64| / max |T64|, e_torch32
torch's own fp32 autograd of the same expression on the CPU (for the fixture: the reference's own math, stored).
  measured gate   the fixture's inputs against its fp64 losses, step means and gradients
  pinned targets  the case table; reference and yardstick are given the same fp32 two-hot rows as constants, so the gate measures
                  the softmax and the seeds' arithmetic, not the rounding of `off`; worst ratios go to the file TDMPC2_LOSS_JSON names
                  (profiles/loss_grad_edges.json)
Exact checks compare bits.  No NaN target is ever given to torch: its expected values come from the numpy closed form."""
import json
import os

import numpy as np
import pytest
import torch

from tests import loss_grad_common as lc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = 8  # floats in front of and behind every output
SENTINEL = -777.25


def _merge_json(key, value):
    path = os.environ.get("TDMPC2_LOSS_JSON")
    if not path:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.setdefault("gate", "e <= 4 * max(e_torch32, 2^-23) per tensor, e = max |T - T64| / max |T64|")
    doc[key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def _shapes(case):
    T, B, L, NB, Q = case["T"], case["B"], case["L"], case["NB"], case["Q"]
    s = dict(d_z_pred=(T, B, L), d_reward_logits=(T, B, NB), d_q_logits=(Q, T, B, NB), losses=(5,), step_means=(4, T))
    if case["episodic"]:
        s["d_term_logit"] = (T, B)
    return s


class Rig:
    """The inputs of a case on the device, guarded outputs, one forward + backward."""

    def __init__(self, case, x, h=None):
        from tdmpc2_amd import native

        self.case, self.h = case, h or lc.hyper(case["NB"])
        self.desc = native.loss_desc(case["T"], case["B"], case["L"], case["Q"], case["NB"], case["episodic"],
                                     **{k: self.h[k] for k in lc.HYPER_KEYS})
        self.set_inputs(x)
        self.ws = torch.empty(native.loss_workspace_bytes(self.desc), dtype=torch.uint8, device=DEV)
        self.buf = {k: torch.full((int(np.prod(s)) + 2 * GUARD,), SENTINEL, device=DEV) for k, s in _shapes(case).items()}
        self.out = {k: self.buf[k][GUARD:-GUARD] for k in self.buf}

    def set_inputs(self, x):
        self.ins = [None if k not in x else torch.tensor(x[k], device=DEV).contiguous() for k in lc.INPUTS]

    def forward(self, step_means=True):
        from tdmpc2_amd import native

        native.loss_forward(self.desc, *self.ins, losses=self.out["losses"], step_means=self.out["step_means"] if step_means else None,
                            ws=self.ws)

    def backward(self, g=None, want=lc.SEEDS):
        from tdmpc2_amd import native

        outs = {k: (self.out[k] if k in want and k in self.out else None) for k in lc.SEEDS}
        native.loss_backward(self.desc, *self.ins, grad_total=g, **outs)

    def run(self, g=None, want=lc.SEEDS):
        self.forward()
        self.backward(g, want)
        return self.read()

    def read(self):
        torch.cuda.synchronize()
        for k, b in self.buf.items():
            edge = torch.cat([b[:GUARD], b[-GUARD:]]).cpu().numpy()
            assert (edge == np.float32(SENTINEL)).all(), f"guard floats around {k} were written"
        return {k: v.cpu().numpy().reshape(_shapes(self.case)[k]).copy() for k, v in self.out.items()}


def _bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ---------------------------------------------------------------- measured gates
def test_measured_gate_against_the_fixture():
    z = np.load(lc.GOLDEN)
    h = dict(zip(lc.HYPER_KEYS, (float(v) for v in z["hyper"])))
    x = {k: z[k] for k in lc.INPUTS}
    got = Rig(lc.FIXTURE_CASE, x, h).run()
    worst = {}
    for k in ("losses", "step_means") + lc.SEEDS:
        e, bound = lc.gate(got[k], z[k + "_64"], z[k + "_32"])
        worst[k] = round(e / (bound / lc.MARGIN), 3)
        print(f"fixture {k}: e {e:.3e} bound {bound:.3e} ratio {worst[k]}")
    _merge_json("fixture", worst)
    for k, r in worst.items():
        assert r <= lc.MARGIN, (k, r)


@pytest.fixture(scope="module")
def pinned_worst():
    worst = {}
    yield worst
    if worst:
        _merge_json("pinned_targets", {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("name", [c["name"] for c in lc.CASE_LIST])
def test_pinned_target_gate(name, pinned_worst):
    case = lc.CASES[name]
    h = lc.hyper(case["NB"])
    x = lc.make_inputs(case)
    th = lc.pinned_rows(x, case, h)
    ref = lc.torch_ref(x, case, h, torch.float64, th)
    yard = lc.torch_ref(x, case, h, torch.float32, th)
    got = Rig(case, x, h).run()
    fails = []
    for k in ("losses", "step_means") + lc.SEEDS:
        if k not in ref:
            continue
        e, bound = lc.gate(got[k], ref[k], yard[k])
        ratio = e / (bound / lc.MARGIN)
        pinned_worst[k] = max(pinned_worst.get(k, 0.0), ratio)
        print(f"{name} {k}: e {e:.3e} bound {bound:.3e} ratio {ratio:.3f}")
        if ratio > lc.MARGIN:
            fails.append((k, e, bound))
    assert not fails, fails


# ---------------------------------------------------------------- exact checks
def test_grad_total_zero_coefficients_and_null_outputs():
    case = lc.CASES["mid"]
    x = lc.make_inputs(case)
    rig = Rig(case, x)
    one = rig.run(g=torch.ones(1, device=DEV))
    null = rig.run(g=None)
    two = rig.run(g=torch.full((1,), 2.0, device=DEV))
    for k in lc.SEEDS:
        assert _bits(null[k], one[k]), k
        assert _bits(two[k], np.float32(2) * one[k]), k
    assert all(_bits(null[k], one[k]) for k in ("losses", "step_means"))
    # an output that is NULL is not computed and the others keep their bits
    for want in (("d_z_pred",), ("d_q_logits", "d_term_logit"), ("d_reward_logits",)):
        r2 = Rig(case, x)
        part = r2.run(want=want)
        for k in lc.SEEDS:
            if k in want:
                assert _bits(part[k], one[k]), (want, k)
            else:
                assert (part[k] == np.float32(SENTINEL)).all(), (want, k)
    # zero coefficients: seeds of exactly +-0
    h0 = dict(lc.hyper(case["NB"]), reward_coef=0.0, consistency_coef=0.0)
    z = Rig(case, x, h0).run()
    assert not z["d_reward_logits"].any() and not z["d_z_pred"].any()
    assert _bits(z["d_q_logits"], one["d_q_logits"]) and _bits(z["d_term_logit"], one["d_term_logit"])


def test_rows_do_not_depend_on_other_rows():
    case = lc.CASES["flag"]
    x = lc.make_inputs(case)
    a = Rig(case, x).run()
    y = lc.make_inputs(case, seed=3)
    t, b = 1, 17

    def row(v):  # [..., T, B, width] or [T, B]
        return v[..., t, b, :] if v.ndim >= 3 else v[t:t + 1, b]

    for k in lc.INPUTS:
        row(y[k])[...] = row(x[k])
    got = Rig(case, y).run()
    for k in lc.SEEDS:
        assert _bits(row(got[k]), row(a[k])), k
        assert not _bits(got[k], a[k]), k


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    case = lc.CASES["five"]
    x = lc.make_inputs(case)
    rig = Rig(case, x)
    g = torch.full((1,), 0.75, device=DEV)
    a = rig.run(g=g)
    for b in rig.buf.values():
        b[GUARD:-GUARD] = 0
    b2 = rig.run(g=g)
    assert all(_bits(a[k], b2[k]) for k in a)
    for b in rig.buf.values():
        b[GUARD:-GUARD] = 0
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):  # forward + backward capture as they are: no allocation, no host sync
            rig.forward()
            rig.backward(g)
    graph.replay()
    c = rig.read()
    assert all(_bits(a[k], c[k]) for k in a)


def test_one_nan_reward_poisons_its_row_and_its_loss_only():
    case = lc.CASES["mid"]
    h = lc.hyper(case["NB"])
    x = lc.make_inputs(case)
    clean = Rig(case, x).run()
    x2 = {k: v.copy() for k, v in x.items()}
    x2["reward"][1, 7] = np.nan
    bad = Rig(case, x2).run()
    want = lc.closed_form(x2, case, h, np.float32)  # where the NaNs must be
    for k in ("losses", "step_means") + lc.SEEDS:
        assert np.array_equal(np.isnan(bad[k]), np.isnan(want[k])), k
        keep = ~np.isnan(want[k])
        assert _bits(bad[k][keep], clean[k][keep]), k
    assert np.isnan(bad["d_reward_logits"][1, 7]).all() and np.isnan(bad["d_reward_logits"]).sum() == case["NB"]
    assert np.isnan(bad["losses"]).tolist() == [False, True, False, False, True]
    assert np.isnan(bad["step_means"]).sum() == 1 and np.isnan(bad["step_means"][1, 1])
    # +-Inf targets clamp to vmin / vmax: the seeds of +-1e5
    x3 = {k: v.copy() for k, v in x.items()}
    x3["td_target"][0, 0], x3["td_target"][0, 1] = np.inf, -np.inf
    x4 = {k: v.copy() for k, v in x.items()}
    x4["td_target"][0, 0], x4["td_target"][0, 1] = 1e5, -1e5
    assert all(_bits(u, v) for u, v in zip(Rig(case, x3).run().values(), Rig(case, x4).run().values()))


# ---------------------------------------------------------------- against the library's forward and under autograd
def _tiny_agent(episodic=False, name="tiny"):
    from tdmpc2_amd import TDMPC2
    from tdmpc2_amd.config import named_config

    cfg = named_config(name, dropout=0.0, episodic=episodic)
    torch.manual_seed(9)
    agent = TDMPC2(cfg, device=DEV)
    with torch.no_grad():  # away from the init's zero biases and unit gains
        for n, p in agent.model.named_parameters():
            p.add_(torch.randn_like(p) * (0.1 if n.endswith("weight") and p.dim() >= 2 else 0.2))
    agent.native_autograd = True
    return cfg, agent


def _update_batch(cfg, B=33, dtype=torch.float32, device=DEV):
    rng = np.random.default_rng(21)
    H = cfg.horizon
    t = lambda a: torch.tensor(a, dtype=dtype, device=device)  # noqa: E731
    return dict(obs=t(rng.standard_normal((H + 1, B, cfg.obs_shape["state"][0]))), action=t(np.tanh(rng.standard_normal((H, B, cfg.action_dim)))),
                reward=t(np.sinh(rng.uniform(-3, 3, (H, B, 1)))), terminated=t((rng.random((H, B, 1)) < 0.3).astype(np.float64)),
                td=t(np.sinh(rng.uniform(-5, 5, (H, B, 1)))))


def _case_of(cfg, B):
    return dict(T=cfg.horizon, B=B, L=cfg.latent_dim, NB=cfg.num_bins, Q=cfg.num_q, episodic=bool(cfg.episodic))


def _hyper_of(cfg):
    return lc.hyper(cfg.num_bins, cfg.vmin, cfg.vmax, cfg.rho, (cfg.consistency_coef, cfg.reward_coef, cfg.value_coef, cfg.termination_coef))


@pytest.mark.parametrize("episodic", [False, True])
def test_cross_check_with_model_losses(episodic):
    """The logits of model_rollout through tdmpc2_loss_forward, beside model_losses_latent on the same batch; both against fp64 of
    the same logits, yardstick torch's fp32 of them."""
    cfg, agent = _tiny_agent(episodic)
    B = 33
    bt = _update_batch(cfg, B)
    with torch.no_grad():
        z0 = agent.model.encode(bt["obs"][0], None).contiguous()
        next_z = agent.model.encode(bt["obs"][1:], None).contiguous()
    want = ("zs", "reward_logits", "q_logits") + (("term_logit",) if episodic else ())
    ro = agent.model_rollout(z0, bt["action"], want=want)
    x = dict(z_pred=ro["zs"][1:], next_z=next_z, reward_logits=ro["reward_logits"], reward=bt["reward"][..., 0], q_logits=ro["q_logits"],
             td_target=bt["td"][..., 0])
    if episodic:
        x.update(term_logit=ro["term_logit"][1:, :, 0], terminated=bt["terminated"][..., 0])
    x = {k: v.contiguous().cpu().numpy() for k, v in x.items()}
    case, h = _case_of(cfg, B), _hyper_of(cfg)
    ref, yard = lc.closed_form(x, case, h, np.float64), lc.torch_ref(x, case, h, torch.float32)
    got = Rig(case, x, h).run()
    ml = agent.model_losses_latent(z0, next_z, bt["action"], bt["reward"], bt["td"], bt["terminated"] if episodic else None, step_means=True)
    ml_losses = np.asarray([float(ml[k]) for k in ("consistency_loss", "reward_loss", "value_loss", "termination_loss", "total_loss")])
    for i, name in enumerate(("consistency", "reward", "value", "termination", "total")):
        if ref["losses"][i] == 0:
            assert got["losses"][i] == 0 and ml_losses[i] == 0
            continue
        et = max(abs(yard["losses"][i] - ref["losses"][i]) / abs(ref["losses"][i]), lc.FLOOR)
        e, e_ml = (abs(v - ref["losses"][i]) / abs(ref["losses"][i]) for v in (got["losses"][i], ml_losses[i]))
        print(f"{name}: loss unit {e / et:.3f}, model_losses {e_ml / et:.3f} (x max(e_torch32, 2^-23))")
        assert e <= lc.MARGIN * et and e_ml <= lc.MARGIN * et, (name, e, e_ml, et)
    e, bound = lc.gate(got["step_means"], ref["step_means"], yard["step_means"])
    assert e <= bound
    assert lc.rel_err(ml["step_means"].cpu().numpy(), ref["step_means"]) <= bound


def _rollout_loss(model, cfg, bt, loss_fn):
    """The model half of _update up to the total, on `model` (any device / dtype): two-step rollout, then loss_fn."""
    z = model.encode(bt["obs"][0], None)
    with torch.no_grad():
        next_z = model.encode(bt["obs"][1:], None)
    zs = [z]
    for t in range(cfg.horizon):
        z = model.next(z, bt["action"][t], None)
        zs.append(z)
    _zs, z_pred = torch.stack(zs[:-1]), torch.stack(zs[1:])
    T, B = bt["action"].shape[:2]  # (the module path of the Q ensemble takes rows: [T * B, .])
    qs = model.Q(_zs.reshape(T * B, -1), bt["action"].reshape(T * B, -1), None, return_type="all").reshape(cfg.num_q, T, B, -1)
    rp = model.reward(_zs, bt["action"], None)
    tp = model.termination(z_pred, None, unnormalized=True) if cfg.episodic else None
    return loss_fn(z_pred, next_z, rp, bt["reward"], qs, bt["td"], tp, bt["terminated"] if cfg.episodic else None)


def _torch_loss_fn(cfg, B):
    case, h = _case_of(cfg, B), _hyper_of(cfg)

    def fn(z_pred, next_z, rp, reward, qs, td, tp, terminated):
        sq = lambda v: None if v is None else v[..., 0]  # noqa: E731
        losses, _ = lc.torch_total(z_pred, next_z, rp, sq(reward), qs, sq(td), sq(tp), sq(terminated), case, h)
        return losses
    return fn


def _cpu_model(cfg, start, dtype):
    from tdmpc2_amd.world_model import WorldModel

    m = WorldModel(cfg)
    with torch.no_grad():
        for p, q in zip(m.parameters(), start):
            p.copy_(q)
    return m.to(dtype=dtype)


@pytest.mark.parametrize("episodic", [False, True])
def test_parameter_gradients_through_model_loss(episodic, monkeypatch):
    from tdmpc2_amd import autograd, native

    cfg, agent = _tiny_agent(episodic)
    B = 33
    start = [p.detach().cpu().clone() for p in agent.model.parameters()]
    grads = {}
    for tag, dtype in (("ref", torch.float64), ("yard", torch.float32)):
        m = _cpu_model(cfg, start, dtype)
        m.train()
        _rollout_loss(m, cfg, _update_batch(cfg, B, dtype, "cpu"), _torch_loss_fn(cfg, B))[4].backward()
        grads[tag] = {n: p.grad.numpy().copy() for n, p in m.named_parameters() if p.grad is not None}
    agent.model.train()
    calls0 = native.LOSS_CALLS
    total, parts = _rollout_loss(agent.model, cfg, _update_batch(cfg, B), lambda *a: autograd.model_loss(cfg, *a))
    total.backward()
    assert native.LOSS_CALLS - calls0 == 2 and parts.shape == (4,) and not parts.requires_grad and total.dim() == 0
    used = {n for n, p in agent.model.named_parameters() if not n.startswith("_pi.")}
    assert set(grads["ref"]) == used
    worst = 0.0
    for n, p in agent.model.named_parameters():
        if n not in used:
            assert p.grad is None or not p.grad.any(), n
            continue
        e, bound = lc.gate(p.grad.cpu().numpy(), grads["ref"][n], grads["yard"][n])
        worst = max(worst, e / (bound / lc.MARGIN))
        assert e <= bound, (n, e, bound)
    print("worst parameter-gradient ratio", round(worst, 3))
    _merge_json(f"autograd_{'episodic' if episodic else 'plain'}", round(worst, 3))
    # an input without requires_grad gets a NULL output
    seen = []
    real = native.loss_backward
    monkeypatch.setattr(native, "loss_backward", lambda *a, **k: (seen.append({n: v is not None for n, v in k.items()}), real(*a, **k))[1])
    case = _case_of(cfg, 5)
    x = {k: torch.tensor(v, device=DEV) for k, v in lc.make_inputs(dict(case, scale=1.0)).items()}
    x["reward_logits"].requires_grad_(True)
    args = [x.get(k) for k in lc.INPUTS]
    total, _ = autograd.model_loss(cfg, *args)
    (total * 3.0).backward()
    assert seen and seen[-1]["d_reward_logits"] and not seen[-1]["d_z_pred"] and not seen[-1]["d_q_logits"] and not seen[-1]["d_term_logit"]
    ref = lc.closed_form({k: v.detach().cpu().numpy() for k, v in x.items()}, case, _hyper_of(cfg), np.float64, g=3.0)
    assert lc.rel_err(x["reward_logits"].grad.cpu().numpy(), ref["d_reward_logits"]) <= 1e-4 and x["z_pred"].grad is None


# ---------------------------------------------------------------- update_model
KEYS = ("consistency_loss", "reward_loss", "value_loss", "termination_loss", "total_loss", "grad_norm")


@pytest.mark.parametrize("episodic", [False, True])
def test_update_model_against_a_torch_only_path(episodic):
    """Three steps on one batch with fixed td_targets.  Reference: the modules, the torch losses, clip_grad_norm_ and Adam (widened fp32
    hyperparameters) in fp64 on the CPU; yardstick: the same path in fp32.  Gated per step: the five losses and grad_norm."""
    from tests import optim_common as oc

    cfg, agent = _tiny_agent(episodic)
    B, steps = 33, 3
    start = [p.detach().cpu().clone() for p in agent.model.parameters()]

    def torch_path(dtype):
        m = _cpu_model(cfg, start, dtype)
        bt = _update_batch(cfg, B, dtype, "cpu")
        groups = [{"params": list(m._encoder.parameters()), "lr": oc.widen(cfg.lr * cfg.enc_lr_scale)}] + \
                 [{"params": list(x.parameters())} for x in (m._dynamics, m._reward, m._termination if episodic else None, m._Qs) if x is not None]
        ps = [p for g in groups for p in g["params"]]
        opt = torch.optim.Adam(groups, lr=oc.widen(cfg.lr), betas=(oc.widen(0.9), oc.widen(0.999)), eps=oc.widen(1e-8))
        out = []
        for _ in range(steps):
            m.train()
            losses = _rollout_loss(m, cfg, bt, _torch_loss_fn(cfg, B))
            losses[4].backward()
            norm = torch.nn.utils.clip_grad_norm_(ps, oc.widen(cfg.grad_clip_norm))
            opt.step()
            opt.zero_grad()
            out.append([float(v.detach()) for v in losses] + [float(norm)])
        return out

    ref, t32 = torch_path(torch.float64), torch_path(torch.float32)
    bt = _update_batch(cfg, B)
    agent.planner()  # the handle exists: the step re-packs it
    got = []
    for _ in range(steps):
        info = agent.update_model(bt["obs"], bt["action"], bt["reward"], bt["terminated"] if episodic else None, td_targets=bt["td"])
        assert set(info) == set(KEYS) and all(v.dim() == 0 and v.is_cuda for v in info.values())
        got.append([float(info[k]) for k in KEYS])
    assert not agent.model.training
    worst = dict.fromkeys(KEYS, 0.0)
    fails = []
    for s in range(steps):
        for i, k in enumerate(KEYS):
            if ref[s][i] == 0:
                assert got[s][i] == 0, (s, k)
                continue
            e, et = abs(got[s][i] - ref[s][i]) / abs(ref[s][i]), abs(t32[s][i] - ref[s][i]) / abs(ref[s][i])
            ratio = e / max(et, lc.FLOOR)
            worst[k] = max(worst[k], ratio)
            print("step", s, k, "lib", got[s][i], "ref64", ref[s][i], "e", e, "e_torch32", et, "ratio", round(ratio, 3))
            if ratio > lc.MARGIN:
                fails.append((s, k, e, et, ratio))
    _merge_json(f"update_model_{'episodic' if episodic else 'plain'}", {k: round(v, 3) for k, v in worst.items()})
    assert not fails, fails


def test_update_model_repacks_the_planner_and_uses_the_library_td_target():
    from tdmpc2_amd.native import NativeError, NativePlanner

    cfg, agent = _tiny_agent()
    bt = _update_batch(cfg, 12)
    agent.planner()
    before = agent.planner().export_packed()
    H, B = bt["action"].shape[:2]
    pi_eps = torch.randn(H, B, cfg.action_dim, device=DEV)
    qidx = torch.tensor([2, 0], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        next_z = agent.model.encode(bt["obs"][1:], None)
    expect = agent._td_target(next_z, bt["reward"], torch.zeros_like(bt["reward"]), None, pi_eps=pi_eps, qidx=qidx)
    agent.update_model(bt["obs"], bt["action"], bt["reward"], pi_eps=pi_eps, qidx=qidx)
    assert agent.last_td_targets.shape == (H, B, 1) and torch.equal(agent.last_td_targets, expect)
    after = agent.planner().export_packed()
    A = NativePlanner(agent.cfg, agent.cfg.iterations, DEV, max_envs=1, log_std_min=agent._planner_log_std[0],
                      log_std_dif=agent._planner_log_std[1])
    sd = {k: v for k, v in agent.model.state_dict().items() if torch.is_tensor(v)}
    A.bind_state_dict(sd)
    A.bind_encoder(sd)
    assert after == A.export_packed() and after != before
    A.close()
    agent.native_autograd = False
    with pytest.raises(NativeError, match="native_autograd"):
        agent.update_model(bt["obs"], bt["action"], bt["reward"], td_targets=bt["td"])
