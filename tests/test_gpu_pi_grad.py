"""GPU: the policy-loss unit (tdmpc2_pigrad_*, autograd.PiHeadFn / PiLossFn / pi_loss, WorldModel.pi's library tail, WorldModel.Q_pair,
TDMPC2.update_pi / _update / update) against fp64.

Gates (tests/pi_grad_common.py: gate): e <= MARGIN * max(e_torch32, FLOOR) per tensor, e = max |T - T64| / max |T64|, e_torch32
torch's own fp32 autograd of the same expression on the CPU (for the fixture: the reference's own code, stored).  Worst ratios go to
the file TDMPC2_PI_GRAD_JSON names (profiles/pi_grad_edges.json).  Exact checks compare bits.  +-Inf logits are out of scope."""
import json
import os

import numpy as np
import pytest
import torch

from tests import pi_grad_common as pc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = 8  # floats in front of and behind every output
SENTINEL = -777.25
OUTPUTS = pc.FORWARD + pc.SEEDS


def _merge_json(key, value):
    path = os.environ.get("TDMPC2_PI_GRAD_JSON")
    if not path:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.setdefault("gate", "e <= 4 * max(e_torch32, 2^-23) per tensor, e = max |T - T64| / max |T64|; values are e / max(e_torch32, 2^-23)")
    doc[key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def _shapes(case):
    T, B, A, NB = case["T"], case["B"], case["A"], case["NB"]
    return dict(action=(T, B, A), entropy=(T, B), scaled_entropy=(T, B), q=(T, B), losses=(3,), step_means=(T,),
                d_scaled_entropy=(T, B), d_q_logits=(2, T, B, NB), d_pi_out=(T, B, 2 * A))


class Rig:
    """The inputs of a case on the device, guarded outputs, the five calls chained as update_pi chains them."""

    def __init__(self, case, x, scale, h=None):
        from tdmpc2_amd import native

        self.case, self.h = case, h or pc.hyper()
        self.desc = native.pigrad_desc(case["T"], case["B"], case["A"], case["NB"], x.get("mask") is not None,
                                       **{k: self.h[k] for k in pc.HYPER_KEYS})
        self.scale = torch.tensor([scale], dtype=torch.float32, device=DEV)
        self.set_inputs(x)
        self.buf = {k: torch.full((int(np.prod(s)) + 2 * GUARD,), SENTINEL, device=DEV) for k, s in _shapes(case).items()}
        self.out = {k: self.buf[k][GUARD:-GUARD] for k in self.buf}

    def set_inputs(self, x):
        self.ins = {k: (None if x.get(k) is None else torch.tensor(x[k], device=DEV).contiguous()) for k in pc.INPUTS}

    def forward(self, step_means=True):
        from tdmpc2_amd import native

        i, o = self.ins, self.out
        native.pigrad_head_forward(self.desc, i["pi_out"], i["eps"], i["mask"], o["action"], o["entropy"], o["scaled_entropy"])
        native.pigrad_value_forward(self.desc, i["q_logits"], o["q"])
        native.pigrad_loss_forward(self.desc, o["q"], o["entropy"], o["scaled_entropy"], self.scale, o["losses"],
                                   o["step_means"] if step_means else None)

    def backward(self, g=None, want=("d_q_logits", "d_scaled_entropy"), d_action=True, d_se=True):
        from tdmpc2_amd import native

        i, o = self.ins, self.out
        native.pigrad_loss_backward(self.desc, i["q_logits"], self.scale, g, o["d_q_logits"] if "d_q_logits" in want else None,
                                    o["d_scaled_entropy"] if "d_scaled_entropy" in want else None)
        native.pigrad_head_backward(self.desc, i["pi_out"], i["eps"], i["mask"], i["d_action"] if d_action else None,
                                    o["d_scaled_entropy"] if d_se else None, o["d_pi_out"])

    def run(self, g=None):
        self.forward()
        self.backward(g)
        return self.read()

    def read(self):
        torch.cuda.synchronize()
        for k, b in self.buf.items():
            assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all()), f"guard floats of {k}"
        return {k: v.cpu().numpy().reshape(_shapes(self.case)[k]).copy() for k, v in self.out.items()}


def _gate_all(got, ref, yard, tag):
    worst, fails = {}, []
    for k in OUTPUTS:
        e, bound = pc.gate(got[k], ref[k], yard[k])
        worst[k] = round(e / (bound / pc.MARGIN), 3)
        print(tag, k, "e", e, "bound", bound, "ratio", worst[k])
        if not e <= bound:
            fails.append((k, e, bound))
    return worst, fails


@pytest.fixture(scope="module")
def golden():
    return np.load(pc.GOLDEN)


def _fixture_inputs(g, name):
    return {k: (g[f"{name}.{k}"] if f"{name}.{k}" in g.files else None) for k in pc.INPUTS}


# ---------------------------------------------------------------- 1. the measured gate on the fixture
@pytest.mark.parametrize("scale", pc.SCALES)
@pytest.mark.parametrize("name", list(pc.FIXTURE_CASES))
def test_measured_gate_on_the_fixture(golden, name, scale):
    case = pc.FIXTURE_CASES[name]
    got = Rig(case, _fixture_inputs(golden, name), scale).run()
    ref = {k: golden[f"{name}.s{scale}.{k}.f64"] for k in OUTPUTS}
    yard = {k: golden[f"{name}.s{scale}.{k}.f32"] for k in OUTPUTS}
    worst, fails = _gate_all(got, ref, yard, f"{name} s{scale}")
    _merge_json(f"fixture_{name}_s{scale}", worst)
    assert not fails, fails
    NB = case["NB"]
    assert not got["d_q_logits"].reshape(-1, NB)[1].any()  # one-hot on the centre bin: the seed is exactly 0
    # the loss from the rows the device wrote, in the published order of sums (pi_grad_route.h), bit for bit
    want_l, want_sm = pc.loss_model(got["q"], got["entropy"], got["scaled_entropy"], pc.hyper(), scale)
    assert _bits(got["losses"]) == _bits(want_l) and _bits(got["step_means"]) == _bits(want_sm)


# ---------------------------------------------------------------- 2. shape edges
@pytest.mark.parametrize("name", [c["name"] for c in pc.CASE_LIST])
def test_shape_edges_against_fp64_autograd(name):
    case, h, scale = pc.CASES[name], pc.hyper(), 2.5
    x = pc.make_inputs(case)
    ref, yard = pc.torch_ref(x, case, h, scale, torch.float64), pc.torch_ref(x, case, h, scale, torch.float32)
    got = Rig(case, x, scale, h).run()
    worst, fails = _gate_all(got, ref, yard, name)
    _merge_json(f"shape_{name}", worst)
    assert not fails, fails


# ---------------------------------------------------------------- 3. bit checks
def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def test_grad_total_two_one_and_null():
    case = pc.CASES["small"]
    x = pc.make_inputs(case)
    rig = Rig(case, x, 37.5)
    null = rig.run(None)
    one = rig.run(torch.ones(1, device=DEV))
    two = rig.run(torch.full((1,), 2.0, device=DEV))
    for k in ("d_q_logits", "d_scaled_entropy"):
        assert _bits(null[k]) == _bits(one[k]) and _bits(np.float32(2) * one[k]) == _bits(two[k]), k
    for k in pc.FORWARD:
        assert _bits(null[k]) == _bits(two[k]), k


def test_zero_entropy_coef_and_masked_columns():
    case = pc.CASES["masked"]
    x = pc.make_inputs(case)
    got = Rig(case, x, 1.0, dict(pc.hyper(), entropy_coef=0.0)).run()
    assert not got["d_scaled_entropy"].any()  # exactly +-0
    A = case["A"]
    got = Rig(case, x, 1.0).run()
    dead = np.broadcast_to(x["mask"][None] == 0, got["action"].shape)
    assert dead.any() and not got["d_pi_out"][..., :A][dead].any() and not got["d_pi_out"][..., A:][dead].any()
    assert not got["action"][dead].any() and got["d_pi_out"][..., :A][~dead].any()


def test_null_outputs_and_null_gradients_do_not_change_the_others():
    case = pc.CASES["odd"]
    x = pc.make_inputs(case)
    rig = Rig(case, x, 2.5)
    full = rig.run()
    for want in (("d_q_logits",), ("d_scaled_entropy",)):
        other = Rig(case, x, 2.5)
        other.forward(step_means=False)
        other.backward(want=want, d_se=False)
        got = other.read()
        assert _bits(got[want[0]]) == _bits(full[want[0]])
        skipped = "d_scaled_entropy" if want[0] == "d_q_logits" else "d_q_logits"
        assert (got[skipped] == SENTINEL).all() and (got["step_means"] == SENTINEL).all()
        assert _bits(got["losses"]) == _bits(full["losses"])
    # head_backward with one incoming gradient: the two add up to the full one (to rounding), and each is finite
    a_only, s_only = Rig(case, x, 2.5), Rig(case, x, 2.5)
    for r, kw in ((a_only, dict(d_se=False)), (s_only, dict(d_action=False))):
        r.forward()
        r.backward(**kw)
    ga, gs = a_only.read()["d_pi_out"], s_only.read()["d_pi_out"]
    assert np.abs(ga + gs - full["d_pi_out"]).max() <= 1e-5 * np.abs(full["d_pi_out"]).max() and ga.any() and gs.any()


def test_row_independence():
    case = pc.CASES["odd"]
    x = pc.make_inputs(case)
    base = Rig(case, x, 2.5).run()
    y = {k: (None if v is None else v.copy()) for k, v in x.items()}
    t, b = 4, 17
    y["pi_out"][t, b] += 0.25
    y["eps"][t, b] -= 0.5
    y["q_logits"][1, t, b] += np.linspace(0, 1, case["NB"], dtype=np.float32)
    got = Rig(case, y, 2.5).run()
    for k in ("action", "entropy", "scaled_entropy", "q", "d_pi_out"):
        keep = np.ones(base[k].shape[:2], bool)
        keep[t, b] = False
        assert _bits(got[k][keep]) == _bits(base[k][keep]) and _bits(got[k][t, b]) != _bits(base[k][t, b]), k
    keep = np.ones((2, case["T"], case["B"]), bool)
    keep[1, t, b] = False
    assert _bits(got["d_q_logits"][keep]) == _bits(base["d_q_logits"][keep])
    assert _bits(got["d_q_logits"][1, t, b]) != _bits(base["d_q_logits"][1, t, b])


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    case = pc.CASES["small"]
    x = pc.make_inputs(case)
    rig = Rig(case, x, 2.5)
    first = rig.run()
    second = rig.run()
    for b in rig.buf.values():
        b[GUARD:-GUARD] = SENTINEL
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rig.forward()
        rig.backward()
    for b in rig.buf.values():
        b[GUARD:-GUARD] = SENTINEL
    graph.replay()
    replay = rig.read()
    for k in OUTPUTS:
        assert _bits(first[k]) == _bits(second[k]) == _bits(replay[k]), k


# ---------------------------------------------------------------- 4. non-finite inputs
def test_one_nan_logit_row_and_one_nan_eps():
    case = pc.CASES["small"]
    x = pc.make_inputs(case)
    base = Rig(case, x, 2.5).run()
    y = {k: (None if v is None else v.copy()) for k, v in x.items()}
    y["q_logits"][0, 1, 4, 7] = np.nan
    y["eps"][2, 3, 1] = np.nan
    got = Rig(case, y, 2.5).run()
    # the logit row: its q, its seeds, the step mean and the loss that sum it
    assert np.isnan(got["q"][1, 4]) and np.isnan(got["d_q_logits"][0, 1, 4]).all() and np.isnan(got["step_means"][1])
    assert np.isnan(got["losses"][0])
    keep = np.ones((2, case["T"], case["B"]), bool)
    keep[0, 1, 4] = False
    assert _bits(got["d_q_logits"][keep]) == _bits(base["d_q_logits"][keep])
    keep = np.ones((case["T"], case["B"]), bool)
    keep[1, 4] = False
    assert _bits(got["q"][keep]) == _bits(base["q"][keep]) and _bits(got["step_means"][0]) == _bits(base["step_means"][0])
    # the eps row: its action, its entropies, its d_pi_out, the two means (and step 2's mean through scaled_entropy)
    for k in ("action", "entropy", "scaled_entropy", "d_pi_out"):
        keep = np.ones((case["T"], case["B"]), bool)
        keep[2, 3] = False
        assert np.isnan(got[k][2, 3]).any() and _bits(got[k][keep]) == _bits(base[k][keep]), k
    assert np.isnan(got["entropy"][2, 3]) and np.isnan(got["scaled_entropy"][2, 3]) and np.isnan(got["d_pi_out"][2, 3]).all()
    assert np.isnan(got["losses"][1]) and np.isnan(got["losses"][2]) and np.isnan(got["step_means"][2])
    assert _bits(got["d_scaled_entropy"]) == _bits(base["d_scaled_entropy"])
    # a NaN scale poisons everything that divides by it, and nothing else
    rig = Rig(case, x, float("nan"))
    got = rig.run()
    assert np.isnan(got["losses"][0]) and np.isnan(got["step_means"]).all() and np.isnan(got["d_q_logits"]).all()
    for k in ("action", "entropy", "scaled_entropy", "q", "d_scaled_entropy"):
        assert _bits(got[k]) == _bits(base[k]), k
    assert _bits(got["losses"][1:]) == _bits(base["losses"][1:])


# ---------------------------------------------------------------- agents
def _agent(name, **over):
    from oracle import cases
    from tdmpc2_amd.tdmpc2 import TDMPC2

    c = cases.build_case(name)
    cfg = c["cfg"].replace(batch_size=12, buffer_size=200, dropout=0.0, **over)
    agent = TDMPC2(cfg, device=DEV)
    agent.load({k: torch.as_tensor(v) for k, v in c["sd"].items()})
    agent.native_autograd = True
    return agent, cfg


def _hyper_of(agent, cfg):
    lmin, ldif = agent._log_std()
    return dict(vmin=pc.widen(cfg.vmin), vmax=pc.widen(cfg.vmax), rho=pc.widen(cfg.rho), entropy_coef=pc.widen(cfg.entropy_coef),
                log_std_min=lmin, log_std_dif=ldif)


def _pi_batch(cfg, B, seed=31):
    rng = np.random.default_rng(seed)
    T = cfg.horizon + 1
    zs = rng.random((T, B, cfg.latent_dim)).astype(np.float32)
    eps = rng.standard_normal((T, B, cfg.action_dim)).astype(np.float32)
    task = (np.arange(B) % len(cfg.tasks)).astype(np.int64) if cfg.multitask else None
    return zs, eps, task


# ---------------------------------------------------------------- 5. the tail against policy_loss
def test_tail_cross_check_with_policy_loss():
    """q, entropy and scaled_entropy of TDMPC2.policy_loss through tdmpc2_pigrad_loss_forward at the same scale: its pi_loss and both
    means, and policy_loss's own, against an fp64 numpy reduction of those rows; yardstick: the same reduction in torch's fp32."""
    from tdmpc2_amd import native

    agent, cfg = _agent("tiny")
    zs, eps, _ = _pi_batch(cfg, 12)
    T, B = zs.shape[:2]
    res = agent.policy_loss(torch.tensor(zs, device=DEV), pi_eps=torch.tensor(eps, device=DEV), qidx=torch.tensor([2, 0], dtype=torch.int32, device=DEV),
                            update_scale=False, want=("q", "entropy", "scaled_entropy"))
    h = _hyper_of(agent, cfg)
    rows = {k: res[k].reshape(T, B).contiguous() for k in ("q", "entropy", "scaled_entropy")}
    d = native.pigrad_desc(T, B, cfg.action_dim, cfg.num_bins, False, **h)
    losses = torch.empty(3, device=DEV)
    native.pigrad_loss_forward(d, rows["q"], rows["entropy"], rows["scaled_entropy"], agent.scale.value, losses)
    scale = float(agent.scale.value)
    r64 = {k: v.cpu().numpy().astype(np.float64) for k, v in rows.items()}
    w = h["rho"] ** np.arange(T)
    ref = np.asarray([(-(h["entropy_coef"] * r64["scaled_entropy"] + r64["q"] / scale).mean(1) * w).mean(), r64["entropy"].mean(),
                      r64["scaled_entropy"].mean()])
    t = {k: v.cpu() for k, v in rows.items()}
    yard = np.asarray([float((-(h["entropy_coef"] * t["scaled_entropy"] + t["q"] / scale).mean(1) * torch.tensor(w, dtype=torch.float32)).mean()),
                       float(t["entropy"].mean()), float(t["scaled_entropy"].mean())])
    own = np.asarray([float(res["pi_loss"]), float(res["pi_entropy"]), float(res["pi_scaled_entropy"])])
    got = losses.cpu().numpy()
    for i, name in enumerate(("pi_loss", "pi_entropy", "pi_scaled_entropy")):
        et = max(abs(yard[i] - ref[i]) / abs(ref[i]), pc.FLOOR)
        e, e_own = abs(got[i] - ref[i]) / abs(ref[i]), abs(own[i] - ref[i]) / abs(ref[i])
        print(f"{name}: pigrad {e / et:.3f}, policy_loss {e_own / et:.3f} (x max(e_torch32, 2^-23))")
        assert e <= pc.MARGIN * et and e_own <= pc.MARGIN * et, (name, e, e_own, et)


# ---------------------------------------------------------------- 6. Q_pair
@pytest.mark.parametrize("qidx", [(2, 0), (0, 4)])
def test_q_pair_equals_the_two_rows_of_q_all(qidx):
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.world_model import WorldModel

    cfg = named_config("tiny", num_q=5)
    torch.manual_seed(3)
    m = WorldModel(cfg).to(DEV)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.add_(torch.randn_like(p) * 0.1)
    m.native_autograd = True
    zs, eps, _ = _pi_batch(cfg, 12)
    z = torch.tensor(zs, device=DEV)
    a = torch.tanh(torch.tensor(eps, device=DEV)).requires_grad_(True)
    with torch.no_grad():
        full = m.Q(z, a, None, return_type="all")
    pair = m.Q_pair(z, a, None, qidx)
    assert pair.shape == (2, *zs.shape[:2], cfg.num_bins)
    assert torch.equal(pair.detach(), full[list(qidx)])
    pair.sum().backward()
    assert a.grad is not None and a.grad.abs().sum() > 0 and all(p.grad is None for p in m._Qs.parameters())


# ---------------------------------------------------------------- the torch-only path of update_pi
def _scale_update(value, x, tau):
    """RunningScale.update in torch (reference common/scale.py): percentiles 5 / 95 of x, clamp(min=1), lerp."""
    x = x.reshape(-1, 1)
    pct = torch.tensor([5.0, 95.0], dtype=x.dtype)
    pos = pct * (x.shape[0] - 1) / 100
    fl = torch.floor(pos)
    ce = torch.clamp(fl + 1, max=x.shape[0] - 1)
    wc = (pos - fl).unsqueeze(-1)
    wf = 1.0 - wc
    xs = torch.sort(x, dim=0).values
    p = xs[fl.long()] * wf + xs[ce.long()] * wc
    new = torch.clamp(p[1] - p[0], min=1.0)
    return value + tau * (new - value)


def _cpu_model(cfg, sd, dtype):
    from tdmpc2_amd.world_model import WorldModel

    m = WorldModel(cfg)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m.to(dtype=dtype)


def _torch_pi_loss(m, cfg, h, zs, eps, task, qidx, value, dtype, update_scale=True):
    from tdmpc2_amd.world_model import two_hot_inv

    T, B = zs.shape[:2]
    z = torch.tensor(zs, dtype=dtype)
    tk = None if task is None else torch.tensor(task)
    action, info = m.pi(z, tk, eps=torch.tensor(eps, dtype=dtype))
    tk_rows = None if tk is None else tk.repeat(T)  # (the module path of the Q ensemble takes rows: [T * B, .])
    ql = m.Q_pair(z.reshape(T * B, -1), action.reshape(T * B, -1), tk_rows, qidx).reshape(2, T, B, -1)
    q = two_hot_inv(ql, cfg).sum(0) / 2
    if update_scale:
        value = _scale_update(value, q[0].detach(), pc.widen(cfg.tau))
    qs = q / value
    rho = torch.tensor([h["rho"] ** i for i in range(T)], dtype=dtype)
    loss = (-(h["entropy_coef"] * info["scaled_entropy"] + qs).mean(dim=(1, 2)) * rho).mean()
    return loss, info, value


# ---------------------------------------------------------------- 7. parameter gradients
@pytest.mark.parametrize("name", ["tiny", "tiny_mt"])
def test_parameter_gradients_of_pi_loss(name):
    from oracle import cases
    from tdmpc2_amd import autograd, native

    agent, cfg = _agent(name)
    sd = cases.build_case(name)["sd"]
    h = _hyper_of(agent, cfg)
    zs, eps, task = _pi_batch(cfg, 9)
    qidx = (2, 0)
    grads = {}
    for tag, dtype in (("ref", torch.float64), ("yard", torch.float32)):
        m = _cpu_model(cfg, sd, dtype)
        loss, _, _ = _torch_pi_loss(m, cfg, h, zs, eps, task, qidx, torch.ones(1, dtype=dtype), dtype, update_scale=False)
        loss.backward()
        grads[tag] = {n: p.grad.numpy().copy() for n, p in m.named_parameters() if p.grad is not None and n.startswith("_pi.")}
        assert all(p.grad is None for n, p in m.named_parameters() if n.startswith("_Qs."))
    m = agent.model
    calls0 = native.PI_GRAD_CALLS
    z = torch.tensor(zs, device=DEV)
    tk = None if task is None else torch.tensor(task, device=DEV)
    action, info = m.pi(z, tk, eps=torch.tensor(eps, device=DEV))
    ql = m.Q_pair(z, action, tk, qidx)
    loss, parts = autograd.pi_loss(cfg, ql, info["entropy"], info["scaled_entropy"], agent.scale, update_scale=False)
    loss.backward()
    torch.cuda.synchronize()
    assert native.PI_GRAD_CALLS - calls0 == 5 and parts.shape == (2,) and not parts.requires_grad and loss.dim() == 0
    assert float(agent.scale.value) == 1.0
    worst = 0.0
    for n, p in m.named_parameters():
        if n.startswith("_Qs."):
            assert p.grad is None or not p.grad.any(), n
        if not n.startswith("_pi."):
            continue
        e, bound = pc.gate(p.grad.cpu().numpy(), grads["ref"][n], grads["yard"][n])
        worst = max(worst, e / (bound / pc.MARGIN))
        print(n, "e", e, "bound", bound)
        assert e <= bound, (n, e, bound)
    _merge_json(f"autograd_{name}", round(worst, 3))


# ---------------------------------------------------------------- 8. update_pi
PI_KEYS = ("pi_loss", "pi_grad_norm", "pi_entropy", "pi_scaled_entropy", "pi_scale")


@pytest.mark.parametrize("name", ["tiny", "tiny_mt"])
def test_update_pi_against_a_torch_only_path(name):
    """Three steps on one batch with pinned pi_eps / qidx.  Reference: the modules, torch math, the RunningScale formulas,
    clip_grad_norm_ and Adam with eps 1e-5 (widened fp32 hyperparameters) in fp64 on the CPU; yardstick: the same path in fp32."""
    from oracle import cases
    from tests import optim_common as oc

    agent, cfg = _agent(name)
    sd = cases.build_case(name)["sd"]
    h = _hyper_of(agent, cfg)
    zs, eps, task = _pi_batch(cfg, 12)
    qidx, steps = (1, 2), 3

    def torch_path(dtype):
        m = _cpu_model(cfg, sd, dtype)
        ps = list(m._pi.parameters())
        opt = torch.optim.Adam(ps, lr=oc.widen(cfg.lr), betas=(oc.widen(0.9), oc.widen(0.999)), eps=oc.widen(1e-5))
        value, out = torch.full((1,), 7.5, dtype=dtype), []  # (away from 1: every step divides by it and lerps it)
        for _ in range(steps):
            m.zero_grad()
            loss, info, value = _torch_pi_loss(m, cfg, h, zs, eps, task, qidx, value, dtype)
            loss.backward()
            norm = torch.nn.utils.clip_grad_norm_(ps, oc.widen(cfg.grad_clip_norm))
            opt.step()
            out.append([float(loss.detach()), float(norm), float(info["entropy"].mean()), float(info["scaled_entropy"].mean()), float(value)])
        return out

    ref, t32 = torch_path(torch.float64), torch_path(torch.float32)
    agent.planner()  # the handle exists: the step re-packs it
    agent.scale.value.fill_(7.5)
    z = torch.tensor(zs, device=DEV)
    tk = None if task is None else torch.tensor(task, device=DEV)
    got = []
    for _ in range(steps):
        info = agent.update_pi(z, tk, pi_eps=torch.tensor(eps, device=DEV), qidx=torch.tensor(qidx, device=DEV))
        assert set(info) == set(PI_KEYS) and all(v.dim() == 0 and v.is_cuda for v in info.values())
        got.append([float(info[k]) for k in PI_KEYS])
    worst, fails = dict.fromkeys(PI_KEYS, 0.0), []
    for s in range(steps):
        for i, k in enumerate(PI_KEYS):
            e, et = abs(got[s][i] - ref[s][i]) / abs(ref[s][i]), abs(t32[s][i] - ref[s][i]) / abs(ref[s][i])
            ratio = e / max(et, pc.FLOOR)
            worst[k] = max(worst[k], ratio)
            print("step", s, k, "lib", got[s][i], "ref64", ref[s][i], "e", e, "e_torch32", et, "ratio", round(ratio, 3))
            if ratio > pc.MARGIN:
                fails.append((s, k, e, et, ratio))
    _merge_json(f"update_pi_{name}", {k: round(v, 3) for k, v in worst.items()})
    assert not fails, fails


# ---------------------------------------------------------------- 9. update(buffer)
REF_KEYS = {"consistency_loss", "reward_loss", "value_loss", "termination_loss", "total_loss", "grad_norm", "pi_loss", "pi_grad_norm",
            "pi_entropy", "pi_scaled_entropy", "pi_scale"}


@pytest.mark.parametrize("name", ["tiny", "small_ep_fire"])
def test_update_from_a_buffer(name):
    from tdmpc2_amd import Buffer
    from tdmpc2_amd.native import NativeError

    agent, cfg = _agent(name)
    H, A, od = cfg.horizon, cfg.action_dim, cfg.obs_shape["state"][0]
    rng = np.random.default_rng(17)
    buf = Buffer(cfg, device=DEV, seed=5)
    for T in (21, 30, 17):
        td = {"obs": torch.as_tensor(rng.standard_normal((T, od)).astype(np.float32)),
              "action": torch.as_tensor(rng.uniform(-1, 1, (T, A)).astype(np.float32)),
              "reward": torch.as_tensor(rng.standard_normal(T).astype(np.float32))}
        if cfg.episodic:
            td["terminated"] = torch.as_tensor((rng.random(T) < 0.2).astype(np.float32))
        buf.add(td)
    planner = agent.planner()
    # update_pi alone: _pi is stepped, nothing else, and the planner's packed weights follow it
    rest = [p.detach().clone() for n, p in agent.model.named_parameters() if not n.startswith("_pi.")]
    packed0 = planner.export_packed()
    zs0, eps0, _ = _pi_batch(cfg, cfg.batch_size)
    agent.update_pi(torch.tensor(zs0, device=DEV), pi_eps=torch.tensor(eps0, device=DEV))
    packed = planner.export_packed()
    assert packed != packed0
    assert all(torch.equal(p, q) for p, q in zip((p for n, p in agent.model.named_parameters() if not n.startswith("_pi.")), rest))
    pi_before = [p.detach().clone() for p in agent.model._pi.parameters()]
    online = [p.detach().clone() for p in agent.model._Qs.parameters()]
    target = [p.detach().clone() for p in agent.model._target_Qs_params.buffers()]
    info = agent.update(buf)
    torch.cuda.synchronize()
    assert set(info) == REF_KEYS | ({"termination_rate", "termination_f1"} if cfg.episodic else set())
    assert all(v.dim() == 0 and v.is_cuda and bool(torch.isfinite(v)) for v in info.values())
    assert agent.last_zs.shape == (H + 1, cfg.batch_size, cfg.latent_dim) and not agent.last_zs.requires_grad
    assert (agent.last_term_logit is not None) == bool(cfg.episodic)
    assert not agent.model.training
    assert all(not torch.equal(p, q) for p, q in zip(agent.model._pi.parameters(), pi_before))
    assert planner.export_packed() != packed  # the planner's packed weights follow _pi (and the model)
    # the target Q moved by tau towards the online parameters after their step
    names = [n for n, _ in agent.model._target_Qs_params.named_buffers()]
    for n, t0, t1, q1 in zip(names, target, agent.model._target_Qs_params.buffers(), agent.model._Qs.parameters()):
        want = t0 + cfg.tau * (q1.detach() - t0)
        assert torch.allclose(t1, want, rtol=1e-5, atol=1e-7), n
    assert any(not torch.equal(a, b) for a, b in zip(online, agent.model._Qs.parameters()))
    agent.native_autograd = False
    with pytest.raises(NativeError, match="native_autograd"):
        agent.update_pi(agent.last_zs)
    with pytest.raises(NativeError, match="native_autograd"):
        agent.update(buf)
