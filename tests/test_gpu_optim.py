"""GPU: tdmpc2_optim_step against the numpy emulation of tests/optim_common.py.
  norm      |norm - norm64| <= (D + 2) 2^-24 norm64 (all terms non-negative; D from optim_route.h), two runs bit-identical, and equal
            bit for bit to the published order restated in numpy; the error of torch's fp32 clip_grad_norm_ is recorded beside it
  exact     every case, both clip regimes, 3 steps with fresh gradients: m, v, p and the zeroed g equal the fp32 emulation (fed the
            library's own norm) bit for bit; get_step == 3; padding still zero; guard floats around misaligned views unchanged
  measured  |g| ~ 1e-25 (v underflows): finite, and within e <= 4 max(e_torch32, 2^-23) of the fp64 emulation
and special gradients, the flags, resume, hipGraph capture, ClipAdam / TDMPC2.optim / pi_optim / optimizer_step, and a 5-step
trajectory against a torch-only fp64 path.  TDMPC2_OPTIM_JSON=<file> merges the measured ratios into that file
(profiles/optim_edges.json)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import optim_common as oc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
B1, B2, EPS = (oc.widen(oc.HYPER[k]) for k in ("beta1", "beta2", "eps"))
GUARD = 5  # floats in front of and behind a misaligned view


def _merge_json(key, value):
    path = os.environ.get("TDMPC2_OPTIM_JSON")
    if not path:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.setdefault("gate", "e <= 4 * max(e_torch32, 2^-23); norm: |norm - norm64| <= (D + 2) 2^-24 norm64")
    doc[key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


class Rig:
    """One tdmpc2_optim_t over the parameters of a case, its three arenas, and the emulation's state beside it."""

    def __init__(self, case, max_norm, seed=0, params=None):
        from tdmpc2_amd import native

        self.case, self.counts, self.groups = case, case["counts"], case["groups"]
        self.lrs = [oc.widen(v) for v in case["lrs"]]
        self.max_norm = oc.widen(max_norm)
        self.p_emu = params if params is not None else oc.make_values(self.counts, [seed, 17], 1e-3, 10.0)
        self.bases, self.views = [], []
        for i, p in enumerate(self.p_emu):
            k = (1, 3)[i % 2] if case["misaligned"] else 0  # floats past a 16-byte boundary
            g = GUARD if case["misaligned"] else 0
            base = torch.full((4 + k + p.size + g,), 777.0 + i, dtype=torch.float32, device=DEV)
            assert base.data_ptr() % 16 == 0
            view = base[4 + k:4 + k + p.size]
            view.copy_(torch.from_numpy(p))
            assert view.data_ptr() % 16 == 4 * k
            self.bases.append(base)
            self.views.append(view)
        self.opt = native.NativeOptim([(v.data_ptr(), v.numel(), g) for v, g in zip(self.views, self.groups)], self.lrs, B1, B2, EPS,
                                      self.max_norm, DEV)
        assert (self.opt.offsets, self.opt.arena_floats) == oc.layout(self.counts)
        n = self.opt.arena_floats
        self.grad, self.m, self.v = (torch.zeros(n, dtype=torch.float32, device=DEV) for _ in range(3))
        self.norm = torch.full((1,), -1.0, dtype=torch.float32, device=DEV)
        self.st = oc.new_state(self.counts, np.float32)
        self.pad = oc.padding_mask(self.counts)

    def set_grads(self, grads):
        self.grad.copy_(torch.from_numpy(oc.to_arena(grads, self.counts)))

    def step(self, zero_grad=True, norm_out=True):
        self.opt.step(self.grad, self.m, self.v, zero_grad, self.norm if norm_out else None)
        torch.cuda.synchronize()
        return self.norm.cpu().numpy()[0]

    def emulate(self, grads, norm, zero_grad=True):
        g = [x.copy() for x in grads]
        oc.emulate_step(self.st, self.p_emu, g, self.groups, self.lrs, B1, B2, EPS, self.max_norm, np.float32, norm=norm, zero_grad=zero_grad)
        return g

    def params(self):
        return [v.cpu().numpy() for v in self.views]

    def check_exact(self, g_emu, what):
        m, v, g = (oc.from_arena(t.cpu().numpy(), self.counts) for t in (self.m, self.v, self.grad))
        for i, (p, pe) in enumerate(zip(self.params(), self.p_emu)):
            for name, a, b in (("p", p, pe), ("m", m[i], self.st["m"][i]), ("v", v[i], self.st["v"][i]), ("g", g[i], g_emu[i])):
                assert a.tobytes() == b.tobytes(), (what, name, i, self.counts[i], int((a != b).sum()))
        for t in (self.m, self.v, self.grad):  # the padding stays zero
            assert not t.cpu().numpy()[self.pad].any(), what
        for i, (base, view) in enumerate(zip(self.bases, self.views)):  # nothing outside a parameter is written
            k = (view.data_ptr() - base.data_ptr()) // 4
            b = base.cpu().numpy()
            assert (b[:k] == 777.0 + i).all() and (b[k + view.numel():] == 777.0 + i).all(), (what, i)


CASE_IDS = sorted(oc.CASES)


@pytest.mark.parametrize("name", CASE_IDS)
def test_norm_bound_order_and_repeatability(name):
    case = oc.CASES[name]
    rig = Rig(case, 1.0)
    grads = oc.make_values(case["counts"], [1, 2])
    arena = oc.to_arena(grads, case["counts"])
    rig.set_grads(grads)
    n1 = rig.step()
    rig.set_grads(grads)
    n2 = rig.step()
    n64 = float(np.sqrt(np.sum(arena.astype(np.float64) ** 2)))
    D = oc.norm_depth(arena.size)
    ts = [torch.from_numpy(g).to(DEV).requires_grad_() for g in grads]
    for t, g in zip(ts, grads):
        t.grad = torch.from_numpy(g).to(DEV)
    nt = float(torch.nn.utils.clip_grad_norm_(ts, 1e30))
    rec = dict(D=D, lib_err_ulps=abs(float(n1) - n64) / (oc.U * n64), torch32_err_ulps=abs(nt - n64) / (oc.U * n64))
    print(name, rec)
    _merge_json(f"norm/{name}", {k: round(v, 3) for k, v in rec.items()})
    assert n1.tobytes() == n2.tobytes()
    assert abs(float(n1) - n64) <= (D + 2) * oc.U * n64
    assert n1.tobytes() == np.float32(oc.norm_model(arena)[0]).tobytes()  # the published order, restated in numpy


@pytest.mark.parametrize("regime", sorted(oc.REGIMES))
@pytest.mark.parametrize("name", CASE_IDS)
def test_exact_gate(name, regime):
    case = oc.CASES[name]
    rig = Rig(case, oc.REGIMES[regime])
    for s in range(3):
        grads = oc.make_values(case["counts"], [3, s])
        rig.set_grads(grads)
        norm = rig.step()
        assert (norm > rig.max_norm) == (regime == "clip")
        rig.check_exact(rig.emulate(grads, norm), (name, regime, s))
    assert rig.opt.get_step() == 3


SMALL = dict(name="small", counts=[5, 64, 257, 1025], groups=[0, 2, 0, 2], lrs=oc.LRS, misaligned=False)


def test_tiny_gradients_outside_the_exact_gate():
    """|g| ~ 1e-25: g * g underflows, so v and the norm are 0 in fp32 (in torch's too): finite results, inside the measured gate."""
    counts = SMALL["counts"]
    rig = Rig(SMALL, 1.0)
    p0 = [p.copy() for p in rig.p_emu]
    gs = [oc.make_values(counts, [5, s], 1e-26, 1e-24) for s in range(2)]
    st = oc.new_state(counts, np.float64)
    ref_p = [p.astype(np.float64) for p in p0]
    for g in gs:
        rig.set_grads(g)
        rig.step()
        oc.emulate_step(st, ref_p, [x.astype(np.float64) for x in g], SMALL["groups"], rig.lrs, B1, B2, EPS, rig.max_norm, np.float64)
    t32 = oc.torch_steps(p0, gs, SMALL["groups"], rig.lrs, B1, B2, EPS, rig.max_norm, torch.float32)
    got = (rig.params(), oc.from_arena(rig.m.cpu().numpy(), counts), oc.from_arena(rig.v.cpu().numpy(), counts))
    worst = {}
    for name, a, t, r in zip(("p", "exp_avg", "exp_avg_sq"), got, t32[:3], (ref_p, st["m"], st["v"])):
        for x, y, z in zip(a, t, r):
            assert np.isfinite(x).all()
            e, et = oc.rel_err(x, z), oc.rel_err(y, z)
            worst[name] = max(worst.get(name, 0.0), e / max(et, oc.FLOOR))
            print(name, x.size, "e", e, "e_torch32", et)
            assert e <= oc.MARGIN * max(et, oc.FLOOR), (name, e, et)
    _merge_json("tiny_gradients", {k: round(v, 3) for k, v in worst.items()})


def test_zero_and_nan_gradients():
    rig = Rig(SMALL, 1.0)
    before = [p.tobytes() for p in rig.params()]
    assert rig.step() == 0.0  # the arena is all zeros
    assert [p.tobytes() for p in rig.params()] == before
    grads = oc.make_values(SMALL["counts"], [6, 0])
    grads[2][100] = np.nan
    rig.set_grads(grads)
    assert np.isnan(rig.step())  # as clip_grad_norm_(error_if_nonfinite=False) and Adam do: the coefficient is NaN, so is every parameter
    assert all(np.isnan(p).all() for p in rig.params())
    for t in (rig.m, rig.v, rig.grad):
        assert not t.cpu().numpy()[rig.pad].any()  # the padding is zero even then


def test_flags_and_resume():
    """zero_grad = 0 stores the CLIPPED gradient back (torch's clip scales in place); norm_out = NULL works; set_step(k) then a step
    has the scalars of k real steps."""
    rig = Rig(SMALL, 1.0)
    grads = oc.make_values(SMALL["counts"], [7, 0])
    rig.set_grads(grads)
    norm = rig.step(zero_grad=False)
    g_emu = rig.emulate(grads, norm, zero_grad=False)
    rig.check_exact(g_emu, "zero_grad=0")
    assert any(g.any() for g in g_emu) and all((np.abs(a) <= np.abs(b)).all() for a, b in zip(g_emu, grads))
    # norm_out = NULL: the step runs (the clipped gradients are its input now), the norm tensor is not written
    rig.norm.fill_(-1.0)
    n = np.float32(oc.norm_model(rig.grad.cpu().numpy())[0])
    assert rig.step(norm_out=False) == -1.0
    rig.check_exact(rig.emulate(g_emu, n), "norm_out=NULL")
    # resume
    k = 1000
    rig.opt.set_step(k)
    oc.set_step(rig.st, k, B1, B2)
    grads = oc.make_values(SMALL["counts"], [7, 1])
    rig.set_grads(grads)
    norm = rig.step()
    rig.check_exact(rig.emulate(grads, norm), "resume")
    assert rig.opt.get_step() == k + 1


def test_captured_step_advances_on_replay():
    case = oc.CASES["edges"]
    eager, cap = Rig(case, 1.0), Rig(case, 1.0)
    gs = [oc.make_values(case["counts"], [8, s]) for s in range(3)]
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):  # nothing allocates, nothing synchronises: the step captures as it is
        cap.opt.step(cap.grad, cap.m, cap.v, True, cap.norm)
    norms = []
    for g in gs:
        eager.set_grads(g)
        norms.append(eager.step().tobytes())
        cap.set_grads(g)
        graph.replay()
        torch.cuda.synchronize()
        assert cap.norm.cpu().numpy()[0].tobytes() == norms[-1]
    for a, b in zip(eager.params() + [t.cpu().numpy() for t in (eager.m, eager.v, eager.grad)],
                    cap.params() + [t.cpu().numpy() for t in (cap.m, cap.v, cap.grad)]):
        assert a.tobytes() == b.tobytes()
    assert cap.opt.get_step() == 3 == eager.opt.get_step()


# ---------------------------------------------------------------- ClipAdam, TDMPC2.optim / pi_optim / optimizer_step
def _tiny_agent(name="tiny"):
    from tdmpc2_amd import TDMPC2
    from tdmpc2_amd.config import named_config

    cfg = named_config(name, dropout=0.0)
    torch.manual_seed(9)
    agent = TDMPC2(cfg, device=DEV)
    with torch.no_grad():  # away from the init's zero biases and unit gains
        for n, p in agent.model.named_parameters():
            p.add_(torch.randn_like(p) * (0.1 if n.endswith("weight") and p.dim() >= 2 else 0.2))
    agent.native_autograd = True
    return cfg, agent


def _batch(cfg, dtype=torch.float32, device=DEV, B=33):
    rng = np.random.default_rng(13)
    obs, a = rng.standard_normal((B, cfg.obs_shape["state"][0])), np.tanh(rng.standard_normal((B, cfg.action_dim)))
    return torch.tensor(obs, dtype=dtype, device=device), torch.tensor(a, dtype=dtype, device=device)


def _model_loss(m, obs, a):
    z = m.encode(obs, None)
    zn = m.next(z, a, None)
    return zn.square().sum() + m.reward(z, a, None).sin().sum() + m.Q(zn, a, None, return_type="all").cos().sum()


def _before(opt):
    """(gradient arena, flat parameters) of a ClipAdam as numpy copies: what the next step reads."""
    return opt.grad.cpu().numpy(), [p.detach().cpu().numpy().reshape(-1).copy() for p in opt.params]


def _emulate_clipadam(opt, st, before, norm):
    """The emulation applied to `before` with the library's own norm -> the parameters it expects."""
    arena, ps = before
    counts = [p.numel() for p in opt.params]
    groups = [gi for gi, g in enumerate(opt.param_groups) for _ in g["params"]]
    lrs = [oc.widen(g["lr"]) for g in opt.param_groups]
    oc.emulate_step(st, ps, oc.from_arena(arena, counts), groups, lrs, oc.widen(opt.betas[0]), oc.widen(opt.betas[1]), oc.widen(opt.eps),
                    oc.widen(opt.max_norm), np.float32, norm=norm.cpu().numpy())
    return ps


def test_clipadam_plumbing_on_a_tiny_world_model():
    cfg, agent = _tiny_agent()
    m = agent.model
    obs, a = _batch(cfg)
    opt, pi_opt = agent.optim, agent.pi_optim
    # the reference's groups, every parameter exactly once, _pi in its own optimiser
    ids = lambda ps: [id(p) for p in ps]  # noqa: E731
    assert sorted(ids(opt.params) + ids(pi_opt.params)) == sorted(ids(m.parameters()))
    assert ids(pi_opt.params) == ids(m._pi.parameters()) and not set(ids(opt.params)) & set(ids(pi_opt.params))
    assert [ids(g["params"]) for g in opt.param_groups] == [ids(m._encoder.parameters()), ids(m._dynamics.parameters()),
                                                             ids(m._reward.parameters()), [], ids(m._Qs.parameters()), []]
    assert opt.param_groups[0]["lr"] == cfg.lr * cfg.enc_lr_scale and all(g["lr"] == cfg.lr for g in opt.param_groups[1:])
    assert (opt.max_norm, opt.eps, pi_opt.eps, pi_opt.max_norm) == (cfg.grad_clip_norm, 1e-8, 1e-5, cfg.grad_clip_norm)
    ptrs = [p.grad.data_ptr() for p in m.parameters()]
    st = oc.new_state([p.numel() for p in opt.params], np.float32)
    pi_before = [p.detach().clone() for p in m._pi.parameters()]
    for _ in range(2):
        _model_loss(m, obs, a).backward()
        assert opt.grad.abs().sum() > 0
        before = _before(opt)
        norm = opt.step()
        want = _emulate_clipadam(opt, st, before, norm)
        assert not opt.grad.any()  # zeroed in the same call
        for p, w in zip(opt.params, want):
            assert p.detach().cpu().numpy().reshape(-1).tobytes() == w.tobytes()
        assert [p.grad.data_ptr() for p in m.parameters()] == ptrs
        assert all(torch.equal(p, q) for p, q in zip(m._pi.parameters(), pi_before))  # untouched by TDMPC2.optim
    # _pi is stepped by pi_optim alone
    model_before = [p.detach().clone() for p in opt.params]
    act, info = m.pi(m.encode(obs, None).detach(), None)
    (act.sum() + 0.1 * info["entropy"].sum()).backward()
    norm = agent.optimizer_step("pi")
    assert float(norm) > 0 and pi_opt._native.get_step() == 1 and opt._native.get_step() == 2
    assert all(not torch.equal(p, q) for p, q in zip(m._pi.parameters(), pi_before))
    assert all(torch.equal(p, q) for p, q in zip(opt.params, model_before))
    with pytest.raises(ValueError):
        agent.optimizer_step("both")


def test_clipadam_on_plain_tensors_with_a_state_dict_round_trip():
    """Two tensors, a per-group lr and an empty group; gradients accumulate in place into the arena views; a new optimiser resumes
    from state_dict() bit for bit."""
    import tdmpc2_amd

    w = [torch.nn.Parameter(torch.from_numpy(v).to(DEV)) for v in oc.make_values([70, 513], [9, 0], 1e-3, 10.0)]
    make = lambda: tdmpc2_amd.ClipAdam([{"params": [w[0]], "lr": 1e-3}, {"params": []}, {"params": [w[1]]}], lr=3e-4, max_norm=0.5)  # noqa: E731
    opt = make()
    st = oc.new_state([70, 513], np.float32)
    for s in range(3):
        if s == 2:  # resume in a new optimiser: arenas and step
            sd = opt.state_dict()
            opt.close()
            opt = make()
            opt.load_state_dict(sd)
            assert sd["step"] == 2
        (w[0] * (s + 1.5)).sum().backward()
        (w[1].square() * 0.01).sum().backward()
        (w[1] * 0.25).sum().backward()  # accumulates in place into the arena view
        before = _before(opt)
        assert np.array_equal(oc.from_arena(before[0], [70, 513])[1], (w[1].detach() * 0.02 + 0.25).cpu().numpy())
        norm = opt.step()
        assert float(norm) > 0.5
        for p, x in zip(opt.params, _emulate_clipadam(opt, st, before, norm)):
            assert p.detach().cpu().numpy().tobytes() == x.tobytes()
        assert not opt.grad.any()
    w[0].grad = None
    with pytest.raises(tdmpc2_amd.native.NativeError):
        opt.step()


def test_optimizer_step_leaves_the_planner_packed_from_the_new_weights():
    from tdmpc2_amd.native import NativePlanner

    cfg, agent = _tiny_agent("small")
    obs, a = _batch(cfg)
    agent.planner()  # the handle exists
    before = agent.planner().export_packed()
    agent.optim  # noqa: B018  (the arenas exist before backward)
    _model_loss(agent.model, obs, a).backward()
    assert float(agent.optimizer_step("model")) > 0
    after = agent.planner().export_packed()
    A = NativePlanner(agent.cfg, agent.cfg.iterations, DEV, max_envs=1, log_std_min=agent._planner_log_std[0],
                      log_std_dif=agent._planner_log_std[1])
    sd = {k: v for k, v in agent.model.state_dict().items() if torch.is_tensor(v)}
    A.bind_state_dict(sd)
    A.bind_encoder(sd)
    assert after == A.export_packed() and after != before
    A.close()


def test_trajectory_against_a_torch_only_path():
    """5 steps on one batch.  Reference: the modules in fp64 on the CPU with clip_grad_norm_ + torch.optim.Adam (the widened fp32
    hyperparameters); yardstick: the same path in fp32.  Gated per step: the loss and the returned grad_norm.  Measured on an
    MI355X (profiles/optim_edges.json): worst ratio 0.81 for the loss, 0.55 for grad_norm."""
    from tdmpc2_amd.world_model import WorldModel

    cfg, agent = _tiny_agent()
    start = [p.detach().cpu().clone() for p in agent.model.parameters()]
    steps = 5

    def torch_path(dtype):
        m = WorldModel(cfg)
        with torch.no_grad():
            for p, q in zip(m.parameters(), start):
                p.copy_(q)
        m = m.to(dtype=dtype)
        m.eval()
        obs, a = _batch(cfg, dtype, "cpu")
        lr = oc.widen(cfg.lr)
        groups = [{"params": list(m._encoder.parameters()), "lr": oc.widen(cfg.lr * cfg.enc_lr_scale)}] + \
                 [{"params": list(x.parameters())} for x in (m._dynamics, m._reward, m._Qs)]
        ps = [p for g in groups for p in g["params"]]
        opt = torch.optim.Adam(groups, lr=lr, betas=(B1, B2), eps=EPS)
        out = []
        for _ in range(steps):
            loss = _model_loss(m, obs, a)
            loss.backward()
            norm = torch.nn.utils.clip_grad_norm_(ps, oc.widen(cfg.grad_clip_norm))
            opt.step()
            opt.zero_grad()
            out.append((float(loss.detach()), float(norm)))
        return out

    ref, t32 = torch_path(torch.float64), torch_path(torch.float32)
    obs, a = _batch(cfg)
    got = []
    agent.optim  # noqa: B018
    for _ in range(steps):
        loss = _model_loss(agent.model, obs, a)
        loss.backward()
        got.append((float(loss.detach()), float(agent.optimizer_step("model"))))
    worst = {"loss": 0.0, "grad_norm": 0.0}
    rows = []
    for s in range(steps):
        for k, name in enumerate(("loss", "grad_norm")):
            e, et = abs(got[s][k] - ref[s][k]) / abs(ref[s][k]), abs(t32[s][k] - ref[s][k]) / abs(ref[s][k])
            ratio = e / max(et, oc.FLOOR)
            worst[name] = max(worst[name], ratio)
            rows.append((s, name, got[s][k], ref[s][k], e, et, ratio))
            print("step", s, name, "lib", got[s][k], "ref64", ref[s][k], "e", e, "e_torch32", et, "ratio", round(ratio, 3))
    _merge_json("trajectory", {k: round(v, 3) for k, v in worst.items()})
    for s, name, _, _, e, et, ratio in rows:
        assert ratio <= oc.MARGIN, (s, name, e, et, ratio)
