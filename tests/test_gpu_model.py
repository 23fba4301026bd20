"""-m gpu: tdmpc2_plan_model_rollout / model_losses (the forward half of TDMPC2._update, reference tdmpc2/tdmpc2.py:259-304)
against the reference-minted fixtures tests/golden/model_<case>.npz (tools/make_model_golden.py).

Gate (every element of every stored field): max(1e-4 max(1, |v|), 2 x <field>_d64) -- 1e-4 relative to max(1, |v|) is the
project's gate for this layer code (TD_RTOL, tests/test_gpu_td_target.py), the second term is the reference's own fp32-vs-fp64
distance stored in the fixture.  The loss stage alone is gated at 1e-5 max(1, |v|) against the numpy restatement of
tests/model_common.py fed with the library's own logits / zs (fp32 reductions over at most 8 x 1024 rows)."""
import numpy as np
import pytest
import torch

from tests import model_common as mc
from tests.gpu_common import case_on_gpu, dev

pytestmark = pytest.mark.gpu

PRECS = [1, 2]  # exact-fp32 MFMA, f16x2 split
# (case, kernel family): the fused cases also run on the layered family
RUNS = [("tiny", 0), ("tiny_mt", 0), ("small_ep_fire", 2), ("c1_ep", 1), ("c1_ep", 2), ("c2", 1), ("c2", 2), ("mt5", 1), ("mt5", 2),
        ("c3", 2), ("c4", 2)]
LOSS_KEYS = ("consistency_loss", "reward_loss", "value_loss", "termination_loss", "total_loss")


_planners = {}


def _planner(name, path, prec, rows=8 * 130):
    """(case, oracle model, planner) like case_on_gpu, with max_envs large enough for `rows` rows of the layered family's
    workspace (max_envs x num_samples rows; the fused family takes any number of rows)."""
    key = (name, path, prec)
    if key not in _planners:
        from tdmpc2_amd.native import NativePlanner

        c, model, _ = case_on_gpu(name, path, prec)
        cfg = c["cfg"]
        if cfg.latent_dim > 1024:   # 317M-class: the fixture's batch is 8 rows
            return c, model, case_on_gpu(name, path, prec)[2]
        planner = NativePlanner(cfg, c["iterations"], dev(), max_envs=max(2, -(-rows // cfg.num_samples)), path=path, precision=prec)
        planner.bind_state_dict(model.sd)
        _planners[key] = (c, model, planner)
    return _planners[key]


def _tables(c, model):
    cfg = c["cfg"]
    if not cfg.multitask:
        return {}
    emb = model.sd["_task_emb.weight"]
    norm = emb.norm(2, dim=-1, keepdim=True)
    emb = torch.where(norm > 1.0, emb * (1.0 / (norm + 1e-7)), emb)  # nn.Embedding(max_norm=1)
    return dict(task_emb_table=emb.to(dev()).contiguous(), act_mask_table=model.sd["_action_masks"].to(torch.float32).to(dev()).contiguous())


def _call(c, model, planner, B, g, prefix, want, losses=True, rows=None, H=None):
    """One library call on the seeded inputs of (case, B); `rows`: a subset of the batch; H: fewer steps."""
    cfg = c["cfg"]
    inp = mc.inputs(cfg, B)
    rows = np.arange(B) if rows is None else np.asarray(rows)
    H = cfg.horizon if H is None else H
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev())
    kw = _tables(c, model)
    if cfg.multitask:
        kw["task_ids"] = d(inp["tasks"][rows].astype(np.int32))
    z0, act = d(inp["z0"][rows]), d(inp["actions"][:H, rows])
    if not losses:
        return planner.model_rollout(z0, act, want=want, **kw)
    td = g["td"]  # the reference's own _td_target output of the batch (stored in the fixture)
    return planner.model_losses(z0, act, d(inp["next_z"][:H, rows]), d(inp["reward"][:H, rows, 0]), d(td[:H, rows]),
                                d(inp["terminated"][:H, rows, 0]) if cfg.episodic else None, rho=cfg.rho,
                                coefs=(cfg.consistency_coef, cfg.reward_coef, cfg.value_coef, cfg.termination_coef), want=want,
                                step_means=True, **kw)


def _dev_args(c, model, B, H=None, seed=31):
    """Device tensors of one call, made BEFORE it (a captured call must not copy from the host): (z0, actions, targets, kw).
    H beyond cfg.horizon: actions and targets of their own (seeded), there is no fixture for those."""
    cfg = c["cfg"]
    H = cfg.horizon if H is None else H
    inp = mc.inputs(cfg, B)
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev())
    kw = _tables(c, model)
    if cfg.multitask:
        kw["task_ids"] = d(inp["tasks"].astype(np.int32))
    rng = np.random.default_rng(seed + H)
    from tdmpc2_amd import synth
    np_in = dict(actions=rng.uniform(-1, 1, (H, B, cfg.action_dim)).astype(np.float32),
                 next_z=synth.make_latents(cfg, H * B, seed=77).reshape(H, B, cfg.latent_dim),
                 reward=rng.standard_normal((H, B)).astype(np.float32), td=(rng.standard_normal((H, B)) * 4).astype(np.float32),
                 terminated=(rng.random((H, B)) < 0.2).astype(np.float32))
    tg = dict(next_z=d(np_in["next_z"]), reward=d(np_in["reward"]), td_target=d(np_in["td"]),
              terminated=d(np_in["terminated"]) if cfg.episodic else None)
    return d(inp["z0"]), d(np_in["actions"]), tg, kw, np_in


def _status(fn):
    """The status code a refused call returns (tdmpc2_status)."""
    from tdmpc2_amd.native import NativeError

    with pytest.raises(NativeError) as ex:
        fn()
    return int(str(ex.value).split("tdmpc2_plan error ")[1].split(":")[0])


INVALID, UNSUPPORTED, STATE = 1, 2, 4


def _check(got, g, prefix, fields, tag):
    bad = []
    for k in fields:
        if f"{prefix}.{k}" not in g:
            continue
        ref = g[f"{prefix}.{k}"]
        v = got[k].cpu().numpy().reshape(ref.shape)
        err = np.abs(v - ref)
        t = mc.tol(ref, g[f"{prefix}.{k}_d64"])
        print(f"[{tag}] {k}: max err {err.max():.3e} (max |v| {np.abs(ref).max():.3g}, d64 {float(g[f'{prefix}.{k}_d64']):.1e}, worst err/tol {np.max(err / t):.3f})")
        if not (err <= t).all():
            bad.append(k)
    assert not bad, f"{tag}: outside the gate: {bad}"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,path", RUNS)
def test_rollout_and_losses_match_reference_golden(name, path, prec):
    c, model, planner = _planner(name, path, prec)
    if path:
        assert planner.path == path
    cfg = c["cfg"]
    g = mc.golden(name)
    b_full, b_small = mc.CASES[name]
    want = ("zs", "reward_logits", "reward", "q_logits", "q") + (("term_logit",) if cfg.episodic else ())
    for B, fields in ((b_full, mc.FULL), (b_small, mc.SMALL)):
        if not B:
            continue
        gg = dict(g, td=g[f"b{B}.td"])
        got = _call(c, model, planner, B, gg, f"b{B}", want)
        _check(got, g, f"b{B}", fields, f"{name} path {planner.path} prec {prec} B {B}")
        # the loss stage alone: the library's own predictions through the numpy restatement, in fp64
        inp = mc.inputs(cfg, B)
        f = lambda k: got[k].cpu().numpy().astype(np.float64)
        tl = f("term_logit")[..., 0] if cfg.episodic else None
        ls, sm = mc.losses_from(cfg, f("zs"), f("reward_logits"), f("q_logits"), tl, inp["next_z"].astype(np.float64),
                                inp["reward"][..., 0].astype(np.float64), gg["td"].astype(np.float64),
                                inp["terminated"][..., 0].astype(np.float64))
        for k, ref in (("losses", ls), ("step_means", sm)):
            err = np.abs(got[k].cpu().numpy() - ref) / np.maximum(1.0, np.abs(ref))
            print(f"[{name} B {B}] loss stage alone, {k}: max rel err {err.max():.2e}")
            assert err.max() <= 1e-5, k
        # only-losses call: the same bits
        only = _call(c, model, planner, B, gg, f"b{B}", ())
        assert torch.equal(only["losses"], got["losses"]) and torch.equal(only["step_means"], got["step_means"])
        # and again: deterministic
        again = _call(c, model, planner, B, gg, f"b{B}", want)
        for k in again:
            assert torch.equal(again[k], got[k]), k
    assert planner.take_fault() == 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,path", [("c2", 1), ("c2", 2), ("mt5", 1), ("c3", 2)])
def test_q_agrees_with_policy_value_and_target_differs(name, path, prec):
    """q[qidx] reduced avg / min equals policy_value's q on the same (z, action) to fp32 round-off; the target ensemble differs."""
    c, model, planner = _planner(name, path, prec)
    cfg = c["cfg"]
    B = 130
    inp = mc.inputs(cfg, B)
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev())
    kw = _tables(c, model)
    if cfg.multitask:
        kw["task_ids"] = d(inp["tasks"].astype(np.int32))
    z = d(inp["z0"])
    qidx = d(inp["qidx"])
    for target in (False, True):
        a, qa = planner.policy_value(z, use_target=target, reduce="avg", pi_eps=d(inp["pi_eps"][0]), qidx=qidx, **kw)
        _, qm = planner.policy_value(z, use_target=target, reduce="min", pi_eps=d(inp["pi_eps"][0]), qidx=qidx, **kw)
        got = planner.model_rollout(z, a.reshape(1, B, -1).contiguous(), use_target=target, want=("q",), **kw)["q"][:, 0, :, 0]
        i0, i1 = int(inp["qidx"][0]), int(inp["qidx"][1])
        for ref, v in ((qa, (got[i0] + got[i1]) / 2), (qm, torch.minimum(got[i0], got[i1]))):
            err = ((v - ref).abs() / ref.abs().clamp(min=1)).max().item()
            print(f"[{name} path {path} prec {prec} target {target}] q vs policy_value: {err:.2e}")
            assert err <= 1e-5
        if target:
            online = planner.model_rollout(z, a.reshape(1, B, -1).contiguous(), want=("q",), **kw)["q"][:, 0, :, 0]
            assert (online - got).abs().max().item() > 1e-2
    assert planner.take_fault() == 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,path", [("c2", 1), ("c2", 2), ("c1_ep", 1), ("small_ep_fire", 2)])
def test_shapes_rows_and_steps(name, path, prec):
    """H = 0, 1, horizon; ragged B; a row's outputs do not depend on the other rows.  The fused family computes a row from its own
    tile row alone: bit-identical.  The layered family's GEMM routes (K-split tiles, TDMPC2_TUNE_KSPLIT) depend on the number of
    rows: equal to the 1e-5 the header states for that knob."""
    c, model, planner = _planner(name, path, prec)
    cfg = c["cfg"]
    want = ("zs", "reward", "q") + (("term_logit",) if cfg.episodic else ())
    full = _call(c, model, planner, 130, {}, "", want, losses=False)
    for rows in ([0], list(range(63)), list(range(65)), [129, 5, 64, 77]):
        sub = _call(c, model, planner, 130, {}, "", want, losses=False, rows=rows)
        for k in want:
            a, b = sub[k], full[k].index_select(-2, torch.as_tensor(rows, device=dev()))
            assert a.shape == b.shape and torch.isfinite(a).all()
            if planner.path == 1:
                assert torch.equal(a, b), (k, len(rows))
            else:
                assert ((a - b).abs() / b.abs().clamp(min=1)).max().item() <= 1e-5, (k, len(rows))
    for H in (0, 1):
        w = ("zs",) + (("term_logit",) if cfg.episodic else ()) + (("reward", "q") if H else ())
        sub = _call(c, model, planner, 130, {}, "", w, losses=False, H=H)
        for k in w:
            n = sub[k].shape[-3]
            ref = full[k][..., :n, :, :]
            assert sub[k].shape == ref.shape
            assert ((sub[k] - ref).abs() / ref.abs().clamp(min=1)).max().item() <= (0 if planner.path == 1 else 1e-5), (k, H)
    assert planner.take_fault() == 0


def test_refusals_return_their_status_and_leave_the_handle_usable():
    """Every refusal of the header's list, with the status it promises."""
    from tdmpc2_amd.native import NativePlanner

    c, model, planner = case_on_gpu("c2", 1, 2)
    cfg = c["cfg"]
    d = dev()
    z = torch.zeros(4, cfg.latent_dim, device=d)
    act = lambda h, a=cfg.action_dim: torch.zeros(h, 4, a, device=d)
    hb = lambda h: torch.zeros(h, 4, device=d)
    nz = lambda h, L=cfg.latent_dim: torch.zeros(h, 4, L, device=d)
    assert _status(lambda: planner.model_rollout(z, act(9))) == INVALID                                   # steps > 8
    assert _status(lambda: planner.model_rollout(z, act(1), want=("term_logit",))) == INVALID             # term_logit, not episodic
    assert _status(lambda: planner.model_losses(z, act(1), nz(1), hb(1), hb(1), terminated=hb(1))) == INVALID   # terminated, not episodic
    assert _status(lambda: planner.model_losses(z, act(0), nz(0), hb(0), hb(0))) == INVALID               # losses with steps = 0
    emb = torch.zeros(3, 8, device=d)
    with pytest.raises(ValueError):                                                                      # tasks on a single-task handle
        planner.model_rollout(z, act(1), task_ids=torch.zeros(4, dtype=torch.int32, device=d), task_emb_table=emb, act_mask_table=emb)
    # use_target without the target ensemble bound: a handle of its own, bound without the target heads
    bare = NativePlanner(cfg, c["iterations"], d, max_envs=2, path=1, precision=2)
    bare.bind_state_dict({k: v for k, v in model.sd.items() if not k.startswith("_target_Qs")})
    assert _status(lambda: bare.model_rollout(z, act(1), use_target=True)) == STATE
    assert torch.isfinite(bare.model_rollout(z, act(1), want=("q",))["q"]).all()                          # ... and stays usable
    # episodic handle without `terminated`
    ce, me, pe = case_on_gpu("c1_ep", 1, 2)
    ze = torch.zeros(4, ce["cfg"].latent_dim, device=d)
    assert _status(lambda: pe.model_losses(ze, act(1, ce["cfg"].action_dim), nz(1), hb(1), hb(1))) == INVALID
    # regression heads (num_bins 0 / 1): the rollout is served, the losses are refused
    for name, path in (("c1_nb0", 1), ("small_nb1_ep", 2)):
        cn, mn, pn = case_on_gpu(name, path, 2)
        cf = cn["cfg"]
        zn = torch.as_tensor(mc.inputs(cf, 4)["z0"]).to(d)
        out = pn.model_rollout(zn, act(1, cf.action_dim), want=("reward", "q", "reward_logits"))
        assert out["reward_logits"].shape == (1, 4, 1) and torch.isfinite(out["q"]).all()
        assert _status(lambda: pn.model_losses(zn, act(1, cf.action_dim), nz(1, cf.latent_dim), hb(1), hb(1),
                                               terminated=hb(1) if cf.episodic else None)) == UNSUPPORTED
        assert pn.take_fault() == 0
    # layered family: batch x steps beyond max_envs x num_samples rows
    c2, model2, lay = case_on_gpu("small_ep_fire", 2, 2)
    cfg2 = c2["cfg"]
    rows = 2 * cfg2.num_samples // 8 + 200
    assert _status(lambda: lay.model_rollout(torch.zeros(rows, cfg2.latent_dim, device=d),
                                             torch.zeros(8, rows, cfg2.action_dim, device=d))) == INVALID
    got = _call(c, model, planner, 12, {}, "", ("q",), losses=False)
    assert torch.isfinite(got["q"]).all()
    got = _call(c2, model2, lay, 12, {}, "", ("q", "term_logit"), losses=False)
    assert torch.isfinite(got["q"]).all() and torch.isfinite(got["term_logit"]).all()
    assert planner.take_fault() == 0 and lay.take_fault() == 0 and pe.take_fault() == 0 and bare.take_fault() == 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,path", [(n, p) for n, p in RUNS if n in mc.TARGET_CASES])
def test_target_ensemble_matches_reference_golden(name, path, prec):
    """use_target = 1 against the reference's Q(..., return_type='all', target=True) on the same rollout (fixture entry "tq")."""
    c, model, planner = _planner(name, path, prec)
    g = mc.golden(name)
    B = mc.CASES[name][0]
    z0, _, _, kw, _ = _dev_args(c, model, B)
    act = torch.as_tensor(mc.inputs(c["cfg"], B)["actions"]).to(dev())
    got = planner.model_rollout(z0, act, use_target=True, want=("q_logits", "q"), **kw)
    _check(got, g, "tq", ("q_logits", "q"), f"{name} path {planner.path} prec {prec} target")
    online = g[f"b{B}.q_logits"]
    assert np.abs(got["q_logits"].cpu().numpy() - online).max() > 1e-2   # not the online heads
    assert planner.take_fault() == 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,path", [("c2", 1), ("c2", 2), ("c1_ep", 1), ("small_ep_fire", 2), ("mt5", 1), ("c3", 2)])
def test_eight_steps(name, path, prec):
    """H = 8 (MAXH), B = 130: the rollout equals eight H = 1 calls chained through zs to 1e-5, the project's fp32 floor (the
    same kernels; not the same bits: the one call keeps the latent's hi / lo pieces in LDS, the chain re-splits their fp32 sum,
    and the layered GEMM routes depend on the row count), the predictions equal those of the H = 1 calls, and
    the losses equal the numpy restatement on the call's own predictions to 1e-5 (rho^7, the 8 / 9-step grids, 8 x 130 rows)."""
    c, model, planner = _planner(name, path, prec)
    cfg = c["cfg"]
    B, H = 130, 8
    z0, act, tg, kw, np_in = _dev_args(c, model, B, H)
    want = ("zs", "reward_logits", "reward", "q_logits", "q") + (("term_logit",) if cfg.episodic else ())
    got = planner.model_losses(z0, act, tg["next_z"], tg["reward"], tg["td_target"], tg["terminated"], rho=cfg.rho,
                               coefs=(cfg.consistency_coef, cfg.reward_coef, cfg.value_coef, cfg.termination_coef), want=want,
                               step_means=True, **kw)
    assert got["zs"].shape == (9, B, cfg.latent_dim) and got["q"].shape == (cfg.num_q, 8, B, 1)
    gate = 1e-5
    z = z0
    for t in range(H):
        one = planner.model_rollout(z, act[t:t + 1].contiguous(), want=("zs", "reward", "q"), **kw)
        for k, a, b in (("zs", got["zs"][t + 1], one["zs"][1]), ("reward", got["reward"][t], one["reward"][0]),
                        ("q", got["q"][:, t], one["q"][:, 0])):
            assert ((a - b).abs() / b.abs().clamp(min=1)).max().item() <= gate, (k, t)
        z = one["zs"][1].contiguous()
    f = lambda k: got[k].cpu().numpy().astype(np.float64)
    ls, sm = mc.losses_from(cfg, f("zs"), f("reward_logits"), f("q_logits"), f("term_logit")[..., 0] if cfg.episodic else None,
                            np_in["next_z"].astype(np.float64), np_in["reward"].astype(np.float64), np_in["td"].astype(np.float64),
                            np_in["terminated"].astype(np.float64))
    for k, ref in (("losses", ls), ("step_means", sm)):
        err = np.abs(got[k].cpu().numpy() - ref) / np.maximum(1.0, np.abs(ref))
        print(f"[{name} path {planner.path} prec {prec}] H = 8, {k}: max rel err {err.max():.2e}")
        assert err.max() <= 1e-5, k
    assert planner.take_fault() == 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["c2", "c1_ep", "c1"])
def test_rollout_agrees_with_estimate_value_trace(name, prec):
    """Fused handles, no golden: zs[t+1] equals the z_{t+1} tiles of estimate_value_trace and reward[t] its r_t scalars, for one
    environment whose N sample rows are the batch (its z0 repeated over the rows), to 1e-5 (Z_GATE: the project's fp32 floor;
    the planner's t = 0 step sums the z0 products separately, lay_cvec / cvec, so the bits differ)."""
    from tests.gpu_common import plan_inputs

    c, model, planner = case_on_gpu(name, 1, prec)
    cfg = c["cfg"]
    H, N, A = cfg.horizon, cfg.num_samples, cfg.action_dim
    inp = plan_inputs(c, model)
    actions = (torch.rand(1, H, N, A, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev())
    _, tiles, scal = planner.estimate_value(inp["z0"][:1].contiguous(), inp["disc_pow"][:1].contiguous(), actions,
                                            inp["tape"]["pi_eps"][:1, 0].contiguous(), inp["tape"]["qidx"][:1, 0].contiguous(), trace=True)
    got = planner.model_rollout(inp["z0"][:1].repeat(N, 1).contiguous(), actions[0].contiguous(), want=("zs", "reward"))
    for t in range(H):
        zt = tiles[:, 5 * t + 4].reshape(N, cfg.latent_dim)
        ez = (got["zs"][t + 1] - zt).abs().max().item()
        er = ((got["reward"][t, :, 0] - scal[0, :, t]).abs() / scal[0, :, t].abs().clamp(min=1)).max().item()
        print(f"[{name} prec {prec}] step {t}: zs vs trace {ez:.2e}, reward vs trace {er:.2e}")
        assert ez <= 1e-5 and er <= 1e-5, t
    assert planner.take_fault() == 0


@pytest.mark.parametrize("name,path", [("c2", 1), ("c1_ep", 1), ("mt5", 1), ("small_ep_fire", 2), ("c3", 2)])
def test_hipgraph_capture_replays_to_the_same_bits(name, path):
    """One model_rollout + one model_losses call captured in a hipGraph after a warm-up call of the shape (which sizes the
    workspace and the task tables): the calls allocate nothing and never synchronise the host, and the replay gives the eager bits."""
    c, model, planner = _planner(name, path, 2)
    cfg = c["cfg"]
    B = 130
    z0, act, tg, kw, _ = _dev_args(c, model, B)
    want = ("zs", "reward_logits", "reward", "q_logits", "q") + (("term_logit",) if cfg.episodic else ())
    coefs = (cfg.consistency_coef, cfg.reward_coef, cfg.value_coef, cfg.termination_coef)

    def both():
        r = planner.model_rollout(z0, act, want=want, **kw)
        l = planner.model_losses(z0, act, tg["next_z"], tg["reward"], tg["td_target"], tg["terminated"], rho=cfg.rho, coefs=coefs,
                                 step_means=True, **kw)
        return r, l

    er, el = both()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up on the side stream, then capture
        both()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        gr, gl = both()
    for i in range(2):
        for t in list(gr.values()) + list(gl.values()):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in er:
            assert torch.equal(gr[k], er[k]), (k, i)
        assert torch.equal(gl["losses"], el["losses"]) and torch.equal(gl["step_means"], el["step_means"]), i
    assert planner.take_fault() == 0


@pytest.mark.parametrize("name", mc.OBS_CASES)
def test_model_losses_from_observations(name):
    """TDMPC2.model_losses(obs, ...) end to end on state observations against the reference's losses of the same batch."""
    from tdmpc2_amd.tdmpc2 import TDMPC2

    c, _, _ = case_on_gpu(name, 0, 0)
    cfg = c["cfg"]
    g = mc.golden(name)
    B = mc.CASES[name][0]
    inp = mc.inputs(cfg, B)
    agent = TDMPC2(cfg.replace(), device=dev(), max_envs=2)
    agent.load({"model": {k: torch.as_tensor(v) for k, v in c["sd"].items()}})
    d = lambda a: torch.as_tensor(a).to(dev())
    res = agent.model_losses(d(mc.obs_inputs(cfg, B)), d(inp["actions"]), d(inp["reward"]), d(inp["terminated"]),
                             None if inp["tasks"] is None else d(inp["tasks"]), pi_eps=d(inp["pi_eps"]), qidx=d(inp["qidx"]))
    assert np.abs(res["zs"][0].cpu().numpy() - g["obs.z"][0]).max() <= 1e-5
    err = np.abs(res["td_targets"].cpu().numpy().reshape(-1) - g["obs.td"].reshape(-1)) / np.maximum(1, np.abs(g["obs.td"].reshape(-1)))
    assert err.max() <= mc.RTOL
    got = np.array([float(res[k]) for k in LOSS_KEYS])
    t = mc.tol(g["obs.losses"], g["obs.losses_d64"])
    print(f"[{name}] model_losses(obs): {got} vs {g['obs.losses']}")
    assert (np.abs(got - g["obs.losses"]) <= t).all()
