"""GPU: the policy prior in HIP (tdmpc2_plan_bind_policy / pi / act_pi / act_pi_pix, policy_kernels.cuh) against the reference's own
outputs (tests/golden/policy.npz) on both routes, forced and auto; masks, eval mode, the in-kernel draws and the call counter;
act_pi_pix against pi(encode_pix); the agent's native_policy route against its PyTorch route; a captured hipGraph; the refusals;
and the planner left untouched by a policy call.

Gates (DESIGN 5's practice: a value is gated against fp32's own distance from fp64): every value of mean, action, log_std,
entropy and scaled_entropy within max(1e-5 x max(1, |v|), 2 x |reference fp32 - fp64|), the fp64 value being the reference's
formula evaluated on the fixture's inputs -- z for pi, the observation through the encoder for act_pi (tests/policy_common.py).
For mean and action (|v| <= 1) the floor is the encoder's Z_GATE of 1e-5.  It is relative beyond 1 because log_std reaches -10
and the entropies are sums of A such terms (a few thousand for scaled_entropy), where fp32's own spacing approaches 1e-5.  The
second term covers the ill-conditioned places: log(relu(1 - tanh^2) + 1e-6) amplifies round-off where tanh saturates (the c2
fixture has such a row), and the 317M chain (c4) puts the reference's own fp32 action 4e-6 from fp64."""
import numpy as np
import pytest
import torch

from tests import policy_common as pc

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = 1, 2, 4
ROUTES = {"auto": 0, "row": 1, "spread": 2}
_cache = {}
_G64_ACT = {}  # fp64 through the encoder as well: the bound of act_pi


def _dev():
    return torch.device("cuda", 0)


def _case(name):
    """(case, golden, planner with max_envs = the fixture's rows, planner weights + encoder + policy bound, tables)."""
    if name in _cache:
        return _cache[name]
    from oracle import cases
    from tdmpc2_amd.native import NativePlanner

    if name == "c4" or "c4" in _cache:  # 317M weights: one such handle at a time
        _cache.clear()
        torch.cuda.empty_cache()
    c = cases.build_case(name)
    g = pc.golden(name)
    n = len(g["z"])
    sd = {k: torch.as_tensor(v) for k, v in c["sd"].items()}
    p = NativePlanner(c["cfg"], c["iterations"], _dev(), max_envs=n)
    p.bind_state_dict(sd)
    p.bind_encoder({k: v for k, v in sd.items() if k.startswith("_encoder.state.")})
    p.bind_policy(sd)
    emb = mask = None
    if g["tasks"] is not None:
        e, m = pc.task_rows(c["sd"], g["tasks"])
        emb, mask = torch.as_tensor(e).to(_dev()), torch.as_tensor(m).to(_dev())
    g64 = pc.fp64_pi(c["cfg"], c["sd"], g["z"], g["tasks"], g["eps"])
    _G64_ACT[name] = pc.fp64_pi(c["cfg"], c["sd"], pc.fp64_encode(c["cfg"], c["sd"], g["obs"], g["tasks"]), g["tasks"], g["eps"])
    _cache[name] = (c, g, g64, p, emb, mask)
    return _cache[name]


def _check(action, info, g, g64, rows):
    gold = {k: (v[rows] if k != "tasks" and v is not None else v) for k, v in g.items()}
    g64r = {k: v[rows] for k, v in g64.items()}
    for key, got in (("action", action), ("mean", info["mean"]), ("log_std", info["log_std"])):
        err = np.abs(got.cpu().numpy().reshape(-1) - gold[key].reshape(-1))
        assert (err <= pc.entropy_bound(g64r, gold, key)).all(), (key, err.max())
    for key in ("entropy", "scaled_entropy"):
        err = np.abs(info[key].cpu().numpy().reshape(-1) - gold[key].reshape(-1))
        assert (err <= pc.entropy_bound(g64r, gold, key)).all(), (key, err, pc.entropy_bound(g64r, gold, key))


def _sl(t, rows):
    return None if t is None else t[rows].contiguous()


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", pc.CASES)
def test_pi_and_act_pi_match_reference_golden(name, route):
    c, g, g64, p, emb, mask = _case(name)
    p.set_policy_route(ROUTES[route])
    n = len(g["z"])
    try:
        for rows in (slice(0, 1), slice(0, n)):  # E = 1 and E = max_envs
            z = torch.as_tensor(g["z"][rows]).to(_dev()).contiguous()
            eps = torch.as_tensor(g["eps"][rows]).to(_dev()).contiguous()
            a, info = p.pi(z, task_emb=_sl(emb, rows), act_mask=_sl(mask, rows), eps=eps)
            _check(a, info, g, g64, rows)
            obs = torch.as_tensor(g["obs"][rows]).to(_dev()).contiguous()
            a2, info2 = p.act_pi(obs, task_emb=_sl(emb, rows), act_mask=_sl(mask, rows), eps=eps)
            _check(a2, info2, g, _G64_ACT[name], rows)
            if mask is not None:  # rows of different tasks: masked action dimensions are exactly 0
                m = mask[rows] == 0
                if rows.stop > 1:
                    assert len({int(r.sum()) for r in mask[rows]}) > 1
                for t in (a, info["mean"], info["log_std"], a2):
                    assert (t[m] == 0).all()
    finally:
        p.set_policy_route(0)


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_routes_agree_and_eval_mode_returns_the_mean(name):
    c, g, _, p, emb, mask = _case(name)
    obs = torch.as_tensor(g["obs"]).to(_dev()).contiguous()
    eps = torch.as_tensor(g["eps"]).to(_dev()).contiguous()
    outs = []
    for mode in (1, 2):
        p.set_policy_route(mode)
        outs.append(p.act_pi(obs, task_emb=emb, act_mask=mask, eps=eps))
        a, info = p.act_pi(obs, task_emb=emb, act_mask=mask, eps=eps, eval_mode=True)
        assert torch.equal(a, info["mean"]) and torch.equal(info["mean"], outs[-1][1]["mean"])
    p.set_policy_route(0)
    assert (outs[0][0] - outs[1][0]).abs().max().item() <= pc.GATE


def test_in_kernel_draws_replay_and_the_call_counter():
    c, g, _, p, emb, mask = _case("c2")
    from tdmpc2_amd.native import NativePlanner

    n, A = 256, c["cfg"].action_dim
    big = NativePlanner(c["cfg"], c["iterations"], _dev(), max_envs=n)
    big.bind_policy({k: torch.as_tensor(v) for k, v in c["sd"].items() if k.startswith("_pi.")})
    z = torch.as_tensor(np.tile(g["z"], (n // len(g["z"]), 1))).to(_dev()).contiguous()
    for mode in (1, 2):
        big.set_policy_route(mode)
        k0 = big.call_counter()
        a, info = big.pi(z, seed=7, return_eps=True)
        assert big.call_counter() == k0 + 1
        a2, info2 = big.pi(z, eps=info["eps"])  # replay with the draws that were used
        assert big.call_counter() == k0 + 2
        assert torch.equal(a, a2) and torch.equal(info["entropy"], info2["entropy"])
        assert torch.equal(info["scaled_entropy"], info2["scaled_entropy"])
        big.set_call_counter(k0)  # same seed and counter: the same draws
        a3, info3 = big.pi(z, seed=7, return_eps=True)
        assert torch.equal(a, a3) and torch.equal(info["eps"], info3["eps"])
        a4, _ = big.pi(z, seed=7)  # the next counter value: other draws
        assert not torch.equal(a, a4)
        e = info["eps"].double().cpu().numpy().reshape(-1)  # 256 x 38 draws ~ N(0, 1): mean and variance within 5 sigma
        N = e.size
        assert abs(e.mean()) <= 5 / np.sqrt(N) and abs(e.var() - 1) <= 5 * np.sqrt(2 / N), (e.mean(), e.var())
        assert len(np.unique(e)) > 0.99 * N  # rows and action indices get their own draws
    big.close()


def test_act_pi_pix_equals_pi_of_encode_pix():
    from tdmpc2_amd import layers, synth
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.native import NativePlanner

    cfg = named_config("c1")
    cfg.obs = "rgb"
    p = NativePlanner(cfg, cfg.iterations, _dev(), max_envs=8)
    sd = {k: torch.as_tensor(v) for k, v in synth.make_state_dict(cfg, 3).items()}
    p.bind_state_dict(sd)
    torch.manual_seed(3)
    m = layers.conv((9, 64, 64), 32, act=layers.SimNorm(8))
    p.bind_pixel_encoder({f"_encoder.rgb.{k}": v for k, v in m.state_dict().items()})
    p.bind_policy(sd)
    for E, mode in ((1, 0), (8, 1), (8, 2)):
        p.set_policy_route(mode)
        obs = torch.randint(0, 256, (E, 9, 64, 64), device=_dev(), dtype=torch.uint8)
        shift = torch.randint(0, 7, (E, 2), device=_dev(), dtype=torch.int32)
        eps = torch.randn(E, cfg.action_dim, device=_dev())
        a, info = p.act_pi_pix(obs, shift, eps=eps)
        b, info_b = p.pi(p.encode_pix(obs, shift), eps=eps)
        assert torch.equal(a, b) and torch.equal(info["entropy"], info_b["entropy"]) and torch.equal(info["log_std"], info_b["log_std"])
        ae, _ = p.act_pi_pix(obs, shift, eps=eps, eval_mode=True)
        assert torch.equal(ae, info["mean"])


def _agents(obs_kind):
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.tdmpc2 import TDMPC2

    out = []
    for native in (True, False):
        cfg = named_config("c1", mpc=False)
        if obs_kind == "rgb":
            cfg.obs, cfg.obs_shape = "rgb", {"rgb": (9, 64, 64)}
        torch.manual_seed(0)
        agent = TDMPC2(cfg, device=_dev(), max_envs=4)
        for prm in agent.model._pi[2].parameters():  # a policy with some spread (the default init is 0.02-small)
            torch.nn.init.normal_(prm, std=0.05)
        agent.native_policy = native
        agent.native_pixel_encoder = native
        agent.sync_planner_weights()
        out.append(agent)
    return out


@pytest.mark.parametrize("obs_kind", ["state", "rgb"])
def test_agent_native_policy_follows_the_torch_route(obs_kind):
    nat, ref = _agents(obs_kind)
    assert not ref.native_policy  # the default stays the PyTorch modules
    g = torch.Generator().manual_seed(5)
    for i in range(4):
        if obs_kind == "rgb":
            obs = torch.randint(0, 256, (9, 64, 64), generator=g, dtype=torch.uint8)
        else:
            obs = torch.randn(nat.cfg.obs_shape["state"][0], generator=g)
        for eval_mode in (False, True):
            torch.manual_seed(100 + i)
            a_nat = nat.act(obs, eval_mode=eval_mode)
            torch.manual_seed(100 + i)
            a_ref = ref.act(obs, eval_mode=eval_mode)
            assert a_nat.shape == a_ref.shape == (nat.cfg.action_dim,)
            assert (a_nat - a_ref).abs().max().item() <= pc.GATE, (i, eval_mode)
    # E environments at once = E single calls (same generator state)
    E = 4
    obs = (torch.randint(0, 256, (E, 9, 64, 64), generator=g, dtype=torch.uint8) if obs_kind == "rgb"
           else torch.randn(E, nat.cfg.obs_shape["state"][0], generator=g))
    torch.manual_seed(9)
    batch = nat.act_policy_batch(obs, eval_mode=True)
    if obs_kind == "state":  # (rgb: ShiftAug draws E shifts at once, so single calls see other shifts)
        single = torch.stack([nat.act(obs[e], eval_mode=True) for e in range(E)])
        assert torch.equal(batch, single)
    torch.manual_seed(9)
    assert (ref.act_policy_batch(obs, eval_mode=True) - batch).abs().max().item() <= pc.GATE


def test_agent_policy_matches_world_model_pi():
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.tdmpc2 import TDMPC2

    cfg = named_config("c1", mpc=False)
    torch.manual_seed(0)
    agent = TDMPC2(cfg, device=_dev())
    zs = torch.softmax(torch.randn(3, 5, cfg.latent_dim // 8, 8, device=_dev()), -1).reshape(3, 5, cfg.latent_dim)
    eps = torch.randn(3, 5, cfg.action_dim, device=_dev())
    a, info = agent.policy(zs, eps=eps)
    with torch.no_grad():
        torch.randn_like, saved = (lambda x, **kw: eps.clone()), torch.randn_like
        try:
            a_ref, info_ref = agent.model.pi(zs, None)
        finally:
            torch.randn_like = saved
    assert a.shape == (3, 5, cfg.action_dim) and info["scaled_entropy"].shape == (3, 5, 1)
    assert (a - a_ref).abs().max().item() <= pc.GATE
    for k in ("entropy", "scaled_entropy"):
        assert ((info[k] - info_ref[k]).abs() <= pc.GATE * info_ref[k].abs().clamp(min=1)).all(), k


@pytest.mark.parametrize("mode", [1, 2])
def test_pi_replays_from_a_hip_graph(mode):
    c, g, _, p, emb, mask = _case("m19_mt30")
    p.set_policy_route(mode)
    z = torch.as_tensor(g["z"]).to(_dev()).contiguous()
    obs = torch.as_tensor(g["obs"]).to(_dev()).contiguous()
    a_eager, i_eager = p.act_pi(obs, task_emb=emb, act_mask=mask, seed=3, return_eps=True)
    k = p.call_counter()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        p.pi(z, task_emb=emb, act_mask=mask, eps=i_eager["eps"])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        a_g, i_g = p.act_pi(obs, task_emb=emb, act_mask=mask, eps=i_eager["eps"])
    for _ in range(2):
        a_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a_g, a_eager) and torch.equal(i_g["scaled_entropy"], i_eager["scaled_entropy"])
    assert p.call_counter() == k + 2  # warm-up and capture; replays do not touch the host counter
    p.set_policy_route(0)


def test_refusals():
    from tdmpc2_amd import native
    from tdmpc2_amd.native import NativeError, NativePlanner, PolicyOut

    c, g, _, p, emb, mask = _case("m19_mt30")
    cfg = c["cfg"]
    fresh = NativePlanner(cfg, c["iterations"], _dev(), max_envs=2)
    lib, h, st = fresh.lib, fresh._h, fresh._stream()
    z = torch.as_tensor(g["z"][:2]).to(_dev()).contiguous()
    act = torch.empty(2, cfg.action_dim, device=_dev())
    out = PolicyOut(action=act.data_ptr())
    e, m = native._ptr(emb[:2].contiguous()), native._ptr(mask[:2].contiguous())
    assert lib.tdmpc2_plan_pi(h, 2, native._ptr(z), e, m, None, 0, out, st) == ERR_STATE  # nothing bound
    sd = {k: torch.as_tensor(v) for k, v in c["sd"].items()}
    fresh.bind_policy(sd)
    obs = torch.as_tensor(g["obs"][:2]).to(_dev()).contiguous()
    assert lib.tdmpc2_plan_act_pi(h, 2, native._ptr(obs), obs.shape[1], e, m, None, 0, 0, out, st) == ERR_STATE  # no encoder
    W = sd["_pi.1.weight"].to(_dev())
    b = sd["_pi.1.bias"].to(_dev())
    rc = lib.tdmpc2_plan_bind_policy(h, 1, native._ptr(W), native._ptr(b), native._ptr(b), native._ptr(b), W.shape[0], W.shape[1] + 1, st)
    assert rc == ERR_INVALID and b"expected" in lib.tdmpc2_last_error()
    W2 = sd["_pi.2.weight"].to(_dev())
    assert lib.tdmpc2_plan_bind_policy(h, 2, native._ptr(W2), native._ptr(b), None, None, W2.shape[0] - 2, W2.shape[1], st) == ERR_INVALID
    assert lib.tdmpc2_plan_pi(h, 2, native._ptr(z), e, m, None, 0, None, st) == ERR_INVALID  # null out
    assert lib.tdmpc2_plan_pi(h, 2, native._ptr(z), e, m, None, 0, PolicyOut(), st) == ERR_INVALID  # null out->action
    assert lib.tdmpc2_plan_pi(h, 2, native._ptr(z), None, None, None, 0, out, st) == ERR_INVALID  # multitask without tables
    fresh.bind_encoder({k: v for k, v in sd.items() if k.startswith("_encoder.state.")})
    for E in (0, 3):
        assert lib.tdmpc2_plan_act_pi(h, E, native._ptr(obs), obs.shape[1], e, m, None, 0, 0, out, st) == ERR_INVALID
    pix = torch.zeros(2, 9, 64, 64, dtype=torch.uint8, device=_dev())
    shift = torch.zeros(2, 2, dtype=torch.int32, device=_dev())
    assert lib.tdmpc2_plan_act_pi_pix(h, 2, native._ptr(pix), 0, 9, native._ptr(shift), None, 0, 0, out, st) == ERR_UNSUPPORTED
    assert fresh.lib.tdmpc2_plan_set_tuning(h, native.TUNE_POLICY_ROUTE, 3) == ERR_INVALID
    with pytest.raises(NativeError):
        fresh.act_pi(torch.zeros(3, obs.shape[1], device=_dev()), task_emb=emb, act_mask=mask)
    a, _ = fresh.pi(z, task_emb=emb[:2].contiguous(), act_mask=mask[:2].contiguous(), eps=torch.as_tensor(g["eps"][:2]).to(_dev()))
    assert np.abs(a.cpu().numpy() - g["action"][:2]).max() <= pc.GATE  # the refused calls left the handle usable
    fresh.close()


def test_planner_is_unchanged_by_the_policy_prior():
    from tests.gpu_common import case_on_gpu, plan_inputs

    c, model, planner = case_on_gpu("c1")
    inp = plan_inputs(c, model)

    def plan():
        pm = inp["prev_mean"].clone()
        a = planner.plan(inp["z0"], inp["disc_pow"], pm, inp["t0"], tape=inp["tape"])
        torch.cuda.synchronize()
        return a.clone(), pm

    a0, pm0 = plan()
    planner.bind_policy(model.sd)
    planner.pi(inp["z0"], seed=1)
    a1, pm1 = plan()
    assert torch.equal(a0, a1) and torch.equal(pm0, pm1)
