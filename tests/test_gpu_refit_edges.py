"""-m gpu: refit_plan (common.cuh) against the fp64 reference of tests/refit_common.py (cases, gates and where they come from:
there; tests/test_refit_edges.py proves them on the CPU).  (a) k_refit alone on crafted values and actions over the grid of sort
widths, elite counts and action shapes; (b) the final pick through the sharded entry points with a chosen tape, then every route a
plan can take -- separate launch, in-launch with 32- and 64-row workgroups, the counting path at 1024 samples, both cluster
paths, the layered family, padded sample counts -- recomputed per iteration from the plan's own returned values and actions, and
the same routes on weights whose values tie in every row.  No case is excluded anywhere.
TDMPC2_REFIT_EDGES_JSON=<file>: the worst err / gate per item and the measured expf error are merged into that file
(profiles/refit_edges.json)."""
import numpy as np
import pytest
import torch

from tests import refit_common as rc
from tests.test_refit_edges import record

pytestmark = pytest.mark.gpu

_worst, _facts = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _dump_worst():
    yield
    record("mi355x_worst_err_over_gate", _worst)
    if _facts:
        record("mi355x", _facts)


def _dev():
    return torch.device("cuda", 0)


def _note(item, ch):
    w = rc.worst(ch)
    _worst[item] = max(_worst.get(item, 0.0), w)
    return w


def _planner(base, E, iterations=1, **over):
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.native import NativePlanner

    cfg = named_config(base, **over)
    assert (cfg.temperature, cfg.min_std, cfg.max_std) == tuple(rc.CFG[k] for k in ("temperature", "min_std", "max_std"))
    return cfg, NativePlanner(cfg, iterations, _dev(), max_envs=E)


# ------------------------------------------------------------------ the device's expf
def test_expf_error_is_what_the_score_gate_assumes():
    """expf against fp64 on [-104, 0] (results that are normal numbers; below them the gate's floor applies): torch's device exp
    on a grid of 2^20 points, and the kernel's own expf read back exactly -- elite 0 at value 0 and 63 elites at 2 x, x <= -22:
    their exponentials sum below half an ulp of 1, so score_k = expf(x_k) bit for bit."""
    x = (-104.0 + 104.0 * np.arange(2 ** 20) / 2 ** 20).astype(np.float32)
    got = torch.exp(torch.as_tensor(x).to(_dev())).cpu().numpy().astype(np.float64)

    def ulps(x, got):
        want = np.exp(x.astype(np.float64))
        ok = want >= rc.FLT_MIN
        return float((np.abs(got - want)[ok] / np.spacing(want[ok].astype(np.float32)).astype(np.float64)).max())

    grid = ulps(x, got)
    E, N = 64, 64
    cfg, p = _planner("c1", E, num_samples=N, num_elites=N, horizon=1, action_dim=1)
    xs = np.sort(np.random.default_rng(0).uniform(-87.0, -22.0, (E, N - 1)).astype(np.float32), axis=1)[:, ::-1]
    value = np.concatenate([np.zeros((E, 1), np.float32), 2.0 * xs], axis=1)
    acts = torch.zeros(E, 1, N, 1, device=_dev())
    _, _, score, idx = p.refit(torch.as_tensor(value).to(_dev()), acts)
    torch.cuda.synchronize()
    score, idx = score.cpu().numpy(), idx.cpu().numpy()
    assert (score[:, 0] == 1.0).all()
    kern = ulps(np.take_along_axis(value, idx, 1)[:, 1:] * np.float32(0.5), score[:, 1:].astype(np.float64))
    print(f"expf worst ulp: device exp on the grid {grid:.3f}, the kernel's scores {kern:.3f}")
    _facts["expf_ulp"] = {"device_exp_on_2^20_points_of_[-104,0]": grid, "kernel_scores_4032_points_of_[-87,-22]": kern,
                          "gate_uses": rc.EXPF_ULP}
    assert max(grid, kern) <= rc.EXPF_ULP, (grid, kern)
    p.close()


# ------------------------------------------------------------------ (a) k_refit alone
def _unstaged(N, K, H, A):
    """Where k_refit cannot stage its elites in 48 KiB: the 5 x 61 actions from 61 elites on, and 1024 elites of 3 x 6."""
    return (H * A == 305 and K >= 61) or (H * A == 18 and K == 1024)


def _refit_call(p, cfg, vals, acts, mask=None):
    value = torch.as_tensor(vals).to(_dev()).contiguous()
    mk = None if mask is None else torch.as_tensor(mask).to(_dev()).contiguous()
    mean, std, score, idx = p.refit(value, torch.as_tensor(acts).to(_dev()).contiguous(), mk)
    torch.cuda.synchronize()
    return [dict(value=value[e].cpu().numpy(), mean=mean[e].cpu().numpy(), std=std[e].cpu().numpy(), score=score[e].cpu().numpy(),
                 elite_idx=idx[e].cpu().numpy()) for e in range(len(vals))]


@pytest.mark.parametrize("H,A", rc.GEOMETRY_HA, ids=[f"H{h}A{a}" for h, a in rc.GEOMETRY_HA])
@pytest.mark.parametrize("N", rc.GEOMETRY_N)
def test_k_refit_on_crafted_values_and_actions(N, H, A):
    for K in sorted(set(rc.K_OF(N))):
        if K > N:
            continue
        br = rc.branches(N, K, H, A)
        assert br["sorted"] and not br["in_launch"] and br["staged"] == (not _unstaged(N, K, H, A)), (N, K, H, A, br)
        assert rc.refit_threads(N) == {64: 64, 192: 256, 512: 512, 1024: 1024}[N]
        names, vals, acts = rc.plans_of(N, K, H, A)
        cfg, p = _planner("c1", len(names), num_samples=N, num_elites=K, horizon=H, action_dim=A, num_pi_trajs=min(24, N - 1))
        got = _refit_call(p, cfg, vals, acts)
        p.close()
        for e, name in enumerate(names):
            ch = rc.check(rc.refit_ref(vals[e], acts[e], K, **rc.CFG), got[e])
            w = _note(f"k_refit N{N} K{K} H{H} A{A} {'staged' if br['staged'] else 'unstaged'}", ch)
            assert w <= 1.0, (N, K, H, A, name, ch)


@pytest.mark.parametrize("K", [3, 61, 64])
def test_k_refit_multitask_mask_with_odd_action_width(K):
    N, H, A = 512, 3, 17
    names, vals, acts = rc.plans_of(N, K, H, A)
    E = len(names)
    rng = np.random.default_rng(K)
    mask = (rng.random((E, A)) < 0.7).astype(np.float32)
    mask[0], mask[1] = 1.0, 0.0
    cfg, p = _planner("mt5", E, num_samples=N, num_elites=K, horizon=H, action_dim=A)
    assert cfg.multitask and rc.branches(N, K, H, A) == dict(sorted=True, staged=True, in_launch=False)
    got = _refit_call(p, cfg, vals, acts, mask)
    p.close()
    for e, name in enumerate(names):
        ch = rc.check(rc.refit_ref(vals[e], acts[e], K, mask=mask[e], **rc.CFG), got[e])
        assert (got[e]["mean"][:, mask[e] == 0] == 0).all() and (got[e]["std"][:, mask[e] == 0] == 0).all()
        assert _note(f"k_refit mt5 N{N} K{K} A{A} masked", ch) <= 1.0, (K, name, ch)


# ------------------------------------------------------------------ (b) the final pick
def _bound(base, E, zero_heads=False, **over):
    from oracle import cases
    from oracle import planner_oracle as po
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.native import NativePlanner

    cfg = named_config(base, **over)
    c = cases.build_custom(cfg, E)
    if zero_heads:  # every row's reward and Q logits are 0: the same value bits in every row
        for k in ("_reward.2.weight", "_reward.2.bias", "_Qs.params.2.weight", "_Qs.params.2.bias"):
            c["sd"][k] = np.zeros_like(c["sd"][k])
    model = po.OracleModel(cfg, {k: torch.as_tensor(v) for k, v in c["sd"].items()})
    planner = NativePlanner(cfg, c["iterations"], _dev(), max_envs=E)
    planner.bind_state_dict(model.sd)
    return c, model, planner


@pytest.mark.parametrize("eval_mode", [False, True], ids=["noise", "eval"])
@pytest.mark.parametrize("K,H,A", [(64, 3, 6), (61, 3, 6), (1, 3, 6), (64, 1, 1)])
def test_final_pick_on_a_chosen_tape(K, H, A, eval_mode):
    """shard_begin, shard_values of the last iteration (which samples the actions), then shard_refit on CRAFTED values with a
    tape whose gumbel_exp / final_eps the test chooses.  Every case either keeps 100 gates between the fp64 top two
    (tests/test_refit_edges.py) or ties them by construction: the pick is checked in all of them."""
    from tests.gpu_common import plan_inputs

    N = 512
    pc = rc.pick_cases(K, H, N, A)
    names = list(pc)
    E = len(names)
    c, model, p = _bound("c1", E, iterations=1, num_elites=K, horizon=H, action_dim=A)
    assert c["iterations"] == 1
    assert rc.branches(N, K, H, A) == dict(sorted=True, staged=True, in_launch=False)
    inp = plan_inputs(c, model)
    tape = dict(inp["tape"])
    tape["gumbel_exp"] = torch.as_tensor(np.stack([pc[n]["gumbel_exp"] for n in names])).to(_dev()).contiguous()
    tape["final_eps"] = torch.as_tensor(np.stack([pc[n]["final_eps"] for n in names])).to(_dev()).contiguous()
    prev = inp["prev_mean"].clone()
    p.shard_begin(inp["z0"], prev, inp["t0"], tape=tape)
    value = torch.zeros(E, N, device=_dev())
    p.shard_values(0, 0, N, inp["z0"], inp["disc_pow"], value)
    value.copy_(torch.as_tensor(np.stack([pc[n]["value"] for n in names])))
    action = torch.full((E, A), 7.0, device=_dev())
    st = p.debug_buffers(E)
    p.shard_refit(0, value, prev, action, eval_mode=eval_mode, stages=st)
    torch.cuda.synchronize()
    st = {k: v.cpu().numpy() for k, v in st.items()}
    action, prev = action.cpu().numpy(), prev.cpu().numpy()
    p.close()
    fused = unfused = 0
    for e, name in enumerate(names):
        ref = rc.refit_ref(pc[name]["value"], st["actions"][e, 0], K, gumbel_exp=pc[name]["gumbel_exp"], final_eps=pc[name]["final_eps"],
                           eval_mode=eval_mode, last=True, **rc.CFG)
        assert ref["pick_tied"] or ref["pick_margin"] > ref["pick_gate"], name
        got = dict(value=st["value"][e, 0], elite_idx=st["elite_idx"][e, 0], score=st["score"][e, 0], mean=st["mean"][e, 0],
                   std=st["std"][e, 0], action=action[e], prev_mean=prev[e])
        ch = rc.check(ref, got)
        assert _note(f"final pick K{K} H{H} A{A} {'eval' if eval_mode else 'noise'}", ch) <= 1.0, (name, ch)
        assert np.abs(action[e]).max() <= 1.0
        if name == "all_tied" and K > 1:
            assert ref["pick"] == 0 and ref["elite_idx"][0] == 0
        if name == "eps_past_one" and not eval_mode:
            assert (np.abs(action[e]) == 1.0).all()
        fused += ch["action_is_fused"] and not ch["action_is_unfused"]
        unfused += ch["action_is_unfused"] and not ch["action_is_fused"]
    if not eval_mode:
        _facts[f"final_action K{K} H{H} A{A}: rows bit-equal to the fused expression only / to the unfused only / of"] = [int(fused), int(unfused), E]


# ------------------------------------------------------------------ (b) every route, from the plan's own stages
def _tune(p, cluster=None, fold=None, rows=None):
    if cluster is not None:
        p.set_cluster(cluster)
    if fold is not None:
        p.set_fold_refit(fold)
    if rows is not None:
        p.set_rows_per_workgroup(rows)


# name: (config, overrides, plans, tuning, in-launch?, the branch the refit must land in)
ROUTES = {
    "separate launch": ("c1", {}, 2, dict(cluster=0, fold=0), dict(sorted=True, staged=True, in_launch=False)),
    "in-launch, 32-row workgroups": ("c1", {}, 2, dict(cluster=0, fold=1, rows=32), dict(sorted=True, staged=True, in_launch=True)),
    "in-launch, 64-row workgroups": ("c1", {}, 2, dict(cluster=0, fold=1, rows=64), dict(sorted=True, staged=True, in_launch=True)),
    "in-launch, 1024 samples: counting": ("c1", dict(num_samples=1024), 2, dict(cluster=0, fold=1), dict(sorted=False, staged=True, in_launch=True)),
    "cluster": ("c1", {}, 2, dict(cluster=1, fold=1), dict(sorted=True, staged=True, in_launch=True)),
    "two clusters, one plan": ("c1", {}, 1, dict(cluster=2, fold=1), dict(sorted=True, staged=True, in_launch=True)),
    # 4 and 2 tiles of 32 rows: less than one group of 8 tiles per role
    "two clusters, one plan of 128 samples": ("c1", dict(num_samples=128, num_elites=16), 1, dict(cluster=2, fold=1), dict(sorted=True, staged=True, in_launch=True)),
    "two clusters, one plan of 64 samples": ("c1", dict(num_samples=64, num_elites=8, num_pi_trajs=8), 1, dict(cluster=2, fold=1),
                                             dict(sorted=True, staged=True, in_launch=True)),
    "cluster, 1024 samples: counting": ("c1", dict(num_samples=1024), 1, dict(cluster=1, fold=1), dict(sorted=False, staged=True, in_launch=True)),
    "layered": ("small", {}, 2, {}, dict(sorted=True, staged=True, in_launch=False)),
    "fused 500 -> 512": ("c1", dict(num_samples=500), 2, dict(cluster=0, fold=1), dict(sorted=True, staged=True, in_launch=True)),
    "fused 500 -> 512, cluster": ("c1", dict(num_samples=500), 1, dict(fold=1), dict(sorted=True, staged=True, in_launch=True)),
    "layered 200 -> 256": ("small", dict(num_samples=200), 2, {}, dict(sorted=True, staged=True, in_launch=False)),
    "layered 72 -> 128": ("small", dict(num_samples=72, num_elites=9, num_pi_trajs=5), 2, {}, dict(sorted=True, staged=True, in_launch=False)),
}


def _plan(c, model, p):
    from tests.test_gpu_planner import _run_native

    return _run_native(c, model, p)


def _check_plan(item, c, got):
    """refit_ref per plan and iteration on the values and actions the plan itself returned: the refit alone, whatever the rollout's
    error.  The last iteration adds the pick, the action and prev_mean."""
    cfg, I = c["cfg"], c["iterations"]
    for e in range(c["n_envs"]):
        for it in range(I):
            last = it == I - 1
            mask = None if not cfg.multitask else np.asarray(c["sd"]["_action_masks"][c["tasks"][e]])
            ref = rc.refit_ref(got["value"][e, it], got["actions"][e, it], cfg.num_elites, mask=mask, last=last,
                               gumbel_exp=c["tape"]["gumbel_exp"][e], final_eps=c["tape"]["final_eps"][e], **rc.CFG)
            g = {k: got[k][e, it] for k in ("value", "elite_idx", "score", "mean", "std")}
            if last:
                assert ref["pick_tied"] or ref["pick_margin"] > ref["pick_gate"], (item, e, "the pick would have to be excluded")
                g.update(action=got["action"][e], prev_mean=got["prev_mean"][e])
            ch = rc.check(ref, g)
            assert _note(item, ch) <= 1.0, (item, e, it, ch)


@pytest.mark.parametrize("name", list(ROUTES))
def test_refit_on_every_route_from_the_plans_own_stages(name):
    base, over, E, tune, want = ROUTES[name]
    c, model, p = _bound(base, E, iterations=2, **over)
    cfg = c["cfg"]
    fused = p.path == 1
    NP = p._npad
    assert rc.branches(NP, cfg.num_elites, cfg.horizon, cfg.action_dim, in_launch=fused and tune.get("fold") == 1) == want, name
    _tune(p, **tune)
    got = _plan(c, model, p)
    assert got["value"].shape[-1] == cfg.num_samples  # (padding rows are not returned: an elite index beyond them fails the check)
    assert np.isfinite(got["action"]).all() and p.take_fault() == 0, name  # (a bounded wait that gave up returns NaN and says so)
    _check_plan(f"route: {name}", c, got)
    if fused and tune.get("fold") == 1:
        # the same plan with the refit as a launch of its own: the same device function on the same data, bit for bit
        _tune(p, fold=0)
        sep = _plan(c, model, p)
        for k in got:
            assert np.array_equal(got[k], sep[k]), (name, k)
    if "cluster" in name:
        _tune(p, cluster=0)
        one = _plan(c, model, p)
        assert not np.array_equal(got["value"][:, 0], one["value"][:, 0]), "the cluster knob did not change the kernel"
    p.close()


# ------------------------------------------------------------------ (b) maximal ties on every route
TIES = dict(ROUTES)
TIES["fused 100 -> 128, every valid sample an elite"] = ("c1", dict(num_samples=100, num_elites=100), 2, dict(cluster=0, fold=1),
                                                         dict(sorted=True, staged=True, in_launch=True))
TIES["fused 100 -> 128, every valid sample an elite, cluster"] = ("c1", dict(num_samples=100, num_elites=100), 1, dict(fold=1),
                                                                  dict(sorted=True, staged=True, in_launch=True))
TIES["layered 72 -> 128, every valid sample an elite"] = ("small", dict(num_samples=72, num_elites=72, num_pi_trajs=5), 2, {},
                                                          dict(sorted=True, staged=True, in_launch=False))


@pytest.mark.parametrize("name", list(TIES))
def test_all_values_tied_elites_are_the_first_k_rows(name):
    """Reward and Q heads with zero last-layer weight and bias: every row evaluates to the same bits, so the contract's order
    makes the elites 0 ... K - 1 on every route, and never a padding row."""
    base, over, E, tune, want = TIES[name]
    c, model, p = _bound(base, E, zero_heads=True, iterations=2, **over)
    cfg = c["cfg"]
    assert rc.branches(p._npad, cfg.num_elites, cfg.horizon, cfg.action_dim, in_launch=p.path == 1 and tune.get("fold") == 1) == want, name
    _tune(p, **tune)
    got = _plan(c, model, p)
    p.close()
    v = got["value"].view(np.uint32)
    assert (v == v[..., :1]).all(), (name, "values are not the same bits in every row")
    K = cfg.num_elites
    assert (got["elite_idx"] == np.arange(K, dtype=np.int32)).all(), name
    assert (got["score"] == np.float32(1.0) / np.float32(K)).all()
    _check_plan(f"ties: {name}", c, got)
