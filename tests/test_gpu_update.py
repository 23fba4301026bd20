"""GPU: `TDMPC2._update` against the reference's own `_update`, step by step (tests/golden/update_steps.npz: K iterations on one
batch per case, run verbatim on the CPU in fp64 and fp32; tests/update_common.py holds the cases and the gates, and
tests/test_update_golden.py shows that every deliberately wrong variant lies at least 10 bounds away).

1. teacher-forced: the fixture's fp64 TD target pinned, every info key of every iteration within MARGIN * max(e_ref32, FLOOR) of the
   fp64 run, e_ref32 the reference's own fp32 run; worst ratios go to the file TDMPC2_UPDATE_JSON names (profiles/update_edges.json);
2. free-running: the library's own TD target after every iteration under value_common.chain_gate, the planner's packed bytes
   against a fresh handle bound from the model, and `native_refresh` on and off bit for bit;
3. `pins=None` is the call without pins; 4. the remainder `update_pi` leaves on the task embedding's gradient.
Nothing here reads the reference tree."""
import json
import os

import numpy as np
import pytest
import torch

from tests import update_common as uc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CASE_IDS = list(uc.CASES)


def _merge_json(key, value):
    path = os.environ.get("TDMPC2_UPDATE_JSON")
    if not path:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.setdefault("gate", "e <= 4 * max(e_ref32, 2^-23) per info key, e = |x - ref64| / |ref64|, e_ref32 the largest error of the "
                           "reference's own fp32 run over the iterations; values are the worst e / max(e_ref32, 2^-23)")
    doc[key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def g():
    return uc.golden()


def _agent(case_id, **attrs):
    from tdmpc2_amd.tdmpc2 import TDMPC2

    cfg, sd = uc.build(case_id)
    agent = TDMPC2(cfg, device=DEV)
    agent.load({k: torch.as_tensor(v) for k, v in sd.items()})
    agent.native_autograd = True
    for k, v in attrs.items():
        setattr(agent, k, v)
    agent.planner()  # the handle exists: every step re-packs it
    agent.scale.value.fill_(uc.SCALE0)
    return agent, cfg


def _batch(g, case_id):
    b = uc.batch_of(g, case_id)
    return tuple(None if b[k] is None else torch.tensor(b[k], device=DEV) for k in ("obs", "action", "reward", "terminated", "task"))


def _pins(g, case_id, it, forced):
    t = lambda k, dtype=torch.float32: torch.tensor(g[f"{case_id}.{k}"][it], dtype=dtype, device=DEV)  # noqa: E731
    pins = {"pi_eps": t("pi_eps"), "qidx": t("qidx", torch.int64)}
    if forced:
        pins["td_targets"] = torch.tensor(g[f"{case_id}.td64"][it].astype(np.float32), device=DEV)
    else:
        pins.update(td_pi_eps=t("td_pi_eps"), td_qidx=t("td_qidx", torch.int32))
    return pins


# ---------------------------------------------------------------- 1. teacher-forced trajectory
@pytest.mark.parametrize("case_id", CASE_IDS)
def test_teacher_forced_trajectory(g, case_id):
    agent, cfg = _agent(case_id)
    keys = uc.info_keys(cfg)
    batch = _batch(g, case_id)
    got = np.zeros((uc.K, len(keys)))
    for it in range(uc.K):
        pins = _pins(g, case_id, it, forced=True)
        info = agent._update(*batch, pins=pins)
        assert set(info) == set(keys) and all(v.dim() == 0 and v.is_cuda for v in info.values())
        assert not agent.model.training and torch.equal(agent.last_td_targets, pins["td_targets"])
        got[it] = [float(info[k]) for k in keys]
    i64, i32 = g[f"{case_id}.info64"], g[f"{case_id}.info32"]
    for it in range(uc.K):
        for j, k in enumerate(keys):
            print(case_id, "iteration", it, k, "lib", got[it, j], "ref64", i64[it, j], "ref32", i32[it, j])
    worst, fails = uc.info_ratios(got, g, case_id, keys)
    print(case_id, "worst e / max(e_ref32, 2^-23):", {k: round(v, 3) for k, v in worst.items()})
    _merge_json(case_id, {k: round(v, 3) for k, v in worst.items()})
    assert not fails, fails


# ---------------------------------------------------------------- 2. free-running TD target and packed weights
_FREE = {}


def _fresh_packed(agent):
    from tdmpc2_amd.native import NativePlanner

    fresh = NativePlanner(agent.cfg, agent.cfg.iterations, DEV, max_envs=1, log_std_min=agent._planner_log_std[0],
                          log_std_dif=agent._planner_log_std[1])
    try:
        sd = {k: v for k, v in agent.model.state_dict().items() if torch.is_tensor(v)}
        fresh.bind_state_dict(sd)
        fresh.bind_encoder(sd)
        return fresh.export_packed()
    finally:
        fresh.close()


def _free_run(g, case_id, native_refresh):
    """K iterations with the four draws pinned and the TD target the library's own, run once per (case, setting):
    (last_td_targets per iteration, packed bytes == a fresh handle's per iteration, packed bytes changed per iteration)."""
    if (case_id, native_refresh) not in _FREE:
        agent, cfg = _agent(case_id, native_refresh=native_refresh)
        batch = _batch(g, case_id)
        tds, same, moved = [], [], []
        before = agent.planner().export_packed()
        for it in range(uc.K):
            agent._update(*batch, pins=_pins(g, case_id, it, forced=False))
            tds.append(agent.last_td_targets.cpu().numpy().astype(np.float64))
            packed = agent.planner().export_packed()
            same.append(packed == _fresh_packed(agent))
            moved.append(packed != before)
            before = packed
        _FREE[(case_id, native_refresh)] = (tds, same, moved)
    return _FREE[(case_id, native_refresh)]


@pytest.mark.parametrize("native_refresh", [False, True])
@pytest.mark.parametrize("case_id", CASE_IDS)
def test_free_running_td_target_and_packed_weights(g, case_id, native_refresh):
    tds, same, moved = _free_run(g, case_id, native_refresh)
    gate, td64 = uc.td_gate(g, case_id), g[f"{case_id}.td64"]
    fails = []
    for it in range(uc.K):
        err = np.abs(tds[it] - td64[it])
        print(case_id, "refresh", native_refresh, "iteration", it, "worst |td - td64| / gate", float((err / gate[it]).max()))
        if not (err <= gate[it]).all():
            fails.append((it, float((err / gate[it]).max())))
    assert not fails, fails
    assert all(same), same    # after the model step, the policy step and the soft update: what a fresh bind of the model packs
    assert all(moved), moved


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_refresh_settings_give_the_same_td_targets(g, case_id):
    off, on = _free_run(g, case_id, False)[0], _free_run(g, case_id, True)[0]
    for it in range(uc.K):
        assert off[it].tobytes() == on[it].tobytes(), it


# ---------------------------------------------------------------- 3. pins=None is the old call
def _buffer(cfg):
    from tdmpc2_amd import Buffer

    A, od = cfg.action_dim, cfg.obs_shape["state"][0]
    rng = np.random.default_rng(17)
    buf = Buffer(cfg, device=DEV, seed=5)
    for e, T in enumerate((21, 30, 17)):
        td = {"obs": torch.as_tensor(rng.standard_normal((T, od)).astype(np.float32)),
              "action": torch.as_tensor(rng.uniform(-1, 1, (T, A)).astype(np.float32)),
              "reward": torch.as_tensor(rng.standard_normal(T).astype(np.float32))}
        if cfg.episodic:
            td["terminated"] = torch.as_tensor((rng.random(T) < 0.2).astype(np.float32))
        if cfg.multitask:
            td["task"] = torch.full((T,), (7 * e + 3) % len(cfg.tasks), dtype=torch.int64)
        buf.add(td)
    return buf


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_pins_none_is_the_call_without_pins(g, case_id):
    batch = _batch(g, case_id)
    runs = []
    for kw in ({}, {"pins": None}):
        agent, cfg = _agent(case_id)
        torch.manual_seed(11)  # update_pi draws its noise and its heads on the framework's generator
        first = agent._update(*batch, **kw)
        assert not agent.model.training
        second = agent.update(_buffer(cfg))
        assert not agent.model.training
        torch.cuda.synchronize()
        runs.append((first, second, agent._seed))
    (a1, a2, seed_a), (b1, b2, seed_b) = runs
    assert seed_a == seed_b
    for a, b in ((a1, b1), (a2, b2)):
        assert set(a) == set(b) == set(uc.info_keys(cfg))
        for k in a:
            assert torch.equal(a[k], b[k]) and bool(torch.isfinite(a[k])), k
    with pytest.raises(ValueError, match="unknown pins"):
        agent._update(*batch, pins={"eps": None})


# ---------------------------------------------------------------- 4. the multitask remainder, directly
def test_update_pi_leaves_its_gradient_on_the_task_embedding(g):
    """What the reference is left with after `update_pi` (tdmpc2.py:227-230): pi_loss.backward() reaches `_task_emb.weight` through
    pi and Q(detach=True), pi_optim.zero_grad clears `_pi` alone, and the remainder enters the next model step.  The numerical
    check of the same thing is iteration 2's grad_norm in test 1."""
    case_id = "tiny_mt-B12"
    agent, cfg = _agent(case_id)
    agent._update(*_batch(g, case_id), pins=_pins(g, case_id, 0, forced=True))
    torch.cuda.synchronize()
    opt = agent.optim
    (i,) = [i for i, p in enumerate(opt.params) if p is agent.model._task_emb.weight]
    off, n = opt.offsets[i], opt.params[i].numel()
    arena = opt.grad.cpu().numpy()
    assert agent.model._task_emb.weight.grad.data_ptr() == opt.grad[off:off + n].data_ptr()
    assert arena[off:off + n].any() and np.isfinite(arena).all()
    rest = arena.copy()
    rest[off:off + n] = 0
    assert not rest.any()
    assert not agent.pi_optim.grad.cpu().numpy().any()
    # only the rows of the tasks in the batch carry it
    rows = arena[off:off + n].reshape(len(cfg.tasks), cfg.task_dim)
    in_batch = np.zeros(len(cfg.tasks), bool)
    in_batch[g[f"{case_id}.task"]] = True
    assert rows[in_batch].any(axis=1).all() and not rows[~in_batch].any()
