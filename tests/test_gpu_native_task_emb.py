"""GPU: the multitask training step with `native_task_emb` on (WorldModel._net_in -> autograd.task_concat, tdmpc2_task_*).

`tiny_mt-B12` of tests/update_common.py, its K iterations with the golden's pins: every info key under `info_bounds` (teacher-forced)
and `last_td_targets` under the TD gate (free-running) -- the gates tests/test_gpu_update.py applies with the flag off, taken from
the reference's own fp32 run against its fp64 run; the fixture's `no_emb_leak` control lies hundreds of bounds away, so a lost or
double-counted embedding gradient cannot pass.  Per `_update` the unit is called 2 H + 11 times (H + 6 forward calls --
encode(obs[1:]), encode(obs[0]), next x H, Q, reward, pi, Q_pair -- and H + 5 backward calls: all of those but encode(obs[1:]),
which runs without gradient).  With the flag off the unit is never called and two fresh agents step bit for bit alike.  After the K
steps the named rows' norms are at most 1 + the renorm bound, unnamed rows are bit-equal to their initial values and the
embedding's gradient holds what `update_pi` left.  A single-task agent steps bit for bit alike with the flag on and off and makes
no task call.  Nothing here reads the reference tree."""
import numpy as np
import pytest
import torch

from tests import task_common as tc
from tests import update_common as uc
from tests.test_gpu_update import _agent, _batch, _pins

pytestmark = pytest.mark.gpu
CASE = "tiny_mt-B12"


@pytest.fixture(scope="module")
def g():
    return uc.golden()


def _run(g, case_id, forced, steps=uc.K, **attrs):
    """`steps` iterations of `_update` -> (info rows, TD targets, agent, cfg, task calls per iteration)."""
    from tdmpc2_amd import native

    agent, cfg = _agent(case_id, **attrs)
    keys = uc.info_keys(cfg)
    batch = _batch(g, case_id)
    infos, tds, calls = np.zeros((steps, len(keys))), [], []
    for it in range(steps):
        before = native.TASK_CALLS
        info = agent._update(*batch, pins=_pins(g, case_id, it, forced=forced))
        calls.append(native.TASK_CALLS - before)
        infos[it] = [float(info[k]) for k in keys]
        tds.append(agent.last_td_targets.cpu().numpy().astype(np.float64))
    torch.cuda.synchronize()
    return infos, tds, agent, cfg, calls


def test_the_step_meets_the_reference_s_gates(g):
    infos, _, agent, cfg, calls = _run(g, CASE, forced=True, native_task_emb=True)
    keys = uc.info_keys(cfg)
    worst, fails = uc.info_ratios(infos, g, CASE, keys)
    print(CASE, "native_task_emb, worst e / max(e_ref32, 2^-23):", {k: round(v, 3) for k, v in worst.items()})
    margin, where = uc.control_margin(g, CASE, "no_emb_leak", keys)
    print("no_emb_leak lies", margin, "bounds away on", where)
    assert not fails, fails
    assert margin >= uc.SENSITIVITY
    assert calls == [2 * cfg.horizon + 11] * uc.K, calls
    assert not agent.model.training


def test_the_free_running_td_target_meets_its_gate(g):
    _, tds, _, cfg, calls = _run(g, CASE, forced=False, native_task_emb=True)
    gate, td64 = uc.td_gate(g, CASE), g[f"{CASE}.td64"]
    fails = []
    for it in range(uc.K):
        err = np.abs(tds[it] - td64[it])
        print(CASE, "native_task_emb, iteration", it, "worst |td - td64| / gate", float((err / gate[it]).max()))
        if not (err <= gate[it]).all():
            fails.append((it, float((err / gate[it]).max())))
    assert not fails, fails
    assert calls == [2 * cfg.horizon + 11] * uc.K, calls  # the TD target reads the task tables, not the unit


def test_the_table_and_its_gradient_after_the_steps(g):
    from tdmpc2_amd.tdmpc2 import TDMPC2

    cfg, sd = uc.build(CASE)
    init = np.asarray(sd["_task_emb.weight"], np.float32)
    _, _, agent, cfg, _ = _run(g, CASE, forced=True, native_task_emb=True)
    assert isinstance(TDMPC2.native_task_emb, property) and agent.model.native_task_emb
    w = agent.model._task_emb.weight.detach().cpu().numpy()
    named = np.zeros(len(cfg.tasks), bool)
    named[g[f"{CASE}.task"]] = True
    norms = np.sqrt((w.astype(np.float64) ** 2).sum(1))
    print("norms of the named rows", norms[named].min(), "..", norms[named].max(), "rows never named:", int((~named).sum()))
    assert (norms[named] <= 1.0 + tc.renorm_tol(cfg.task_dim)).all()
    assert w[~named].tobytes() == init[~named].tobytes()
    assert (w[named] != init[named]).any(axis=1).all()  # the model's optimiser moved every named row
    # what update_pi left on the embedding's gradient waits for the next model step
    grad = agent.model._task_emb.weight.grad.cpu().numpy()
    assert np.isfinite(grad).all() and grad[named].any(axis=1).all() and not grad[~named].any()
    assert not agent.pi_optim.grad.cpu().numpy().any()


def test_flag_off_is_the_old_path(g):
    from tdmpc2_amd import native

    before = native.TASK_CALLS
    runs = [_run(g, CASE, forced=False, steps=2) for _ in range(2)]
    assert native.TASK_CALLS == before and all(r[4] == [0, 0] for r in runs)
    (ia, ta, aa, _, _), (ib, tb, ab, _, _) = runs
    assert not aa.native_task_emb and not aa.model.native_task_emb
    assert ia.tobytes() == ib.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(ta, tb))
    assert torch.equal(aa.model._task_emb.weight, ab.model._task_emb.weight)


def test_a_single_task_agent_is_untouched(g):
    case_id = "tiny-B33"
    (ia, ta, aa, _, ca), (ib, tb, ab, _, cb) = (_run(g, case_id, forced=False, steps=1, native_task_emb=on) for on in (False, True))
    assert ca == cb == [0] and ab.native_task_emb and not aa.native_task_emb
    assert ia.tobytes() == ib.tobytes() and ta[0].tobytes() == tb[0].tobytes()
    for (ka, va), (kb, vb) in zip(aa.model.state_dict().items(), ab.model.state_dict().items()):
        assert ka == kb and (not torch.is_tensor(va) or torch.equal(va, vb)), ka
