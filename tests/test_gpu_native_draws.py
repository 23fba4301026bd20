"""GPU: `TDMPC2.native_draws` -- the draws of a training step made in the library (autograd.Draws) -- on the cases and the fixture
of tests/update_common.py (tests/golden/update_steps.npz) as they are, and the optimiser step without its host reads.

1. the flag against pins: `_update` with `native_draws` on and no pins is bit-equal to `_update` with the flag off and the four draws
   pinned to what the restatement names -- the normals as the unit's stateless call gives them at the restated key and counters
   (an fp64 restatement rounded to fp32 differs from the kernel's fp32 in the last bits, so the pins are the unit's own values, each
   checked here against the fp64 restatement under the gate of tests/draw_common.py), the pairs the restatement's own;
2. `update(buffer)` with dropout on: the counter discipline of one step (buffer, draws, dropout x2, Adam x2), eagerly;
3. `optimizer_step` reads nothing from the device; `sync_planner_weights()` called by a user still compares the constants.
Nothing here reads the reference tree."""
import numpy as np
import pytest
import torch

from tests import draw_common as dr
from tests import update_common as uc
from tests.test_gpu_update import _agent, _batch, _buffer, _fresh_packed

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def g():
    return uc.golden()


def _rows(infos, keys):
    return np.asarray([[float(info[k]) for k in keys] for info in infos])


# ---------------------------------------------------------------- 1. the flag against pins
@pytest.mark.parametrize("case_id", ["tiny-B33", "tiny_mt-B12"])
def test_native_draws_against_the_pinned_restatement(g, case_id):
    from tdmpc2_amd import native

    steps = 2
    batch = _batch(g, case_id)
    on, cfg = _agent(case_id, native_draws=True)
    off, _ = _agent(case_id)
    assert on.native_draws and not off.native_draws and off._draws is None
    H, B, A, nq = cfg.horizon, batch[1].shape[1], cfg.action_dim, cfg.num_q
    key = dr.key_of(cfg.seed)
    assert on.draws.key == key
    keys = uc.info_keys(cfg)
    for it in range(steps):
        calls0 = native.DRAW_CALLS
        a = on._update(*batch)
        td_a = on.last_td_targets.clone()
        assert native.DRAW_CALLS - calls0 == 2 and on.draws.state_dict()["counter"] == 2 * (it + 1)
        # the four draws at the counters the restatement names: 2 it (the TD target), 2 it + 1 (update_pi)
        pins = {}
        for name, qname, shape, call in (("td_pi_eps", "td_qidx", (H, B, A), 2 * it), ("pi_eps", "qidx", (H + 1, B, A), 2 * it + 1)):
            eps = torch.empty(shape, device=DEV)
            native.draw_noise(native.draw_desc(eps.numel(), 0, key, call), None, eps)
            ratio = dr.gate_ratio(eps.cpu().numpy().reshape(-1), dr.normals64(eps.numel(), key, call))
            print(case_id, "step", it, name, "gate ratio against the fp64 restatement", ratio)
            assert ratio <= 1.0, (name, ratio)
            pins[name] = eps
            pins[qname] = torch.tensor(dr.pair_of(nq, key, call), dtype=torch.int32, device=DEV)
        pins["qidx"] = pins["qidx"].long()
        calls0 = native.DRAW_CALLS
        b = off._update(*batch, pins=pins)
        assert native.DRAW_CALLS == calls0 and off._draws is None  # with the flag off it never moves
        assert set(a) == set(b) == set(keys)
        for k in keys:
            assert torch.equal(a[k], b[k]) and bool(torch.isfinite(a[k])), (it, k, float(a[k]), float(b[k]))
        assert torch.equal(td_a, off.last_td_targets), it
    # a pin overrides the drawn value and the draws are made all the same
    calls0 = native.DRAW_CALLS
    c = on._update(*batch, pins=pins)
    d = off._update(*batch, pins=pins)
    assert native.DRAW_CALLS - calls0 == 2 and all(torch.equal(c[k], d[k]) for k in keys)
    if cfg.multitask:
        return
    # update_model / update_pi alone make one draw each; the forward-only entry points make none
    calls0 = native.DRAW_CALLS
    on.update_model(*batch[:3])
    assert native.DRAW_CALLS - calls0 == 1
    on.update_pi(on.last_zs)
    assert native.DRAW_CALLS - calls0 == 2 and on.draws.state_dict()["counter"] == 2 * (steps + 1) + 2
    calls0 = native.DRAW_CALLS
    obs, action, reward = batch[:3]
    with torch.no_grad():
        on._td_target(on.model.encode(obs[1:], None), reward, torch.zeros_like(reward))
        on.policy_value(on.last_zs)
        on.act(obs[0, 0].cpu(), t0=True)
        on.model_losses(obs, action, reward)
        on.update_info(obs, action, reward)
    torch.cuda.synchronize()
    assert native.DRAW_CALLS == calls0 and not on.model.training


# ---------------------------------------------------------------- 2. the counters of one step, from a buffer
def test_update_from_a_buffer_counts_every_stream_once_per_step(g):
    from tdmpc2_amd import native
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.tdmpc2 import TDMPC2

    case_id, steps = "tiny-B33", 3
    cfg, sd = uc.build(case_id)
    cfg = cfg.replace(dropout=named_config("tiny").dropout, seed=7)
    assert cfg.dropout == 0.01
    agent = TDMPC2(cfg, device=DEV)
    agent.load({k: torch.as_tensor(v) for k, v in sd.items()})
    agent.native_autograd = agent.native_refresh = agent.native_draws = agent.native_dropout = True
    agent.planner()
    agent.scale.value.fill_(uc.SCALE0)
    buf = _buffer(cfg)
    keys = uc.info_keys(cfg)
    torch.manual_seed(3)
    rng0 = torch.cuda.get_rng_state(DEV)
    infos = []
    before = agent.planner().export_packed()
    for it in range(steps):
        draw0, drop0 = native.DRAW_CALLS, native.DROPOUT_CALLS
        info = agent.update(buf)
        torch.cuda.synchronize()
        assert native.DRAW_CALLS - draw0 == 2 and native.DROPOUT_CALLS - drop0 == 2 and set(info) == set(keys)
        infos.append(_rows([info], keys)[0])
        packed = agent.planner().export_packed()
        assert packed == _fresh_packed(agent) and packed != before, it
        before = packed
    assert np.isfinite(np.asarray(infos)).all()
    for i in range(steps):
        for j in range(i):
            assert (infos[i] != infos[j]).any(), (i, j)
    # one step: one sample, two draws, two masks, one Adam step of each optimiser
    assert agent.draws.state_dict() == {"seed": 7, "counter": 2 * steps}
    assert agent.model.q_masks.state_dict()["counter"] == 2 * steps
    assert agent.optim._native.get_step() == steps and agent.pi_optim._native.get_step() == steps
    assert buf.native.stats()["next_call"] == steps
    # the framework's generator was not drawn from
    assert torch.equal(torch.cuda.get_rng_state(DEV), rng0) and not agent.model.training


# ---------------------------------------------------------------- 3. the optimiser step reads nothing from the device
def test_optimizer_step_makes_no_host_read_of_the_constants(g):
    case_id = "tiny-H1-B1"
    agent, cfg = _agent(case_id, native_refresh=True, native_draws=True)
    batch = _batch(g, case_id)
    reads = []
    real = agent._log_std
    agent._log_std = lambda: (reads.append(1), real())[1]
    agent._update(*batch)  # two optimiser steps
    assert reads == []
    packed = agent.planner().export_packed()
    assert packed == _fresh_packed(agent)  # the re-pack still follows every step
    agent.sync_planner_weights()  # a user's call keeps its meaning: the comparison is made ...
    assert reads == [1] and agent._planner is not None and agent.planner().export_packed() == packed
    agent.model.log_std_min.fill_(-7.0)  # ... and a handle made with other constants is dropped
    agent.sync_planner_weights()
    assert reads == [1, 1] and agent._planner is None
