"""-m gpu: the per-tile rollout kernel (ks_rollout) keeps its bits when its source is rearranged without touching its arithmetic --
here: the action block of the step loop as a function of its own (fused_kernels.cuh: sample_actions), which changes the machine
code of every instantiation (register allocation) and no operation.  Four ways of holding it to that, all on the per-tile kernel
(set_cluster(0)) at a few plans:

1. the trace instantiation (TR = 1) and the planning one (TR = 0) are separate compilations of the same statements in one
   library: estimate_value without a trace equals the values of the traced call bit for bit (c1: A = 6, 16 action columns; c2:
   A = 38, 48 columns; E = 1 and 3; automatic and forced 64-row workgroups -- a trace always runs 64-row ones);
2. the same plan with 32- and with 64-row workgroups is bit-equal;
3. a Philox plan equals the plan replayed from its exported tape: the sampler's counters are functions of (step, row, column)
   -- refit folded and separate, and a multitask call with an action mask;
4. against the commit before: tests/golden/rollout_plan_digests.json (tests/rollout_bit_rows.py) was minted on that commit's
   library, two runs that agreed; 1 - 3 held on that library as well.
"""
import json

import numpy as np
import pytest
import torch

from tests import rollout_bit_rows as hr

pytestmark = pytest.mark.gpu

with open(hr.GOLDEN) as f:
    GOLDEN = json.load(f)


@pytest.mark.parametrize("rows", [0, 64])
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("name", ["c1", "c2"])
def test_values_equal_the_trace_kernels_bit_for_bit(name, E, rows):
    from tests.gpu_common import dev
    from tests.test_gpu_philox import _many_env_inputs

    c, model = hr.case_model(name)
    cfg = c["cfg"]
    planner = hr.make_planner(c, model, E, dict(rows=rows, cluster=0))
    inp = _many_env_inputs(c, model, E)
    tape = planner.export_noise(hr.SEED, hr.CALL, E)
    N, H, A = cfg.num_samples, cfg.horizon, cfg.action_dim
    actions = torch.as_tensor(np.random.default_rng(3).uniform(-1, 1, (E, H, N, A)).astype(np.float32)).to(dev())
    args = (inp["z0"], inp["disc_pow"], actions, tape["pi_eps"][:, 0].contiguous(), tape["qidx"][:, 0].contiguous())
    kw = dict(task_emb=inp["task_emb"], act_mask=inp["act_mask"])
    plain = planner.estimate_value(*args, trace=False, **kw)
    traced = planner.estimate_value(*args, trace=True, **kw)[0]
    torch.cuda.synchronize()
    planner.close()
    assert torch.isfinite(plain).all() and plain.abs().max() > 0
    assert torch.equal(plain, traced), (name, E, rows, (plain - traced).abs().max().item())


@pytest.mark.parametrize("name,E", [("c1", 3), ("c2", 2)])
def test_32_and_64_row_workgroups_give_the_same_plan(name, E):
    a = hr.run_plan(name, None, E, dict(rows=32, cluster=0))
    b = hr.run_plan(name, None, E, dict(rows=64, cluster=0))
    for k, x, y in zip(("action", "prev_mean") + hr.STAGES, a, b):
        assert torch.equal(x, y), (name, k)


@pytest.mark.parametrize("name,E,fold", [("c1", 2, 0), ("c1", 2, 1), ("c2", 1, 0), ("c2", 1, 1), ("mt5", 2, 0)])
def test_philox_plan_equals_its_exported_tape(name, E, fold):
    from tests.test_gpu_philox import _many_env_inputs, _plan

    c, model = hr.case_model(name)
    planner = hr.make_planner(c, model, E, dict(fold=fold, cluster=0))
    inp = _many_env_inputs(c, model, E)
    if name == "mt5":
        assert inp["act_mask"] is not None and (inp["act_mask"] == 0).any()  # the mask really masks
    seed = 0x0BAD_5EED_0000_0000 + 17 * E + fold
    _plan(planner, inp, None, seed=1)  # an earlier plan: the call counter is not 0 any more
    call = planner.call_counter()
    a0, p0, _ = _plan(planner, inp, None, seed)
    tape = planner.export_noise(seed, call, E)
    a1, p1, _ = _plan(planner, inp, tape, seed=1)  # (the seed is ignored with a tape)
    planner.close()
    assert torch.isfinite(a0).all()
    assert torch.equal(a0, a1), (name, E, fold, (a0 - a1).abs().max().item())
    assert torch.equal(p0, p1), (name, E, fold)


def test_the_golden_file_has_every_row():
    assert set(GOLDEN["rows"]) == set(hr.ROWS)


@pytest.mark.parametrize("rid", sorted(hr.ROWS))
def test_the_plan_returns_the_bits_of_the_commit_before(rid):
    assert hr.run_row(rid) == GOLDEN["rows"][rid], (rid, "minted from", GOLDEN["commit"])
