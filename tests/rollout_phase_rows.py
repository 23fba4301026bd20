"""The rows of tests/golden/rollout_phase_digests.json: per-tile plans (set_cluster(0)) of the geometries at which the phases
between the rollout kernel's GEMMs take another path -- the bias source of the first-layer epilogues (the plain vector, the
per-plan cvec rows at t = 0, the multitask beff rows), the action block at every action padding in PHILOX mode (the digests of
tests/rollout_bit_rows.py and tests/fused_plan_rows.py are tape-driven), the policy-prior rows present and absent, the episodic
kernel, the exact-fp32 arithmetic, and a one-step rollout (the only step that is both first and last) -- and the SHA-256 of what
each returns.  tools/make_rollout_phase_digests.py mints the file from the library of the commit BEFORE a change of those
phases; tests/test_gpu_rollout_phases.py holds the library under test to it bit for bit.  Public Python API only."""
import os

import numpy as np
import torch

from tests.fused_plan_rows import CALL, SEED, STAGES, digest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_phase_digests.json")
PHILOX_SEED = 0x0DDB_17E5_0000_0001

# id: (case, config overrides, E, tuning, noise: "tape" | "philox", exact fp32)
ROWS = {
    "mt5-E5-rows32-tape": ("mt5", {}, 5, dict(rows=32), "tape", False),     # beff bias rows, an action mask
    "mt5-E5-rows64-tape": ("mt5", {}, 5, dict(rows=64), "tape", False),
    "c1-E2-philox": ("c1", {}, 2, dict(), "philox", False),                 # A = 6: 16 action columns
    "c1-A20-E2-philox": ("c1", dict(action_dim=20), 2, dict(), "philox", False),  # 32 columns
    "c2-E1-philox": ("c2", {}, 1, dict(), "philox", False),                 # A = 38: 48 columns, 24 policy-prior rows
    "c2-pi0-E1-philox": ("c2", dict(num_pi_trajs=0), 1, dict(), "philox", False),  # every row sampled
    "c1-A64-H8-E1-philox": ("c1", dict(action_dim=64, horizon=8), 1, dict(), "philox", False),  # 64 columns: the tightest LDS
    "c2_ep-E1-philox": ("c2_ep", {}, 1, dict(), "philox", False),           # the episodic kernel
    "c1-fp32-E1-philox": ("c1", {}, 1, dict(), "philox", True),             # exact-fp32 arithmetic
    "c1-H1-E1-philox": ("c1", dict(horizon=1), 1, dict(), "philox", False),  # z_H with no earlier step
}

_models = {}


def case_model(name, overrides):
    """(case dict, oracle model) of a golden case's model with config overrides"""
    from oracle import cases
    from oracle import planner_oracle as po
    from tdmpc2_amd.config import named_config

    key = (name, tuple(sorted(overrides.items())))
    if key not in _models:
        if not overrides:
            c = cases.build_case(name)
        else:
            cfg_name, base, E, eval_mode, head_std = cases.CASES[name]
            c = cases.build_custom(named_config(cfg_name, **dict(base, **overrides)), E, eval_mode, head_std, name=name)
        _models[key] = (c, po.OracleModel(c["cfg"], {k: torch.as_tensor(v) for k, v in c["sd"].items()}))
    return _models[key]


def run_plan(name, overrides, E, tune, noise, fp32):
    """-> [action, prev_mean, the six debug stages] of the plan on the library tdmpc2_amd.native loads"""
    from tdmpc2_amd import native
    from tests.gpu_common import dev
    from tests.test_gpu_philox import _many_env_inputs

    c, model = case_model(name, overrides)
    planner = native.NativePlanner(c["cfg"], c["iterations"], dev(), max_envs=E, path=native.PATH_FUSED,
                                   precision=native.PREC_FP32 if fp32 else native.PREC_AUTO)
    planner.bind_state_dict(model.sd)
    if "rows" in tune:
        planner.set_rows_per_workgroup(tune["rows"])
    planner.set_cluster(0)
    inp = _many_env_inputs(c, model, E)
    prev = inp["prev_mean"].clone()
    kw = dict(task_emb=inp["task_emb"], act_mask=inp["act_mask"], debug=True)
    if noise == "tape":
        action, st = planner.plan(inp["z0"], inp["disc_pow"], prev, inp["t0"], tape=planner.export_noise(SEED, CALL, E), **kw)
    else:
        action, st = planner.plan(inp["z0"], inp["disc_pow"], prev, inp["t0"], tape=None, seed=PHILOX_SEED, **kw)
    torch.cuda.synchronize()
    faults = planner.take_fault()
    planner.close()
    assert faults == 0, (name, overrides, E, tune, "a bounded wait gave up")
    out = [action, prev] + [st[k] for k in STAGES]
    assert all(np.isfinite(t.float().cpu().numpy()).all() for t in out)
    return out


def run_row(rid):
    return digest(run_plan(*ROWS[rid]))
