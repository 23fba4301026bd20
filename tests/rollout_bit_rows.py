"""The rows of tests/golden/rollout_plan_digests.json: tape-driven per-tile plans of the geometries tests/fused_plan_rows.py lacks
(the benched model at one, two and three plans; forced 32- and 64-row workgroups; the refit folded into the rollout launch; rollouts
of one and of two steps), and the SHA-256 of what each returns.  The file was minted from the library of the commit BEFORE the
rollout kernel's action block became sample_actions (a change of every ks_rollout instantiation's machine code and of none of its
arithmetic); tests/test_gpu_rollout_bits.py holds the library under test to it bit for bit.  Public Python API only.  To mint
(MI355X box, library of COMMIT, two processes):

    python -m tests.rollout_bit_rows COMMIT out_a.json
    python -m tests.rollout_bit_rows COMMIT out_b.json
    python -m tests.rollout_bit_rows --merge out_a.json out_b.json [tests/golden/rollout_plan_digests.json]
"""
import json
import os
import sys

import numpy as np
import torch

from tests.fused_plan_rows import CALL, SEED, STAGES, digest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_plan_digests.json")

# id: (case, horizon override or None, E, tuning); every row runs the per-tile kernel (cluster = 0)
ROWS = {
    "c2-E1-cluster0": ("c2", None, 1, dict(cluster=0)),
    "c2-E3-rows32": ("c2", None, 3, dict(rows=32, cluster=0)),
    "c2-E3-rows64": ("c2", None, 3, dict(rows=64, cluster=0)),
    "c2-E2-fold1": ("c2", None, 2, dict(fold=1, cluster=0)),
    "c1-H1-E2": ("c1", 1, 2, dict(cluster=0)),   # one step: the action block runs once
    "c1-H2-E2": ("c1", 2, 2, dict(cluster=0)),
}

_models = {}


def case_model(name, horizon=None):
    """(case dict, oracle model) of a golden case's model, optionally with another horizon"""
    from oracle import cases
    from oracle import planner_oracle as po
    from tdmpc2_amd.config import named_config

    key = (name, horizon)
    if key not in _models:
        if horizon is None:
            c = cases.build_case(name)
        else:
            cfg_name, overrides, E, eval_mode, head_std = cases.CASES[name]
            c = cases.build_custom(named_config(cfg_name, **dict(overrides, horizon=horizon)), E, eval_mode, head_std, name=name)
        _models[key] = (c, po.OracleModel(c["cfg"], {k: torch.as_tensor(v) for k, v in c["sd"].items()}))
    return _models[key]


def make_planner(c, model, E, tune):
    from tdmpc2_amd.native import NativePlanner
    from tests.gpu_common import dev

    planner = NativePlanner(c["cfg"], c["iterations"], dev(), max_envs=E, path=1)
    planner.bind_state_dict(model.sd)
    if "rows" in tune:
        planner.set_rows_per_workgroup(tune["rows"])
    if "fold" in tune:
        planner.set_fold_refit(tune["fold"])
    planner.set_cluster(tune.get("cluster", 0))
    return planner


def run_plan(name, horizon, E, tune):
    """-> [action, prev_mean, the six debug stages] of the tape-driven plan on the library tdmpc2_amd.native loads"""
    from tests.test_gpu_philox import _many_env_inputs

    c, model = case_model(name, horizon)
    planner = make_planner(c, model, E, tune)
    inp = _many_env_inputs(c, model, E)
    tape = planner.export_noise(SEED, CALL, E)
    prev = inp["prev_mean"].clone()
    action, st = planner.plan(inp["z0"], inp["disc_pow"], prev, inp["t0"], tape=tape, debug=True,
                              task_emb=inp["task_emb"], act_mask=inp["act_mask"])
    torch.cuda.synchronize()
    faults = planner.take_fault()
    planner.close()
    assert faults == 0, (name, horizon, E, tune, "a bounded wait gave up")
    out = [action, prev] + [st[k] for k in STAGES]
    assert all(np.isfinite(t.float().cpu().numpy()).all() for t in out)
    return out


def run_row(rid):
    return digest(run_plan(*ROWS[rid]))


def mint(commit, out):
    rows = {rid: run_row(rid) for rid in ROWS}
    with open(out, "w") as f:
        json.dump({"commit": commit, "rows": rows}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out, len(rows), "rows")


def merge(a, b, out):
    with open(a) as f:
        ja = json.load(f)
    with open(b) as f:
        jb = json.load(f)
    assert ja["commit"] == jb["commit"], "the two runs are of different commits"
    bad = sorted(k for k in ROWS if ja["rows"].get(k) != jb["rows"].get(k))
    assert not bad, f"per-tile rows differ between two runs of one library: {bad}"
    with open(out, "w") as f:
        json.dump({"commit": ja["commit"], "rows": ja["rows"]}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out, len(ja["rows"]), "rows, two runs agree")


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else GOLDEN)
    else:
        mint(sys.argv[1], sys.argv[2])
