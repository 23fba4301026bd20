"""The rows of tests/golden/fused_plan_digests.json: tape-driven calls of the fused family on every host route (per-tile 32- and
64-row workgroups, cluster, two clusters per tile, folded and separate refit, a trace call, a sharded plan), and the SHA-256 of
what each returns.  tools/make_fused_plan_digests.py mints the file from a library; tests/test_gpu_fused_route.py holds the
library under test to it bit for bit.  Public Python API only."""
import hashlib

import numpy as np
import torch

SEED, CALL = 0x5EED_F05E_D000_0001, 7  # the tape of every row: export_noise(SEED, CALL, E)
STAGES = ("value", "elite_idx", "score", "mean", "std", "actions")

# id: (kind, case, E, tuning)
ROWS = {
    "c1-E1-cluster2": ("plan", "c1", 1, dict(cluster=2)),
    "c1-E1-cluster1": ("plan", "c1", 1, dict(cluster=1)),
    "c1-E1-cluster0": ("plan", "c1", 1, dict(cluster=0)),
    "c2_ep-E1-cluster1": ("plan", "c2_ep", 1, dict(cluster=1)),
    "c1-E3-rows32-fold1-cluster0": ("plan", "c1", 3, dict(rows=32, fold=1, cluster=0)),
    "c1-E3-rows64-fold0": ("plan", "c1", 3, dict(rows=64, fold=0)),
    "c1-E16-auto": ("plan", "c1", 16, dict()),   # auto picks 32-row workgroups (0.61 x 1 round < 1 round) ...
    "c1-E32-auto": ("plan", "c1", 32, dict()),   # ... and 64-row ones (0.61 x 2 rounds > 1 round)
    "mt5-E5": ("plan", "mt5", 5, dict()),
    "c1-E2-trace": ("trace", "c1", 2, dict()),
    "c1-E2-shard": ("shard", "c1", 2, dict()),
}
# rows that wait on other workgroups (the cluster hand-overs): the only ones a mint may drop when two runs of one library differ
CLUSTER_ROWS = tuple(k for k, v in ROWS.items() if v[3].get("cluster", 0) > 0)


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        a = np.ascontiguousarray(t.detach().cpu().numpy())
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def run_row(rid):
    """The digest of row `rid` on the library tdmpc2_amd.native loads."""
    from oracle import cases
    from oracle import planner_oracle as po
    from tdmpc2_amd.native import NativePlanner
    from tests.gpu_common import dev
    from tests.test_gpu_philox import _many_env_inputs

    kind, name, E, tune = ROWS[rid]
    c = cases.build_case(name)
    cfg = c["cfg"]
    model = po.OracleModel(cfg, {k: torch.as_tensor(v) for k, v in c["sd"].items()})
    planner = NativePlanner(cfg, c["iterations"], dev(), max_envs=E, path=1)
    planner.bind_state_dict(model.sd)
    if "rows" in tune:
        planner.set_rows_per_workgroup(tune["rows"])
    if "fold" in tune:
        planner.set_fold_refit(tune["fold"])
    if "cluster" in tune:
        planner.set_cluster(tune["cluster"])
    inp = _many_env_inputs(c, model, E)
    tape = planner.export_noise(SEED, CALL, E)
    kw = dict(task_emb=inp["task_emb"], act_mask=inp["act_mask"])
    prev = inp["prev_mean"].clone()
    if kind == "plan":
        action, st = planner.plan(inp["z0"], inp["disc_pow"], prev, inp["t0"], tape=tape, debug=True, **kw)
        out = [action, prev] + [st[k] for k in STAGES]
    elif kind == "trace":
        N, H, A = cfg.num_samples, cfg.horizon, cfg.action_dim
        actions = torch.as_tensor(np.random.default_rng(3).uniform(-1, 1, (E, H, N, A)).astype(np.float32)).to(dev())
        out = list(planner.estimate_value(inp["z0"], inp["disc_pow"], actions, tape["pi_eps"][:, 0].contiguous(),
                                          tape["qidx"][:, 0].contiguous(), trace=True, **kw))
    else:  # one process, two row ranges per iteration
        N = cfg.num_samples
        action = torch.empty(E, cfg.action_dim, device=dev())
        st = planner.debug_buffers(E)
        value = torch.zeros(E, N, device=dev())
        planner.shard_begin(inp["z0"], prev, inp["t0"], tape=tape, **kw)
        for it in range(c["iterations"]):
            for r0, r1 in ((0, N // 2), (N // 2, N)):
                planner.shard_values(it, r0, r1, inp["z0"], inp["disc_pow"], value, act_mask=inp["act_mask"])
            planner.shard_refit(it, value, prev, action, act_mask=inp["act_mask"], stages=st)
        out = [action, prev] + [st[k] for k in STAGES]
    torch.cuda.synchronize()
    faults = planner.take_fault()
    planner.close()
    assert faults == 0, (rid, "a bounded wait gave up")
    return digest(out)
