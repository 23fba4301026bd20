"""Generator of tests/golden/policy.npz: the reference's own WorldModel.encode + WorldModel.pi (tdmpc2/common/world_model.py:103-112,
144-184) on a few rows of five cases, run on the CPU in fp32 with the synthetic weights of oracle.cases and the policy's
torch.randn_like served from a recorded tape.  Only inputs and outputs are stored (obs, task ids, eps, z, action, mean, log_std,
entropy, scaled_entropy), under keys "<case>.<field>".  Needs the reference tree (oracle.ref_runner.available()).

    python tools/make_policy_golden.py            # writes tests/golden/policy.npz
"""
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "policy.npz")

# case: task ids of the rows (None: single-task; the number of rows is the length of the list, or the int given).  The
# multitask cases' rows belong to tasks whose action masks differ (oracle.cases: action_dims = A - (task % 3)).
CASES = {
    "tiny": 3,                 # small dims, row route
    "c2": 2,                   # dog-run 5M, A = 38: row route
    "m19_mt30": [0, 1, 2],     # 19M multitask (L512 M1024 T64): spread route
    "c3": [0, 1, 2],           # mt30 48M (L768 M1792 T64): spread route
    "c4": [0, 1],              # mt80 317M (L1376 M4096 T96): widths of 4096
}
FIELDS = ("obs", "tasks", "eps", "z", "action", "mean", "log_std", "entropy", "scaled_entropy")


def rows(name):
    spec = CASES[name]
    return (spec, None) if isinstance(spec, int) else (len(spec), np.asarray(spec, np.int64))


def inputs(cfg, name):
    """obs [n, obs_dim] and eps [n, A] of a case (deterministic)."""
    from tdmpc2_amd import synth

    n, _ = rows(name)
    obs = synth.make_obs(cfg, n, seed=17)
    eps = np.random.default_rng(23).standard_normal((n, cfg.action_dim)).astype(np.float32)
    return obs, eps


def run_case(name):
    from oracle import cases, ref_runner

    c = cases.build_case(name)
    cfg = c["cfg"]
    sd = {k: torch.as_tensor(v) for k, v in c["sd"].items()}
    agent = ref_runner.build_agent(cfg, sd, c["discounts"][0])
    n, tasks = rows(name)
    obs, eps = inputs(cfg, name)
    task_t = None if tasks is None else torch.as_tensor(tasks)
    saved = torch.randn_like

    def randn_like(x, **kw):
        assert tuple(x.shape) == eps.shape, (tuple(x.shape), eps.shape)
        return torch.as_tensor(eps).to(x.dtype).clone()

    torch.randn_like = randn_like
    try:
        with torch.no_grad():
            z = agent.model.encode(torch.as_tensor(obs), task_t)
            action, info = agent.model.pi(z, task_t)
    finally:
        torch.randn_like = saved
    out = {"obs": obs, "tasks": np.full(n, -1, np.int64) if tasks is None else tasks, "eps": eps, "z": z.numpy(),
           "action": action.numpy(), "mean": info["mean"].numpy(), "log_std": info["log_std"].numpy(),
           "entropy": info["entropy"].numpy(), "scaled_entropy": info["scaled_entropy"].numpy()}
    del agent, c, sd
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def generate():
    torch.set_num_threads(1)  # one thread: the same reduction order on every machine
    res = {}
    for name in CASES:
        for k, v in run_case(name).items():
            res[f"{name}.{k}"] = v
    return res


def main():
    from oracle import ref_runner

    if not ref_runner.available():
        raise SystemExit("the reference tree is not available: nothing to generate")
    res = generate()
    buf = io.BytesIO()
    np.savez_compressed(buf, **res)
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(f"wrote {OUT}: {len(buf.getvalue())} bytes, {len(res)} arrays")


if __name__ == "__main__":
    main()
