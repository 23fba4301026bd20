"""Policy-prior latency (act() with cfg.mpc == False, tdmpc2/tdmpc2.py:114-120): the PyTorch-ROCm route (WorldModel.encode + pi)
against the library's row and spread routes (tdmpc2_plan_act_pi, TDMPC2_TUNE_POLICY_ROUTE) on the 5M (c2) and 48M (c3) models at
E = 1 (act()) and E = 256 (act_policy_batch), plus the two routes alone (NativePlanner.act_pi) on the 5M, 19M and 48M models at
several row counts -- the measurement behind policy_route.h's threshold.  Medians of CUDA-event timings after warm-up, one process.
MI355X box:

    python tools/policy_latency.py > out.json
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ROUTES = {"row": 1, "spread": 2}


def _timed(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def _agent(name, max_envs):
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.tdmpc2 import TDMPC2

    cfg = named_config(name, mpc=False)
    torch.manual_seed(0)
    agent = TDMPC2(cfg, device=torch.device("cuda", 0), max_envs=max_envs)
    agent.planner()
    return agent


def act_times(name):
    """act() at E = 1 and act_policy_batch at E = 256: torch route, native row route, native spread route (microseconds)."""
    agent = _agent(name, 256)
    cfg = agent.cfg
    g = torch.Generator().manual_seed(1)
    obs1 = torch.randn(cfg.obs_shape["state"][0], generator=g)
    obs256 = torch.randn(256, cfg.obs_shape["state"][0], generator=g)
    task1 = 0 if cfg.multitask else None
    tasks256 = torch.arange(256) % len(cfg.tasks) if cfg.multitask else None
    res = {}
    for way in ("torch", "row", "spread"):
        agent.native_policy = way != "torch"
        if way != "torch":
            agent.act(obs1, task=task1)  # binds the policy copy
            agent.planner().set_policy_route(ROUTES[way])
        with torch.no_grad():
            res[way] = {"E1_act_us": round(_timed(lambda: agent.act(obs1, task=task1), reps=100), 1),
                        "E256_act_us": round(_timed(lambda: agent.act_policy_batch(obs256, tasks=tasks256), reps=30), 1)}
    agent.planner().set_policy_route(0)
    return res


def route_times(name, rows=(1, 8, 64, 256)):
    """NativePlanner.act_pi (observation -> action, no host copy) per route and row count (microseconds)."""
    agent = _agent(name, max(rows))
    cfg, p = agent.cfg, agent.planner()
    agent._bind_policy()
    dev = agent.device
    res = {}
    for E in rows:
        obs = torch.randn(E, cfg.obs_shape["state"][0], device=dev)
        eps = torch.randn(E, cfg.action_dim, device=dev)
        emb = mask = None
        if cfg.multitask:
            t = torch.arange(E, device=dev) % len(cfg.tasks)
            emb = agent.model._task_emb(t).detach().contiguous()
            mask = agent.model._action_masks[t].contiguous()
        for way, mode in ROUTES.items():
            p.set_policy_route(mode)
            res.setdefault(way, {})[f"E{E}_us"] = round(_timed(lambda: p.act_pi(obs, task_emb=emb, act_mask=mask, eps=eps)), 1)
    p.set_policy_route(0)
    return res


def main():
    out = {"device": torch.cuda.get_device_name(0), "routes": {}, "act": {}}
    for name in ("c2", "m19_mt30", "c3"):
        out["routes"][name] = route_times(name)
        print(json.dumps({name: out["routes"][name]}), file=sys.stderr, flush=True)
    for name in ("c2", "c3"):
        out["act"][name] = act_times(name)
        print(json.dumps({name: out["act"][name]}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
