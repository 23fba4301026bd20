"""Pixel encoder latency: the library's encoder (tdmpc2_plan_encode_pix) against the PyTorch-ROCm module (layers.conv) at E = 1, 8
and 256, and one act() step of a c1-sized rgb agent with each, in one process (CUDA-event medians).  MI355X box:

    python tools/pixel_latency.py > out.json                       # the timings
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/pixel_latency.py --act-loop native   # launches per act() step
    python tools/pixel_latency.py --count-trace DIR/.../kernel_trace.csv --steps 20             # ... counted
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ACT_STEPS = 20


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


def _agent(native):
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.tdmpc2 import TDMPC2

    cfg = named_config("c1")
    cfg.obs, cfg.obs_shape = "rgb", {"rgb": (9, 64, 64)}
    torch.manual_seed(0)
    agent = TDMPC2(cfg, device=torch.device("cuda", 0))
    agent.native_pixel_encoder = native
    agent.planner()
    return agent


def encoder_times():
    from tdmpc2_amd import layers
    from tdmpc2_amd.native import NativePlanner

    dev = torch.device("cuda", 0)
    agent = _agent(True)
    p = agent.planner()
    out = {}
    big = NativePlanner(agent.cfg, agent.cfg.iterations, dev, max_envs=256)
    big.bind_pixel_encoder({k: v for k, v in agent.model.state_dict().items() if k.startswith("_encoder.rgb.")})
    m = agent.model._encoder["rgb"]
    for E in (1, 8, 256):
        obs = torch.randint(0, 256, (E, 9, 64, 64), device=dev, dtype=torch.uint8)
        shift = NativePlanner.draw_shift(E, dev)
        h = p if E == 1 else big
        with torch.no_grad():
            t_nat = _timed(lambda: h.encode_pix(obs, shift))
            t_torch = _timed(lambda: m(obs))  # ShiftAug's x.float() included, as in act()
        out[f"E{E}"] = {"native_us": round(t_nat, 1), "torch_us": round(t_torch, 1)}
    return out


def act_times():
    res = {}
    g = torch.Generator().manual_seed(1)
    obs = torch.randint(0, 256, (9, 64, 64), generator=g, dtype=torch.uint8)
    for native in (True, False):
        agent = _agent(native)
        agent.act(obs, t0=True)
        res["native" if native else "torch"] = {"act_us": round(_timed(lambda: agent.act(obs), reps=30), 1)}
    return res


def act_loop(mode):
    agent = _agent(mode == "native")
    obs = torch.randint(0, 256, (9, 64, 64), dtype=torch.uint8)
    agent.act(obs, t0=True)
    torch.cuda.synchronize()
    for _ in range(ACT_STEPS):
        agent.act(obs)
    torch.cuda.synchronize()


def count_trace(path, steps):
    """Kernel dispatches in a rocprofv3 kernel trace whose names are not the set-up's (per act() step, last `steps` steps)."""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r.get("Start_Timestamp", 0)))
    names = [r.get("Kernel_Name", "") for r in rows]
    return {"dispatches": len(names), "per_step_upper_bound": round(len(names) / steps, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--act-loop", choices=["native", "torch"])
    ap.add_argument("--count-trace")
    ap.add_argument("--steps", type=int, default=ACT_STEPS + 1)
    a = ap.parse_args()
    if a.count_trace:
        print(json.dumps(count_trace(a.count_trace, a.steps)))
        return
    if a.act_loop:
        act_loop(a.act_loop)
        return
    print(json.dumps({"device": torch.cuda.get_device_name(0), "encoder": encoder_times(), "act_step": act_times()}))


if __name__ == "__main__":
    main()
