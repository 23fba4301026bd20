"""Latency of telling the planner that the weights moved: the per-layer route (`bind_state_dict` + `bind_encoder` as
TDMPC2.sync_planner_weights calls them, their closing stream synchronisations included) against `refresh_state_dict` + one
stream synchronisation, and `torch.lerp_` on the target tensors + the 15 target binds against `soft_update_target`.
Models: c2 (5M, fused family), c3 (48M) and c4 (317M), target ensemble and state encoder bound.  The two ways alternate inside
one process; every measurement is taken with device events AND the wall clock (the per-layer route is host-bound on the small
model); every leg runs for at least a second per way after warm-up; medians and minima; the clocks and socket power under
each leg's load are recorded (bench.py's sampler).  No ratio is asserted.  MI355X box:

    python tools/refresh_latency.py [c2 c3 c4]     # writes profiles/refresh_latency.json
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _time_ways(fns, budget_s=1.0, warm=3, cap_s=90.0):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ev, wall = {k: [] for k in fns}, {k: [] for k in fns}
    t_end = time.time() + cap_s
    while min(sum(v) for v in wall.values()) < budget_s * 1e6 and time.time() < t_end:
        for k, fn in fns.items():  # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn()  # ends with its own stream synchronisation
            b.record()
            b.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e6)
            ev[k].append(a.elapsed_time(b) * 1e3)
    return {k: {"event_median_us": statistics.median(ev[k]), "event_min_us": min(ev[k]), "wall_median_us": statistics.median(wall[k]),
                "wall_min_us": min(wall[k]), "n": len(ev[k]), "wall_s": round(sum(wall[k]) * 1e-6, 3),
                "budget_reached": sum(wall[k]) >= budget_s * 1e6} for k in fns}


def leg(name):
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.native import NET_TARGET_Q, _ptr
    from tdmpc2_amd.tdmpc2 import TDMPC2

    cfg = named_config(name)
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    agent = TDMPC2(cfg, device=dev, max_envs=1)
    agent.model.eval()
    pl = agent.planner()
    stream = torch.cuda.current_stream(dev)
    sd = agent._refresh_state_dict()
    enc = {k: v for k, v in sd.items() if k.startswith("_encoder.state.")}
    tq = {k: v for k, v in sd.items() if k.startswith("_target_Qs_params.")}
    q = {k.replace("_target_Qs_params.", "_Qs.params."): None for k in tq}
    for k in q:
        q[k] = sd[k]

    def bind_route():  # what sync_planner_weights() does by default
        pl.bind_state_dict(agent.model.planner_state_dict())
        if enc:
            pl.bind_encoder(enc)

    def refresh_route():
        pl.refresh_state_dict(sd)
        stream.synchronize()

    def lerp_and_bind():
        with torch.no_grad():
            for k, t in tq.items():
                t.lerp_(q[k.replace("_target_Qs_params.", "_Qs.params.")], cfg.tau)
        for layer in range(3):  # 3 layers x num_q members
            t = [tq.get(f"_target_Qs_params.{layer}.{n}") for n in ("weight", "bias", "ln.weight", "ln.bias")]
            pl._check(pl.lib.tdmpc2_plan_bind_weights(pl._h, NET_TARGET_Q, layer, _ptr(t[0]), _ptr(t[1]), _ptr(t[2]), _ptr(t[3]),
                                                      int(t[0].shape[-2]), int(t[0].shape[-1]), pl._stream()))
        stream.synchronize()

    def soft_update():
        pl.soft_update_target(sd, cfg.tau)
        stream.synchronize()

    res = {"case": name, "path": pl.path, "precision": pl.precision, "num_q": int(cfg.num_q),
           "weight_floats": int(sum(v.numel() for v in sd.values())), "device_bytes": pl.device_bytes}
    res["weights"] = _time_ways({"bind": bind_route, "refresh": refresh_route})
    res["soft_update"] = _time_ways({"lerp_bind": lerp_and_bind, "native": soft_update})
    from bench import box_under_load  # the clocks / socket power under this leg's own load, as bench.py samples them

    def queue():
        for _ in range(50):
            refresh_route()
    res["clocks_under_load"] = box_under_load(queue, dev)
    agent._planner.close()
    return res


def main():
    names = sys.argv[1:] or ["c2", "c3", "c4"]
    out = {"legs": [leg(n) for n in names]}
    path = os.path.join(ROOT, "profiles", "refresh_latency.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
