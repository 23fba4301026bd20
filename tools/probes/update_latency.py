"""One eager training step, `TDMPC2.update(buffer)`, on the 5M model for dog-run (H 3, B 256, cfg.dropout 0.01, `native_autograd`,
`native_refresh` and `native_dropout` on), three ways on one agent, the setting toggled between rounds:

    compare_consts   `native_draws` off and the optimiser step as it was before it stopped comparing: the raw `ClipAdam.step()`, then
                     `sync_planner_weights()` alone -- the comparison of log_std_min / log_std_dif with the handle's (two
                     `float(device_tensor)` reads, hence two stream synchronisations) and ONE re-pack, as in the other two ways
    draws_off        `native_draws` off: the host seed and the framework's generator, no comparison
    draws_on         `native_draws` on: both draws of the step from `autograd.Draws` (two launches each)

and the draw unit alone at the step's two shapes against `torch.randn` + `torch.randperm(num_q)[:2]`.  Interleaved in one process:
ROUNDS rounds, in each the time of CALLS back-to-back repetitions between two device events, divided by CALLS; reported are the
median of the rounds and their spread.  Also recorded: the library calls of the stateless units per step (their host-side counters).
A step replayed from a graph is not measured: capturing the whole step is not part of the package.
`--count-launches` is a run of its own: one `update(buffer)` with `native_draws` on under torch.profiler's device trace, the count of
its device activities (kernels, copies and fills, the library's launches included) merged into the file the first run wrote.
`--multitask` is the multitask arm, a file of its own: the `mt5` model (30 tasks, task_dim 64), H 3, B 256, the same flags and
`native_draws` on, `native_task_emb` off and on toggled between rounds by the same protocol; with `--count-launches` the device
activities of one step with the flag off and of one with it on.
`--rgb` is the rgb arm, a file of its own: the 5M model on 9 x 64 x 64 uint8 frame stacks (C 32), H 3, B 256, the same flags and
`native_draws` on, `native_pixel_grad` off (MIOpen convolutions and grid_sample under autograd) and on (the pixel unit, forward and
backward) toggled between rounds by the same protocol.
Measured, not gated: the script always exits 0.  MI355X box:

    python tools/probes/update_latency.py                    # writes profiles/update_latency.json
    python tools/probes/update_latency.py --count-launches   # adds the launches per step to it
    python tools/probes/update_latency.py --multitask                    # writes profiles/update_latency_mt.json
    python tools/probes/update_latency.py --multitask --count-launches   # adds both launch counts to it
    python tools/probes/update_latency.py --rgb                          # writes profiles/update_latency_rgb.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROUNDS, CALLS, WARM = 7, 5, 3
DRAW_CALLS_PER_ROUND = 20
P = 0.01
B = 256


def _per_call_us(fn, calls):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def _interleaved(fns, calls):
    rounds = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            rounds[k].append(_per_call_us(fn, calls))
    return {k: {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2), "rounds_us": [round(x, 2) for x in v]}
            for k, v in rounds.items()}


def _buffer(cfg, dev, episodes=8):
    from tdmpc2_amd import Buffer

    A, od = cfg.action_dim, cfg.obs_shape["state"][0]
    rng = np.random.default_rng(17)
    buf = Buffer(cfg, device=dev, seed=5)
    for e in range(episodes):
        T = 501
        td = {"obs": torch.as_tensor(rng.standard_normal((T, od)).astype(np.float32)),
              "action": torch.as_tensor(rng.uniform(-1, 1, (T, A)).astype(np.float32)),
              "reward": torch.as_tensor(rng.standard_normal(T).astype(np.float32))}
        if cfg.multitask:  # one task per episode, every task of the set
            td["task"] = torch.full((T,), e % len(cfg.tasks), dtype=torch.int64)
        buf.add(td)
    return buf


def _agent_and_buffer(name="c2"):
    from tdmpc2_amd import TDMPC2
    from tdmpc2_amd.config import named_config

    dev = torch.device("cuda", 0)
    cfg = named_config(name, dropout=P, batch_size=B, buffer_size=20_000)
    torch.manual_seed(5)
    agent = TDMPC2(cfg, device=dev)
    with torch.no_grad():
        for _, p in agent.model.named_parameters():
            p.add_(torch.randn_like(p) * 0.02)
    agent.native_autograd = agent.native_refresh = agent.native_dropout = True
    agent.planner()
    return agent, cfg, _buffer(cfg, dev, len(cfg.tasks) if cfg.multitask else 8)


def measure_update():
    from tdmpc2_amd import native

    agent, cfg, buf = _agent_and_buffer()
    step_without = agent.optimizer_step

    def step_with(which="model"):  # the optimiser step as it was: the raw step, then the comparison and one re-pack -- never both re-packs
        norm = (agent.optim if which == "model" else agent.pi_optim).step()
        agent.sync_planner_weights()
        return norm

    def run(draws, compare):
        def fn():
            agent.native_draws = draws
            agent.optimizer_step = step_with if compare else step_without
            agent.update(buf)
        return fn

    ways = {"compare_consts": run(False, True), "draws_off": run(False, False), "draws_on": run(True, False)}
    res = _interleaved(ways, CALLS)
    names = ("LAYER_CALLS", "LOSS_CALLS", "PI_GRAD_CALLS", "DROPOUT_CALLS", "DRAW_CALLS")
    before = {n: getattr(native, n) for n in names}
    ways["draws_on"]()
    torch.cuda.synchronize()
    res["unit_calls_per_step_draws_on"] = {n: getattr(native, n) - before[n] for n in names}
    res["draws_on_over_draws_off"] = round(res["draws_on"]["median_us"] / res["draws_off"]["median_us"], 4)
    res["draws_off_over_compare_consts"] = round(res["draws_off"]["median_us"] / res["compare_consts"]["median_us"], 4)
    res["shape"] = {"H": cfg.horizon, "B": B, "A": cfg.action_dim, "num_q": cfg.num_q, "mlp_dim": cfg.mlp_dim}
    return res


def measure_draws():
    from tdmpc2_amd import autograd
    from tdmpc2_amd.config import named_config

    dev = torch.device("cuda", 0)
    cfg = named_config("c2")
    draws = autograd.Draws(1, dev)
    res = {}
    for name, steps in (("td_target", cfg.horizon), ("update_pi", cfg.horizon + 1)):
        shape = (steps, B, cfg.action_dim)
        r = _interleaved({"library": lambda s=shape: draws.draw(s, cfg.num_q),
                          "torch": lambda s=shape: (torch.randn(s, device=dev), torch.randperm(cfg.num_q, device=dev)[:2])},
                         DRAW_CALLS_PER_ROUND)
        r["shape"], r["library_launches"] = list(shape), 2
        res[name] = r
    return res


def count_launches():
    """Device activities of one eager `update(buffer)` with `native_draws` on, by name: what one step puts on the stream."""
    from collections import Counter

    from torch.profiler import ProfilerActivity, profile

    agent, _, buf = _agent_and_buffer()
    agent.native_draws = True
    for _ in range(WARM):
        agent.update(buf)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        agent.update(buf)
        torch.cuda.synchronize()
    names = Counter(e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    copies = sum(n for k, n in names.items() if k.lower().startswith(("memcpy", "memset")) or "copybuffer" in k.lower() or "fillbuffer" in k.lower())
    total = sum(names.values())
    return {"device_activities": total, "of_which_copies_and_fills": copies, "kernels": total - copies, "distinct_names": len(names),
            "most_frequent": [[k[:80], n] for k, n in names.most_common(12)]}


UNIT_COUNTERS = ("LAYER_CALLS", "LOSS_CALLS", "PI_GRAD_CALLS", "DROPOUT_CALLS", "DRAW_CALLS", "TASK_CALLS")


def measure_update_mt():
    """The multitask step (`mt5`, H 3, B 256) with `native_task_emb` off and on, interleaved on one agent."""
    from tdmpc2_amd import native

    agent, cfg, buf = _agent_and_buffer("mt5")
    agent.native_draws = True

    def run(on):
        def fn():
            agent.native_task_emb = on
            agent.update(buf)
        return fn

    ways = {"task_emb_off": run(False), "task_emb_on": run(True)}
    res = _interleaved(ways, CALLS)
    for k, fn in ways.items():
        before = {n: getattr(native, n) for n in UNIT_COUNTERS}
        fn()
        torch.cuda.synchronize()
        res["unit_calls_per_step_" + k] = {n: getattr(native, n) - before[n] for n in UNIT_COUNTERS}
    res["task_emb_on_over_off"] = round(res["task_emb_on"]["median_us"] / res["task_emb_off"]["median_us"], 4)
    res["shape"] = {"H": cfg.horizon, "B": B, "A": cfg.action_dim, "num_q": cfg.num_q, "mlp_dim": cfg.mlp_dim, "tasks": len(cfg.tasks),
                    "task_dim": cfg.task_dim}
    return res


def count_launches_mt():
    """Device activities of one eager multitask `update(buffer)` with `native_task_emb` off, then on (one agent, one process)."""
    from collections import Counter

    from torch.profiler import ProfilerActivity, profile

    agent, _, buf = _agent_and_buffer("mt5")
    agent.native_draws = True
    out = {}
    for key, on in (("task_emb_off", False), ("task_emb_on", True)):
        agent.native_task_emb = on
        for _ in range(WARM):
            agent.update(buf)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            agent.update(buf)
            torch.cuda.synchronize()
        names = Counter(e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        copies = sum(n for k, n in names.items() if k.lower().startswith(("memcpy", "memset")) or "copybuffer" in k.lower() or "fillbuffer" in k.lower())
        total = sum(names.values())
        out[key] = {"device_activities": total, "of_which_copies_and_fills": copies, "kernels": total - copies,
                    "task_unit_kernels": sum(n for k, n in names.items() if "k_task_" in k), "distinct_names": len(names),
                    "most_frequent": [[k[:80], n] for k, n in names.most_common(12)]}
    out["fewer_with_the_flag_on"] = out["task_emb_off"]["device_activities"] - out["task_emb_on"]["device_activities"]
    return out


def measure_update_rgb():
    """The rgb step (5M model, 9 x 64 x 64 uint8 frames, H 3, B 256) with `native_pixel_grad` off and on, interleaved on one agent."""
    from tdmpc2_amd import TDMPC2, Buffer, native
    from tdmpc2_amd.config import named_config

    dev = torch.device("cuda", 0)
    cfg = named_config("c2", dropout=P, batch_size=B, buffer_size=2_000)
    cfg.obs, cfg.obs_shape, cfg.num_channels, cfg.latent_dim = "rgb", {"rgb": (9, 64, 64)}, 32, 512
    torch.manual_seed(5)
    agent = TDMPC2(cfg, device=dev)
    agent.native_autograd = agent.native_refresh = agent.native_dropout = agent.native_draws = True
    agent.planner()
    rng = np.random.default_rng(17)
    buf = Buffer(cfg, device=dev, seed=5)
    for _ in range(8):
        T = 101
        buf.add({"obs": torch.as_tensor(rng.integers(0, 256, (T, 9, 64, 64), dtype=np.uint8)),
                 "action": torch.as_tensor(rng.uniform(-1, 1, (T, cfg.action_dim)).astype(np.float32)),
                 "reward": torch.as_tensor(rng.standard_normal(T).astype(np.float32))})

    def run(on):
        def fn():
            agent.native_pixel_grad = on
            agent.update(buf)
        return fn

    ways = {"pixel_grad_off": run(False), "pixel_grad_on": run(True)}
    res = _interleaved(ways, CALLS)
    counters = UNIT_COUNTERS + ("PIXEL_GRAD_CALLS",)
    for k, fn in ways.items():
        before = {n: getattr(native, n) for n in counters}
        fn()
        torch.cuda.synchronize()
        res["unit_calls_per_step_" + k] = {n: getattr(native, n) - before[n] for n in counters}
    res["pixel_grad_on_over_off"] = round(res["pixel_grad_on"]["median_us"] / res["pixel_grad_off"]["median_us"], 4)
    res["shape"] = {"H": cfg.horizon, "B": B, "A": cfg.action_dim, "C": 32, "cin": 9, "frames_per_step": (cfg.horizon + 1) * B}
    return res


def main_rgb(a):
    path = a.out or os.path.join(ROOT, "profiles", "update_latency_rgb.json")
    out = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "gated": False,
           "per_round": f"{CALLS} back-to-back repetitions between two device events after {WARM} warm-ups, per repetition",
           "graph_replay": "not measured: capturing the whole step is not part of the package"}
    try:
        out["update"] = measure_update_rgb()
    except Exception as e:  # measured, not gated
        out["update"] = {"not_measured": f"{type(e).__name__}: {str(e)[:300]}"}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


def main_mt(a):
    path = a.out or os.path.join(ROOT, "profiles", "update_latency_mt.json")
    out = {}
    if a.count_launches and os.path.exists(path):
        with open(path) as f:
            out = json.load(f)
    key, fn = ("launches_of_one_update", count_launches_mt) if a.count_launches else ("update", measure_update_mt)
    if not a.count_launches:
        out = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "gated": False,
               "per_round": f"{CALLS} back-to-back repetitions between two device events after {WARM} warm-ups, per repetition",
               "graph_replay": "not measured: capturing the whole step is not part of the package"}
    try:
        out[key] = fn()
    except Exception as e:  # measured, not gated
        out[key] = {"not_measured": f"{type(e).__name__}: {str(e)[:300]}"}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--count-launches", action="store_true")
    ap.add_argument("--multitask", action="store_true")
    ap.add_argument("--rgb", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU: there is nothing to report without one"
    if a.rgb:
        return main_rgb(a)
    if a.multitask:
        return main_mt(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "update_latency.json")
    if a.count_launches:
        out = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                out = json.load(f)
        try:
            out["launches_of_one_update_draws_on"] = count_launches()
        except Exception as e:
            out["launches_of_one_update_draws_on"] = {"not_measured": f"{type(e).__name__}: {str(e)[:200]}"}
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return 0
    out = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS,
           "per_round": f"{CALLS} ({DRAW_CALLS_PER_ROUND} for a draw) back-to-back repetitions between two device events after {WARM} "
                        "warm-ups, per repetition",
           "graph_replay": "not measured: capturing the whole step is not part of the package", "gated": False}
    for key, fn in (("update", measure_update), ("draw", measure_draws)):
        try:
            out[key] = fn()
        except Exception as e:  # measured, not gated
            out[key] = {"not_measured": f"{type(e).__name__}: {str(e)[:300]}"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
