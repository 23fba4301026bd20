"""Dropout masks: one `autograd.DropoutMasks.draw` (tdmpc2_dropout_mask: the mask kernel and the one-thread counter launch) against
`F.dropout(torch.ones(...))` on the same GPU, at the two mask shapes of the 5M model for dog-run -- [5, 3 * 256, 512] for the
value-loss pass of `_update` and [2, 4 * 256, 512] for `update_pi`'s pair -- eager and replayed from a hipGraph; then
`TDMPC2._update` end to end on that model with `native_dropout` off and on (cfg.dropout = 0.01, one agent, the flag toggled between
rounds).  Interleaved in one process: ROUNDS rounds, in each the time of CALLS back-to-back repetitions between two device events,
divided by CALLS; reported are the median of the rounds and their spread.  Measured, not gated: the script always exits 0.
MI355X box:

    python tools/probes/dropout_latency.py                    # writes profiles/dropout_latency.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

ROUNDS, CALLS, WARM = 7, 20, 5
UPDATE_CALLS = 5
SHAPES = {"value_pass": (5, 3 * 256, 512), "update_pi": (2, 4 * 256, 512)}
P = 0.01


def _per_call_us(fn, calls=CALLS):
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


def _interleaved(fns, calls=CALLS):
    rounds = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            rounds[k].append(_per_call_us(fn, calls))
    return {k: {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2), "rounds_us": [round(x, 2) for x in v]}
            for k, v in rounds.items()}


def draw_ways(shape):
    from tdmpc2_amd import autograd

    dev = torch.device("cuda", 0)
    masks = autograd.DropoutMasks(1, dev)
    ones = torch.ones(shape, device=dev)
    return (lambda: masks.draw(shape, P)), (lambda: F.dropout(ones, P, True))


def measure_draws():
    res = {}
    for name, shape in SHAPES.items():
        library, torch_way = draw_ways(shape)
        r = _interleaved({"library": library, "torch": torch_way})
        torch.cuda.synchronize()
        graphs = {}
        for key, fn in (("library_graph_replay", library), ("torch_graph_replay", torch_way)):
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    keep = fn()  # noqa: F841  (the graph's pool owns the output)
                graphs[key] = g.replay
            except Exception as e:  # measured, not gated: a way that does not capture is reported as such
                r[key] = {"capture_failed": f"{type(e).__name__}: {str(e)[:200]}"}
                torch.cuda.synchronize()
        if graphs:
            r.update(_interleaved(graphs))
        r["shape"] = list(shape)
        r["mask_bytes"] = 4 * shape[0] * shape[1] * shape[2]
        r["library_launches"] = 2
        r["torch_over_library"] = round(r["torch"]["median_us"] / r["library"]["median_us"], 2)
        res[name] = r
    return res


def measure_update():
    """TDMPC2._update on the 5M dog-run model (H 3, B 256) with cfg.dropout = 0.01: native_dropout off and on."""
    from tdmpc2_amd import TDMPC2
    from tdmpc2_amd.config import named_config

    dev = torch.device("cuda", 0)
    cfg = named_config("c2", dropout=P)
    torch.manual_seed(5)
    agent = TDMPC2(cfg, device=dev)
    with torch.no_grad():
        for _, p in agent.model.named_parameters():
            p.add_(torch.randn_like(p) * 0.02)
    agent.native_autograd = True
    agent.native_refresh = True
    agent.planner()
    H, B = cfg.horizon, 256
    obs = torch.randn(H + 1, B, cfg.obs_shape["state"][0], device=dev)
    action = torch.rand(H, B, cfg.action_dim, device=dev) * 2 - 1
    reward = torch.randn(H, B, 1, device=dev)

    def run(flag):
        def fn():
            agent.native_dropout = flag
            agent._update(obs, action, reward)
        return fn

    res = _interleaved({"flag_off": run(False), "flag_on": run(True)}, UPDATE_CALLS)
    res["on_over_off"] = round(res["flag_on"]["median_us"] / res["flag_off"]["median_us"], 4)
    res["shape"] = {"H": H, "B": B, "num_q": cfg.num_q, "mlp_dim": cfg.mlp_dim}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_latency.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU: there is nothing to report without one"
    out = {"device": torch.cuda.get_device_name(0), "p": P, "rounds": ROUNDS,
           "per_round": f"{CALLS} ({UPDATE_CALLS} for _update) back-to-back repetitions between two device events after {WARM} warm-ups, per repetition",
           "baseline": "F.dropout(torch.ones(shape), p, True) on the same GPU; _update with native_dropout off", "gated": False}
    out["draw"] = measure_draws()
    try:
        out["update"] = measure_update()
    except Exception as e:  # measured, not gated
        out["update"] = {"not_measured": f"{type(e).__name__}: {str(e)[:300]}"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
