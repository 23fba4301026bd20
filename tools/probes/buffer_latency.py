"""Replay buffer: one `Buffer.sample()` (two launches: draw, grouped gather) against the same batch built from torch on the same
GPU -- per-field advanced indexing with a ready-made flat index, then view, permute and contiguous, which is what the reference's
torchrl path does underneath -- at B = 256, H = 3 with state observations of 24 and 223 dims and with uint8 [9, 64, 64] frame
stacks.  One process, the ways interleaved: ROUNDS rounds, in each the time of CALLS back-to-back calls between two device events
(single calls are too short for an event pair), divided by CALLS; reported are the median of the rounds and their spread.  Also
recorded: the bytes a sample moves (read + written), what fraction of the 6.29 TB/s float4-copy rate that is at the measured
time (recorded, not gated: the state shapes move under 1 MB and are launch-bound), and the same two launches replayed from a
hipGraph (the device side alone).  GATE: the library call is no slower than the torch composition at every shape; the script
exits 1 otherwise.  MI355X box:

    python tools/probes/buffer_latency.py            # writes profiles/buffer_latency.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ROUNDS, CALLS, WARM = 7, 200, 20
COPY_RATE = 6.29e12  # bytes / s: the measured float4 copy on this part
B, H = 256, 3
SHAPES = {  # name -> (per-step obs shape, obs dtype, action_dim, capacity, episodes, episode length)
    "state24": ((24,), torch.float32, 6, 100_000, 100, 500),
    "state223": ((223,), torch.float32, 38, 100_000, 100, 500),
    "rgb": ((9, 64, 64), torch.uint8, 6, 8_000, 16, 250),
}


def _per_call_us(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS


def _interleaved(fns):
    rounds = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            rounds[k].append(_per_call_us(fn))
    return {k: {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2), "rounds_us": [round(x, 2) for x in v]}
            for k, v in rounds.items()}


def one_shape(name):
    from tdmpc2_amd import Buffer
    from tdmpc2_amd.config import named_config

    obs_shape, obs_dtype, A, cap, n_eps, T = SHAPES[name]
    dev = torch.device("cuda", 0)
    cfg = named_config("c1", horizon=H)
    cfg.batch_size, cfg.buffer_size, cfg.action_dim = B, cap, A
    g = torch.Generator().manual_seed(0)
    if obs_dtype == torch.uint8:
        obs = torch.randint(0, 256, (n_eps, T) + obs_shape, generator=g, dtype=torch.uint8).to(dev)
    else:
        obs = torch.randn((n_eps, T) + obs_shape, generator=g).to(dev)
    td = {"obs": obs, "action": (torch.rand(n_eps, T, A, generator=g) * 2 - 1).to(dev), "reward": torch.randn(n_eps, T, generator=g).to(dev)}
    buf = Buffer(cfg, device=dev, seed=1)
    buf.load(td)
    # the torch composition reads the same rows: flat storage (no wrap here: logical == physical), slice-major flat index as torchrl's
    # sampler returns it, ready-made (drawing it is not charged)
    flat = {k: v.reshape((n_eps * T,) + tuple(v.shape[2:])) for k, v in td.items()}
    index = buf.sample(return_index=True)[-1]
    idx = (index[:, None] + torch.arange(H + 1, device=dev)[None, :]).reshape(-1)

    def torch_way():
        o = flat["obs"][idx].view(B, H + 1, *obs_shape).transpose(0, 1).contiguous()
        a = flat["action"][idx].view(B, H + 1, A).transpose(0, 1)[1:].contiguous()
        r = flat["reward"][idx].view(B, H + 1).transpose(0, 1)[1:].unsqueeze(-1).contiguous()
        return o, a, r, torch.zeros_like(r), None

    # same values both ways, at the size timed
    buf.native.set_call_counter(0)
    got, want = buf.sample(), torch_way()
    assert all(torch.equal(x, y) for x, y in zip(got[:4], want[:4]))

    res = _interleaved({"library": buf.sample, "torch": torch_way})
    # the two launches alone, replayed from a graph
    nat = buf.native
    outs = [torch.empty((sc, B, rb), dtype=torch.uint8, device=dev) for rb, _, sc in nat.fields]
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        nat.sample(outs, seed=1)
    res.update(_interleaved({"library_graph_replay": gr.replay}))
    moved = 2 * sum(rb * sc * B for rb, _, sc in nat.fields)
    res["bytes_moved"] = moved
    for k in ("library", "library_graph_replay"):
        res[k]["fraction_of_copy_rate"] = round(moved / (res[k]["median_us"] * 1e-6) / COPY_RATE, 4)
    res["torch_over_library"] = round(res["torch"]["median_us"] / res["library"]["median_us"], 2)
    res["gate_library_not_slower"] = res["library"]["median_us"] <= res["torch"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "buffer_latency.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU: there is nothing to report without one"
    out = {"device": torch.cuda.get_device_name(0), "B": B, "H": H, "rounds": ROUNDS,
           "per_round": f"{CALLS} back-to-back calls between two device events after {WARM} warm-ups, per call",
           "copy_rate_bytes_per_s": COPY_RATE, "shapes": {}}
    with torch.no_grad():
        for name in SHAPES:
            out["shapes"][name] = one_shape(name)
    out["gate_passed"] = all(s["gate_library_not_slower"] for s in out["shapes"].values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if out["gate_passed"] else 1


if __name__ == "__main__":
    sys.exit(main())
