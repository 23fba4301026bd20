"""Pixel encoder in training: forward + backward of the convolutional encoder at n = 256 frame stacks, C = 32, cin = 9 (the 5M rgb
model's batch), through the C ABI (tdmpc2_pixgrad_forward + tdmpc2_pixgrad_backward, every dW / db) against torch autograd of
`layers.conv` on the same GPU (MIOpen convolutions, grid_sample) with the same shifts and a ready-made dz.  One process, the ways
interleaved: ROUNDS rounds, in each the time of CALLS back-to-back forward + backward pairs between two device events, divided by
CALLS; reported are the median of the rounds and their spread.  Also recorded: the library pair replayed from a hipGraph, the device
activities of one pair on both sides (torch.profiler's device trace, a pass of its own) and the unit's workspace sizes at this n.
Measured, not gated: the script always exits 0.  MI355X box:

    python tools/probes/pixel_grad_latency.py        # writes profiles/pixel_grad_latency.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ROUNDS, CALLS, WARM = 7, 10, 3
N, C, CIN = 256, 32, 9


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


def _activities(fn):
    from collections import Counter

    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = Counter(e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    return {"device_activities": sum(names.values()), "most_frequent": [[k[:80], n] for k, n in names.most_common(16)]}


def measure():
    from tdmpc2_amd import layers, native

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    seq = layers.conv((CIN, 64, 64), C, act=layers.SimNorm(8)).to(dev)
    obs = torch.randint(0, 256, (N, CIN, 64, 64), dtype=torch.uint8, device=dev)
    shift = native.NativePlanner.draw_shift(N, dev)
    dz = torch.randn(N, 16 * C, device=dev)
    convs = [seq[i] for i in (2, 4, 6, 8)]
    Ws, bs = [m.weight.detach().contiguous() for m in convs], [m.bias.detach().contiguous() for m in convs]
    d = native.pixgrad_desc(N, CIN, C, 0)
    ab, fb, bb = native.pixgrad_workspace_bytes(d)
    mk = lambda nbytes: torch.empty(nbytes // 4, dtype=torch.float32, device=dev)  # noqa: E731
    acts, fwd_ws, bwd_ws = mk(ab), mk(fb), mk(bb)
    dW, db = [torch.empty_like(w) for w in Ws], [torch.empty_like(b) for b in bs]
    tab = native.pixgrad_shift_table(dev)

    def library():
        native.pixgrad_forward(d, obs, shift, tab, Ws, bs, fwd_ws, acts)
        native.pixgrad_backward(d, obs, shift, tab, Ws, acts, dz, bwd_ws, dW, db)

    params = [t for m in convs for t in (m.weight, m.bias)]
    pinned = shift.to(torch.float32).view(N, 1, 1, 2)
    real = torch.randint

    def torch_way():
        torch.randint = lambda *a, **k: pinned.clone()   # ShiftAug's draw, pinned to the library's shifts
        try:
            z = seq(obs)
        finally:
            torch.randint = real
        return torch.autograd.grad(z, params, dz)

    library()
    want = torch_way()
    torch.cuda.synchronize()
    got = [t for pair in zip(dW, db) for t in pair]
    agree = {f"{'dW' if i % 2 == 0 else 'db'}{i // 2}": float((a - t).abs().max() / t.abs().max().clamp_min(1e-30))
             for i, (a, t) in enumerate(zip(got, want))}
    res = _interleaved({"library": library, "torch": torch_way})
    torch.cuda.synchronize()
    try:
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            library()
        res.update(_interleaved({"library_graph_replay": gr.replay}))
    except Exception as e:  # measured, not gated
        res["library_graph_replay"] = {"not_measured": f"{type(e).__name__}: {str(e)[:200]}"}
    res["library_over_torch"] = round(res["library"]["median_us"] / res["torch"]["median_us"], 3)
    res["max_rel_difference_to_torch"] = {k: float(f"{v:.2e}") for k, v in agree.items()}
    res["workspace_bytes"] = {"acts": ab, "fwd_ws": fb, "bwd_ws": bb}
    try:
        res["device_activities_per_pair"] = {"library": _activities(library), "torch": _activities(torch_way)}
    except Exception as e:
        res["device_activities_per_pair"] = {"not_measured": f"{type(e).__name__}: {str(e)[:200]}"}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_grad_latency.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU: there is nothing to report without one"
    out = {"device": torch.cuda.get_device_name(0), "n": N, "C": C, "cin": CIN, "rounds": ROUNDS, "gated": False,
           "per_round": f"{CALLS} back-to-back forward + backward pairs between two device events after {WARM} warm-ups, per pair"}
    try:
        out["pair"] = measure()
    except Exception as e:
        out["pair"] = {"not_measured": f"{type(e).__name__}: {str(e)[:300]}"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
