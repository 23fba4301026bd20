"""Trainable layer: forward + backward of one NormedLinear (Mish) at R = 1024, K = 518, N = 512 and of the G = 5 ensemble layer of
the same shape (shared input), through the C ABI (tdmpc2_layer_forward + tdmpc2_layer_backward, all gradients) against torch
autograd of the same layer on the same GPU (F.linear / baddbmm, F.layer_norm, F.mish, then autograd.grad with a ready-made dy).
One process, the ways interleaved: ROUNDS rounds, in each the time of CALLS back-to-back forward + backward pairs between two
device events, divided by CALLS; reported are the median of the rounds and their spread.  Also recorded: the same library pair
replayed from a hipGraph (the device side alone), the contraction FLOPs of a pair (three GEMMs of 2 R K N per group) and what
fraction of the 157 TFLOP/s fp32 matrix peak that is at the measured time.  Measured, not gated: the script always exits 0.  MI355X box:

    python tools/probes/layer_grad_latency.py        # writes profiles/layer_grad_latency.json
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

ROUNDS, CALLS, WARM = 7, 50, 10
PEAK = 157e12  # fp32-input MFMA FLOP/s of the part
R, K, N = 1024, 518, 512
SHAPES = {"layer": 1, "ensemble5": 5}


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


def one_shape(G):
    from tdmpc2_amd import native

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    shared = G > 1
    x = rnd(R, K) if shared else rnd(1, R, K)
    w, b, lw, lb, dy = rnd(G, N, K) / K ** 0.5, 0.1 * rnd(G, N), 1 + 0.1 * rnd(G, N), 0.1 * rnd(G, N), rnd(G, R, N)
    d = native.layer_desc(native.LAYER_MISH, G, R, K, N, shared)
    new = lambda t: torch.empty_like(t)  # noqa: E731
    y, pre, stat = new(dy), new(dy), torch.empty(G, R, 2, device=dev)
    dx, dw, db, dlw, dlb = new(x), new(w), new(b), new(lw), new(lb)
    ws = torch.empty(native.layer_workspace_bytes(d), dtype=torch.uint8, device=dev)

    def library():
        native.layer_forward(d, x, w, b, lw, lb, None, y, pre, stat)
        native.layer_backward(d, x, w, lw, lb, pre, stat, None, dy, dx, dw, db, dlw, dlb, ws)

    leaves = [t.clone().requires_grad_(True) for t in (x, w, b, lw, lb)]

    def torch_way():
        tx, tw, tb, tlw, tlb = leaves
        if shared:
            h = torch.baddbmm(tb.unsqueeze(1), tx.unsqueeze(0).expand(G, R, K), tw.transpose(1, 2))
            h = F.layer_norm(h, (N,), None, None, 1e-5) * tlw.unsqueeze(1) + tlb.unsqueeze(1)
        else:
            h = F.layer_norm(F.linear(tx[0], tw[0], tb[0]), (N,), tlw[0], tlb[0], 1e-5).unsqueeze(0)
        return torch.autograd.grad(F.mish(h), leaves, dy)

    # same values both ways, at the size timed
    library()
    want = torch_way()
    torch.cuda.synchronize()
    agree = {n: float((a - t).abs().max() / t.abs().max()) for n, a, t in zip(("dx", "dw", "db", "dln_w", "dln_b"), (dx, dw, db, dlw, dlb), want)}
    assert max(agree.values()) < 1e-4, agree

    res = _interleaved({"library": library, "torch": torch_way})
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        library()
    res.update(_interleaved({"library_graph_replay": gr.replay}))
    flops = 3 * 2 * G * R * K * N
    res["contraction_flops"] = flops
    for k in ("library", "library_graph_replay", "torch"):
        res[k]["fraction_of_fp32_matrix_peak"] = round(flops / (res[k]["median_us"] * 1e-6) / PEAK, 4)
    res["torch_over_library"] = round(res["torch"]["median_us"] / res["library"]["median_us"], 2)
    res["max_rel_difference_to_torch"] = {k: float(f"{v:.2e}") for k, v in agree.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layer_grad_latency.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU: there is nothing to report without one"
    out = {"device": torch.cuda.get_device_name(0), "R": R, "K": K, "N": N, "kind": "mish", "rounds": ROUNDS,
           "per_round": f"{CALLS} back-to-back forward + backward pairs between two device events after {WARM} warm-ups, per pair",
           "fp32_matrix_peak_flops": PEAK, "gated": False, "shapes": {}}
    for name, G in SHAPES.items():
        out["shapes"][name] = one_shape(G)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
