"""Optimiser step: one model step over the 5M model's parameter list (the reference's groups, tdmpc2.py:22-30) and one `_pi` step
(tdmpc2.py:31) through tdmpc2_amd.ClipAdam (three launches) against torch's clip_grad_norm_ + Adam(capturable=True) + zero_grad on
the same tensors on the same GPU.  Both ways first refill the gradients from a stored random arena with one device copy (a step
zeroes them), whose time alone is reported beside them.  One process, the ways interleaved: ROUNDS rounds, in each the time of
CALLS back-to-back steps between two device events, divided by CALLS; reported are the median of the rounds and their spread,
eager and replayed from a hipGraph.  Also recorded: the bytes a library step moves (norm pass 4 N, update pass 4 reads + 4 writes
of 4 N: 36 N) over its time, as a fraction of the 8 TB/s HBM peak (about 6.3 TB/s is achievable by a streaming kernel).
Measured, not gated: the script always exits 0.  MI355X box:

    python tools/probes/optim_latency.py        # writes profiles/optim_latency.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ROUNDS, CALLS, WARM = 7, 50, 10
HBM_PEAK = 8e12  # bytes/s


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


def one_optimiser(groups, lr, eps, max_norm):
    """groups: list of dicts (params, optional lr) over parameters on the GPU."""
    from tdmpc2_amd import ClipAdam

    lib = ClipAdam(groups, lr=lr, eps=eps, max_norm=max_norm)  # every p.grad is a view into lib.grad from here on
    params = lib.params
    ref = torch.optim.Adam([g for g in groups if g["params"]], lr=lr, eps=eps, capturable=True)
    fresh = torch.randn(lib.grad.numel(), device=lib.grad.device) * 0.01
    fresh[torch.from_numpy(_padding(lib)).to(fresh.device)] = 0  # the padding of the arena stays zero

    def refill():
        lib.grad.copy_(fresh)

    def library():
        refill()
        lib.step()

    def torch_way():
        refill()
        torch.nn.utils.clip_grad_norm_(params, max_norm)
        ref.step()
        ref.zero_grad(set_to_none=False)

    res = _interleaved({"library": library, "torch": torch_way, "refill_copy_alone": refill})
    torch.cuda.synchronize()
    graphs = {}
    for name, fn in (("library_graph_replay", library), ("torch_graph_replay", torch_way)):
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            graphs[name] = g.replay
        except Exception as e:  # measured, not gated: a way that does not capture is reported as such
            res[name] = {"capture_failed": f"{type(e).__name__}: {str(e)[:200]}"}
            torch.cuda.synchronize()
    if graphs:
        res.update(_interleaved(graphs))
    n = lib.grad.numel()
    res["elements"], res["tensors"], res["arena_floats"] = sum(p.numel() for p in params), len(params), n
    res["library_bytes_per_step"] = 36 * n
    for k in ("library", "library_graph_replay"):
        if "median_us" in res.get(k, {}):
            step_us = res[k]["median_us"] - res["refill_copy_alone"]["median_us"]
            res[k]["bytes_per_second_without_refill"] = round(36 * n / (step_us * 1e-6), 1)
            res[k]["fraction_of_hbm_peak_without_refill"] = round(36 * n / (step_us * 1e-6) / HBM_PEAK, 4)
    res["torch_over_library"] = round(res["torch"]["median_us"] / res["library"]["median_us"], 2)
    lib.close()
    return res


def _padding(lib):
    import numpy as np

    m = np.ones(lib.grad.numel(), bool)
    for p, off in zip(lib.params, lib.offsets):
        m[off:off + p.numel()] = False
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_latency.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU: there is nothing to report without one"
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.world_model import WorldModel

    cfg = named_config("c1")
    m = WorldModel(cfg).to(torch.device("cuda", 0))
    out = {"device": torch.cuda.get_device_name(0), "model": "c1 (5M)", "rounds": ROUNDS,
           "per_round": f"{CALLS} back-to-back steps between two device events after {WARM} warm-ups, per step",
           "baseline": "clip_grad_norm_ + torch.optim.Adam(capturable=True) + zero_grad(set_to_none=False) on the same tensors",
           "hbm_peak_bytes_per_second": HBM_PEAK, "gated": False}
    groups = [{"params": list(m._encoder.parameters()), "lr": cfg.lr * cfg.enc_lr_scale}, {"params": list(m._dynamics.parameters())},
              {"params": list(m._reward.parameters())}, {"params": []}, {"params": list(m._Qs.parameters())}, {"params": []}]
    out["model_step"] = one_optimiser(groups, cfg.lr, 1e-8, cfg.grad_clip_norm)
    out["pi_step"] = one_optimiser([{"params": list(m._pi.parameters())}], cfg.lr, 1e-5, cfg.grad_clip_norm)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
