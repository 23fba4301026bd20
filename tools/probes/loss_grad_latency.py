"""Loss seeds: forward + backward of the library's loss unit (tdmpc2_loss_forward + tdmpc2_loss_backward: three launches) against
torch autograd of the same expression (tests/loss_grad_common.py: torch_total -- log_softmax against a two-hot row per step and
head, mse, binary cross-entropy, the Python loops of tdmpc2/tdmpc2.py:272-304) on the same GPU, at the 5M model's shape: T = 3,
B = 256, L = 512, 101 bins, 5 heads.  Three ways, interleaved in one process: the two library calls on preallocated outputs,
`autograd.model_loss(...)` + `total.backward()` (the same calls under torch's autograd, with its allocations), and torch.  ROUNDS
rounds, in each the time of CALLS back-to-back repetitions between two device events, divided by CALLS; reported are the median of
the rounds and their spread, eager and (the library calls and torch) replayed from a hipGraph.
`--count-launches` is a run of its own: one torch forward + backward under torch.profiler's kernel trace, its kernel count merged
into the file the first run wrote.  Measured, not gated: the script always exits 0.  MI355X box:

    python tools/probes/loss_grad_latency.py                    # writes profiles/loss_grad_latency.json
    python tools/probes/loss_grad_latency.py --count-launches   # adds torch's launch count to it
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ROUNDS, CALLS, WARM = 7, 20, 5
CASE = dict(name="5M", T=3, B=256, L=512, NB=101, Q=5, episodic=False, scale=4.0)


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


def ways(episodic):
    from tdmpc2_amd import autograd, native
    from tdmpc2_amd.config import named_config
    from tests import loss_grad_common as lc

    dev = torch.device("cuda", 0)
    case = dict(CASE, episodic=episodic)
    h = lc.hyper(case["NB"])
    x = {k: torch.tensor(v, device=dev) for k, v in lc.make_inputs(case).items()}
    leaves = ["z_pred", "reward_logits", "q_logits"] + (["term_logit"] if episodic else [])
    for k in leaves:
        x[k].requires_grad_(True)
    args = [x.get(k) for k in lc.INPUTS]
    cfg = named_config("c1", episodic=episodic)
    assert (cfg.num_bins, cfg.latent_dim, cfg.num_q, cfg.horizon) == (case["NB"], case["L"], case["Q"], case["T"])
    desc = native.loss_desc(case["T"], case["B"], case["L"], case["Q"], case["NB"], episodic, **h)
    ws = torch.empty(native.loss_workspace_bytes(desc), dtype=torch.uint8, device=dev)
    losses, one = torch.empty(5, device=dev), torch.ones(1, device=dev)
    det = [None if t is None else t.detach() for t in args]
    outs = {"d_" + k: torch.empty_like(x[k]) for k in leaves}

    def library():
        native.loss_forward(desc, *det, losses=losses, ws=ws)
        native.loss_backward(desc, *det, grad_total=one, **outs)

    def library_autograd():
        for k in leaves:
            x[k].grad = None
        total, _ = autograd.model_loss(cfg, *args)
        total.backward()

    def torch_way():
        for k in leaves:
            x[k].grad = None
        lc.torch_total(*args, case, h)[0][4].backward()

    return library, library_autograd, torch_way


def measure(episodic):
    library, library_autograd, torch_way = ways(episodic)
    res = _interleaved({"library": library, "library_autograd": library_autograd, "torch": torch_way})
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
    res["library_launches"] = 3
    res["torch_over_library"] = round(res["torch"]["median_us"] / res["library"]["median_us"], 2)
    res["torch_over_library_autograd"] = round(res["torch"]["median_us"] / res["library_autograd"]["median_us"], 2)
    return res


def count_launches():
    from torch.profiler import ProfilerActivity, profile

    out = {}
    for episodic in (False, True):
        _, _, torch_way = ways(episodic)
        for _ in range(3):
            torch_way()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            torch_way()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        out["episodic" if episodic else "plain"] = len(kernels)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_grad_latency.json"))
    ap.add_argument("--count-launches", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU: there is nothing to report without one"
    if a.count_launches:
        out = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                out = json.load(f)
        try:
            out["torch_device_activities_of_one_forward_backward"] = count_launches()
        except Exception as e:
            out["torch_device_activities_of_one_forward_backward"] = {"not_measured": f"{type(e).__name__}: {str(e)[:200]}"}
    else:
        out = {"device": torch.cuda.get_device_name(0), "shape": {k: CASE[k] for k in ("T", "B", "L", "NB", "Q")}, "rounds": ROUNDS,
               "per_round": f"{CALLS} back-to-back forward + backward between two device events after {WARM} warm-ups, per repetition",
               "baseline": "torch autograd of the same expression (Python loops over steps and heads) on the same tensors", "gated": False,
               "plain": measure(False), "episodic": measure(True)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
