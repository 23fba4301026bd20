"""Policy loss seeds: the five calls of the library's policy-loss unit (tdmpc2_pigrad_head_forward / value_forward / loss_forward /
loss_backward / head_backward) against torch autograd of the same expression (world_model._pi_tail, two_hot_inv, the loss line of
tdmpc2/tdmpc2.py:226) on the same GPU, at the 5M model's shape for dog-run: T = 4, B = 256, A = 38, 101 bins.  Interleaved in one
process: the five library calls on preallocated outputs and torch, eager and replayed from a hipGraph; then `TDMPC2.update_pi` end
to end against the same steps with the tail forced through torch (the layers, the running scale and the optimiser step stay in the
library on both sides).  ROUNDS rounds, in each the time of CALLS back-to-back repetitions between two device events, divided by
CALLS; reported are the median of the rounds and their spread.
`--count-launches` is a run of its own: one forward + backward of the torch tail under torch.profiler's kernel trace, its count of
device activities merged into the file the first run wrote.  Measured, not gated: the script always exits 0.  MI355X box:

    python tools/probes/pi_grad_latency.py                    # writes profiles/pi_grad_latency.json
    python tools/probes/pi_grad_latency.py --count-launches   # adds torch's device-activity count to it
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
CASE = dict(name="5M", T=4, B=256, A=38, NB=101, live=None)
SCALE = 4.0


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


def _torch_tail(cfg, h, y, eps, ql, scale, rho, lmin, ldif):
    from tdmpc2_amd import world_model as wm

    action, info = wm._pi_tail(y, eps, None, None, lmin, ldif)
    q = wm.two_hot_inv(ql, cfg).sum(0) / 2
    loss = (-(h["entropy_coef"] * info["scaled_entropy"] + q / scale).mean(dim=(1, 2)) * rho).mean()
    return loss, action


def ways():
    from tdmpc2_amd import native
    from tdmpc2_amd.config import named_config
    from tests import pi_grad_common as pc

    dev = torch.device("cuda", 0)
    h = pc.hyper()
    cfg = named_config("c2")
    assert (cfg.num_bins, cfg.action_dim, cfg.horizon + 1) == (CASE["NB"], CASE["A"], CASE["T"])
    x = {k: (None if v is None else torch.tensor(v, device=dev)) for k, v in pc.make_inputs(CASE).items()}
    T, B, A, NB = CASE["T"], CASE["B"], CASE["A"], CASE["NB"]
    desc = native.pigrad_desc(T, B, A, NB, False, **h)
    new = lambda *s: torch.empty(s, device=dev)  # noqa: E731
    o = dict(action=new(T, B, A), entropy=new(T, B), se=new(T, B), q=new(T, B), losses=new(3), d_se=new(T, B), d_q=new(2, T, B, NB),
             d_y=new(T, B, 2 * A))
    scale, one = torch.full((1,), SCALE, device=dev), torch.ones(1, device=dev)

    def library():
        native.pigrad_head_forward(desc, x["pi_out"], x["eps"], None, o["action"], o["entropy"], o["se"])
        native.pigrad_value_forward(desc, x["q_logits"], o["q"])
        native.pigrad_loss_forward(desc, o["q"], o["entropy"], o["se"], scale, o["losses"])
        native.pigrad_loss_backward(desc, x["q_logits"], scale, one, o["d_q"], o["d_se"])
        native.pigrad_head_backward(desc, x["pi_out"], x["eps"], None, x["d_action"], o["d_se"], o["d_y"])

    y, ql = x["pi_out"].clone().requires_grad_(True), x["q_logits"].clone().requires_grad_(True)
    rho = torch.tensor([h["rho"] ** i for i in range(T)], device=dev)
    lmin, ldif = torch.tensor(h["log_std_min"], device=dev), torch.tensor(h["log_std_dif"], device=dev)

    def torch_way():
        y.grad = ql.grad = None
        loss, action = _torch_tail(cfg, h, y, x["eps"], ql, scale, rho, lmin, ldif)
        torch.autograd.backward([loss, action], [None, x["d_action"]])

    return library, torch_way


def update_pi_ways():
    """TDMPC2.update_pi on the 5M dog-run model, and the same steps with everything between the layers in torch."""
    from tdmpc2_amd import TDMPC2
    from tdmpc2_amd import world_model as wm
    from tdmpc2_amd.config import named_config

    dev = torch.device("cuda", 0)
    cfg = named_config("c2", dropout=0.0)
    torch.manual_seed(5)
    agent = TDMPC2(cfg, device=dev)
    with torch.no_grad():
        for n, p in agent.model.named_parameters():
            p.add_(torch.randn_like(p) * 0.02)
    agent.native_autograd = True
    agent.native_refresh = True
    agent.planner()
    T, B = CASE["T"], CASE["B"]
    zs = torch.rand(T, B, cfg.latent_dim, device=dev)
    eps = torch.randn(T, B, cfg.action_dim, device=dev)
    qidx = torch.tensor([1, 3], device=dev)
    rho = torch.tensor([cfg.rho ** i for i in range(T)], device=dev)
    m = agent.model

    def library():
        agent.update_pi(zs, None, pi_eps=eps, qidx=qidx)

    def torch_tail():
        agent.pi_optim  # noqa: B018
        out = m._mlp(m._pi, zs)
        action, info = wm._pi_tail(out, eps, None, None, m.log_std_min, m.log_std_dif)
        q = wm.two_hot_inv(m.Q_pair(zs, action, None, qidx), cfg).sum(0) / 2
        agent.scale.update(q[0])
        loss = (-(cfg.entropy_coef * info["scaled_entropy"] + q / agent.scale.value).mean(dim=(1, 2)) * rho).mean()
        loss.backward()
        agent.optimizer_step("pi")

    return library, torch_tail


def measure():
    library, torch_way = ways()
    res = _interleaved({"library": library, "torch": torch_way})
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
    res["library_launches"] = 5
    res["torch_over_library"] = round(res["torch"]["median_us"] / res["library"]["median_us"], 2)
    lib_pi, torch_pi = update_pi_ways()
    res["update_pi"] = _interleaved({"library_tail": lib_pi, "torch_tail": torch_pi})
    res["update_pi"]["torch_tail_over_library_tail"] = round(res["update_pi"]["torch_tail"]["median_us"] /
                                                             res["update_pi"]["library_tail"]["median_us"], 3)
    return res


def count_launches():
    from torch.profiler import ProfilerActivity, profile

    _, torch_way = ways()
    for _ in range(3):
        torch_way()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        torch_way()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pi_grad_latency.json"))
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
        out = {"device": torch.cuda.get_device_name(0), "shape": {k: CASE[k] for k in ("T", "B", "A", "NB")}, "rounds": ROUNDS,
               "per_round": f"{CALLS} back-to-back repetitions between two device events after {WARM} warm-ups, per repetition",
               "baseline": "torch autograd of the same expression on the same tensors", "gated": False}
        out.update(measure())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
