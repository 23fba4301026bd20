"""Latency of the forward half of TDMPC2._update after encode / _td_target (tdmpc2/tdmpc2.py:268-304: latent rollout, predictions,
losses): tdmpc2_plan_model_losses against the same forward through the PyTorch-ROCm modules of tdmpc2_amd/world_model.py in eager
mode under no_grad -- which is how these numbers were computed before the library had the entry point.  Legs: c2 at B = 256,
H = 3; c3 at B = 256, H = 3; c4 at B = 64, H = 5.  The two ways alternate inside one process, each measurement is a device-event
timing, every leg runs for at least a second per way after warm-up.  Also written: launches per call (model_route.h compiled on the host), the clocks under each leg's load (bench.py's sampler), MACs and
bytes per call from the shapes, and the achieved rate of the WHOLE call (not a kernel's share of peak).  MI355X box:

    python tools/model_latency.py            # writes profiles/model_latency.json
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

LEGS = (("c2", 256, 3), ("c3", 256, 3), ("c4", 64, 5))


def shape_costs(cfg, B, H):
    """MACs and minimum bytes of one call from the shapes: per chain two hidden layers and a head; weights read once per call."""
    L, M, A, T, nb, nq = cfg.latent_dim, cfg.mlp_dim, cfg.action_dim, cfg.task_dim, max(cfg.num_bins, 1), cfg.num_q
    k0 = L + T + A
    dyn = k0 * M + M * M + M * L
    head = k0 * M + M * M + M * nb
    term = ((L + T) * M + M * M + M) if cfg.episodic else 0
    macs = H * B * (dyn + (1 + nq) * head) + (H + 1) * B * term
    wbytes = 4 * (dyn + (1 + nq) * head + term)
    io = 4 * (B * L * (2 * H + 1) + H * B * (A + 3))   # z0, next_z, zs through HBM; actions and the scalar targets
    return macs, wbytes + io


def soft_ce(pred, target, cfg):
    """Cross entropy of logits against the soft two-hot encoding of symlog(target), as a torch user writes it (math.py:5-9, 58-71)."""
    pred = F.log_softmax(pred, dim=-1)
    x = (torch.sign(target) * torch.log(1 + target.abs())).clamp(cfg.vmin, cfg.vmax).squeeze(-1)
    bin_size = (cfg.vmax - cfg.vmin) / (cfg.num_bins - 1)
    idx = torch.floor((x - cfg.vmin) / bin_size)
    off = ((x - cfg.vmin) / bin_size - idx).unsqueeze(-1)
    idx = idx.long().unsqueeze(-1)
    two_hot = torch.zeros_like(pred).scatter(-1, idx, 1 - off).scatter(-1, (idx + 1) % cfg.num_bins, off)
    return -(two_hot * pred).sum(-1, keepdim=True)


def eager_losses(agent, z0, action, next_z, reward, td, terminated, task):
    """tdmpc2.py:268-304 on the PyTorch-ROCm modules of tdmpc2_amd/world_model.py, eval mode, no_grad."""
    cfg, m = agent.cfg, agent.model
    H = action.shape[0]
    zs = [z0]
    cons = 0
    for t in range(H):
        zs.append(m.next(zs[-1], action[t], task))
        cons = cons + F.mse_loss(zs[-1], next_z[t]) * cfg.rho ** t
    zs = torch.stack(zs)
    B = z0.shape[0]   # (this package's ensemble takes 2-D batches: the H x B rows flattened, the task of a row repeated over H)
    zf, af, tf = zs[:-1].reshape(H * B, -1), action.reshape(H * B, -1), None if task is None else task.repeat(H)
    qs = m.Q(zf, af, tf, return_type="all").reshape(cfg.num_q, H, B, -1)
    rew = m.reward(zf, af, tf).reshape(H, B, -1)
    rl = vl = 0
    for t in range(H):
        rl = rl + soft_ce(rew[t], reward[t], cfg).mean() * cfg.rho ** t
        for i in range(cfg.num_q):
            vl = vl + soft_ce(qs[i, t], td[t], cfg).mean() * cfg.rho ** t
    tl = F.binary_cross_entropy_with_logits(m._termination(zs[1:]), terminated) if cfg.episodic else 0.0
    return cfg.consistency_coef * cons / H + cfg.reward_coef * rl / H + cfg.termination_coef * tl + cfg.value_coef * vl / (H * cfg.num_q)


def launch_count(agent, B, H):
    """Kernel launches of one only-losses call: model_route.h itself, compiled on the host (tests/model_route_model.py)."""
    import tempfile

    from tests import model_route_model as mrm

    cfg, pl = agent.cfg, agent.planner()
    with tempfile.TemporaryDirectory() as tmp:
        lib = mrm.build(tmp)
        layered = pl.path == 2
        cap = -(-(max(agent.max_envs, 1) * cfg.num_samples) // 128) * 128
        r = mrm.route(lib, mrm.LAYERED if layered else mrm.FUSED, B, H, cfg.num_q, cfg.num_bins, cfg.episodic, mrm.LOSSES, cap,
                      ln_after=0)   # default handles: f16x2-split arithmetic with the NormedLinear epilogue inside the GEMM
    return r["launches"]


def _time_leg(fns, budget_s=1.0, warm=5):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    spent = {k: 0.0 for k in fns}
    t_end = time.time() + 60
    while min(spent.values()) < budget_s and time.time() < t_end:
        for k, fn in fns.items():   # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            ts[k].append(ms * 1e3)
            spent[k] += ms * 1e-3
    # (the wall-clock cap ends a leg whose ways never reach the budget: `device_s` says how much each way got)
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "n": len(v), "device_s": round(spent[k], 3),
                "budget_reached": spent[k] >= budget_s} for k, v in ts.items()}


def leg(name, B, H):
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.tdmpc2 import TDMPC2

    cfg = named_config(name, horizon=H)
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    agent = TDMPC2(cfg, device=dev, max_envs=max(1, -(-(H * B) // cfg.num_samples)))
    agent.model.eval()
    agent.planner()
    g = torch.Generator().manual_seed(1)
    z = torch.softmax(torch.randn((H + 1) * B, cfg.latent_dim // 8, 8, generator=g), -1).reshape(H + 1, B, cfg.latent_dim).to(dev)
    action = (torch.rand(H, B, cfg.action_dim, generator=g) * 2 - 1).to(dev)
    reward, td = torch.randn(H, B, 1, generator=g).to(dev), (torch.randn(H, B, 1, generator=g) * 5).to(dev)
    term = torch.zeros(H, B, 1, device=dev)
    task = (torch.arange(B) % len(cfg.tasks)).to(dev) if cfg.multitask else None
    with torch.no_grad():
        fns = {"native": lambda: agent.model_losses_latent(z[0], z[1:], action, reward, td, term, task, want=()),
               "eager": lambda: eager_losses(agent, z[0], action, z[1:], reward, td, term, task)}
        res = _time_leg(fns)
        from bench import box_under_load   # the clocks / socket power under this leg's own load, as bench.py samples them

        def queue():
            for _ in range(200):
                fns["native"]()
        res["clocks_under_load"] = box_under_load(queue, dev)
    try:
        res["native_launches"] = launch_count(agent, B, H)
    except Exception as ex:   # no host compiler on the box: the count is in DESIGN section 3.4d
        res["native_launches"] = None
        res["native_launches_error"] = repr(ex)[:120]
    macs, nbytes = shape_costs(cfg, B, H)
    res.update(case=name, B=B, H=H, macs=macs, bytes=nbytes, path=agent.planner().path,
               native_whole_call_tflops=2 * macs / (res["native"]["median_us"] * 1e-6) / 1e12,
               speedup=res["eager"]["median_us"] / res["native"]["median_us"])
    return res


def main():
    out = {"legs": [leg(*l) for l in LEGS]}
    path = os.path.join(ROOT, "profiles", "model_latency.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
