"""Latency of the forward of TDMPC2.update_pi (tdmpc2/tdmpc2.py:208-239: pi, Q 'avg', RunningScale.update, the loss):
tdmpc2_plan_policy_loss against the same forward through the PyTorch-ROCm modules of tdmpc2_amd/world_model.py in eager mode under
no_grad.  Legs: c2 (fused family) and c3 (layered family) at B = 256, H = 3.  Method of tools/model_latency.py: the two ways
alternate inside one process, every measurement is a device-event timing, every leg runs for at least a second per way after
warm-up, medians; the clocks under each leg's load are recorded (bench.py's sampler).  No ratio is asserted.  MI355X box:

    python tools/policy_loss_latency.py            # writes profiles/policy_loss_latency.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from model_latency import _time_leg  # noqa: E402

LEGS = (("c2", 256, 3), ("c3", 256, 3))


def eager_policy_loss(agent, zs, task, value):
    """tdmpc2.py:221-228 and common/scale.py:21-42 on the PyTorch-ROCm modules, eval mode, no_grad; `value` [1] is lerped in place."""
    cfg, m = agent.cfg, agent.model
    T, B = zs.shape[0], zs.shape[1]
    zf, tf = zs.reshape(T * B, -1), None if task is None else task.repeat(T)   # (this package's ensemble takes 2-D batches)
    action, info = m.pi(zf, tf)
    qs = m.Q(zf, action, tf, return_type="avg").reshape(T, B, 1)
    x = torch.sort(qs[0].flatten(), dim=0).values
    pos = torch.tensor([5.0, 95.0], device=x.device) * (B - 1) / 100
    fl = torch.floor(pos)
    ce = torch.clamp(fl + 1, max=B - 1)
    wc = pos - fl
    pct = x[fl.long()] * (1.0 - wc) + x[ce.long()] * wc
    value.lerp_(torch.clamp(pct[1] - pct[0], min=1.0), cfg.tau)
    qs = qs / value
    rho = torch.pow(cfg.rho, torch.arange(T, device=x.device))
    se = info["scaled_entropy"].reshape(T, B, 1)
    return (-(cfg.entropy_coef * se + qs).mean(dim=(1, 2)) * rho).mean()


def leg(name, B, H):
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.tdmpc2 import TDMPC2

    cfg = named_config(name, horizon=H)
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    agent = TDMPC2(cfg, device=dev, max_envs=max(1, -(-((H + 1) * B) // cfg.num_samples)))
    agent.model.eval()
    agent.planner()
    g = torch.Generator().manual_seed(1)
    zs = torch.softmax(torch.randn((H + 1) * B, cfg.latent_dim // 8, 8, generator=g), -1).reshape(H + 1, B, cfg.latent_dim).to(dev)
    task = (torch.arange(B) % len(cfg.tasks)).to(dev) if cfg.multitask else None
    value = torch.ones(1, device=dev)
    with torch.no_grad():
        fns = {"native": lambda: agent.policy_loss(zs, task), "eager": lambda: eager_policy_loss(agent, zs, task, value)}
        res = _time_leg(fns)
        from bench import box_under_load   # the clocks / socket power under this leg's own load, as bench.py samples them

        def queue():
            for _ in range(200):
                fns["native"]()
        res["clocks_under_load"] = box_under_load(queue, dev)
    res.update(case=name, B=B, H=H, path=agent.planner().path, speedup=res["eager"]["median_us"] / res["native"]["median_us"])
    return res


def main():
    out = {"legs": [leg(*l) for l in LEGS]}
    path = os.path.join(ROOT, "profiles", "policy_loss_latency.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
