"""Pixel encoder on training batches: the MFMA batch route (tdmpc2_plan_encode_pix_batch) against the route it replaces at batch
size (tdmpc2_plan_encode_pix at 256 images with max_envs = 256: the per-image route) and against the PyTorch-ROCm module
(layers.conv, as TDMPC2.model_losses calls it: one encode per time step), at 256 and 1 024 images (uint8, C = 32, Cin = 9), and
one model_losses call of a c1-sized rgb agent at B = 256, H = 3 with native_pixel_encoder on and off.  One process, the ways
interleaved: ROUNDS rounds, in each a CUDA-event median of 50 calls after 5 warm-ups per way; reported are the median of the
rounds' medians and their spread (max - min), the run-to-run spread a difference has to exceed.  The clocks under the batch
route's load are recorded (bench.py's sampler).  No ratio is asserted.  MI355X box:

    python tools/pixel_batch_latency.py            # writes profiles/pixel_batch_latency.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ROUNDS = 5


def _median_us(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def _interleaved(fns, reps=50):
    """{way: {median_us, spread_us, rounds_us}}: the ways take turns, round by round."""
    rounds = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            rounds[k].append(_median_us(fn, reps=reps))
    return {k: {"median_us": round(statistics.median(v), 1), "spread_us": round(max(v) - min(v), 1), "rounds_us": [round(x, 1) for x in v]}
            for k, v in rounds.items()}


def _agent(native, H=3, max_envs=1):
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.tdmpc2 import TDMPC2

    cfg = named_config("c1", horizon=H)
    cfg.obs, cfg.obs_shape = "rgb", {"rgb": (9, 64, 64)}
    torch.manual_seed(0)
    agent = TDMPC2(cfg, device=torch.device("cuda", 0), max_envs=max_envs)
    agent.native_pixel_encoder = native
    agent.planner()
    return agent


def encoder_times():
    from bench import box_under_load
    from tdmpc2_amd.native import NativePlanner

    dev = torch.device("cuda", 0)
    agent = _agent(True)
    sd = {k: v for k, v in agent.model.state_dict().items() if k.startswith("_encoder.rgb.")}
    big = NativePlanner(agent.cfg, agent.cfg.iterations, dev, max_envs=256)
    big.bind_pixel_encoder(sd)
    big.reserve_pix_batch(256)
    m = agent.model._encoder["rgb"]
    out = {}
    for n, B in ((256, 64), (1024, 256)):  # (H + 1) B frames with H = 3
        obs = torch.randint(0, 256, (n, 9, 64, 64), device=dev, dtype=torch.uint8)
        shift = NativePlanner.draw_shift(n, dev)
        z = torch.empty(n, agent.cfg.latent_dim, device=dev)
        steps = obs.reshape(n // B, B, 9, 64, 64)

        def module():  # ShiftAug's x.float() and its draw included, as in model_losses
            return torch.stack([m(steps[i]) for i in range(steps.shape[0])])

        fns = {"batch_route": lambda: big.encode_pix_batch(obs, shift, out=z), "module": module}
        if n == 256:
            fns["encode_pix_max_envs_256"] = lambda: big.encode_pix(obs, shift, out=z)
        with torch.no_grad():
            res = _interleaved(fns)
            if n == 256:
                def queue():
                    for _ in range(400):
                        fns["batch_route"]()
                res["clocks_under_load"] = box_under_load(queue, dev)
        out[f"n{n}"] = res
    return out


def model_losses_times(B=256, H=3):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    obs = torch.randint(0, 256, (H + 1, B, 9, 64, 64), generator=g, dtype=torch.uint8).to(dev)
    fns = {}
    for native in (True, False):
        agent = _agent(native, H, max_envs=2)  # (H + 1) B rows of the value kernels: 2 plans' worth of samples
        A = agent.cfg.action_dim
        act = (torch.rand(H, B, A, generator=g) * 2 - 1).to(dev)
        rew = torch.randn(H, B, 1, generator=g).to(dev)
        fns["native_pixel_encoder" if native else "module"] = (lambda ag, a, r: lambda: ag.model_losses(obs, a, r))(agent, act, rew)
    return dict(_interleaved(fns, reps=20), B=B, H=H)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_batch_latency.json"))
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "per_round": "median of 50 event timings after 5 warm-ups (model_losses: 20)",
           "encoder": encoder_times(), "model_losses": model_losses_times()}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
