"""Generator of tests/golden/model_<case>.npz: the forward half of TDMPC2._update (tdmpc2/tdmpc2.py:259-304) through the
reference's OWN modules -- WorldModel.next / reward / Q(return_type='all') / termination and common.math.soft_ce, called verbatim
on the CPU in eval mode under no_grad, on the synthetic weights of oracle.cases.  Only the short loop and the loss assembly of
tdmpc2.py:268-304 are restated here (line numbers in the comments).  Every case runs twice: in fp32, and through the same modules
in fp64 (agent.model.double(), inputs cast up); the fp64 run is stored as ONE number per field, <field>_d64 = max |fp32 - fp64|.

Per case: a full entry at B = 12 ("b12.<field>": zs, every logit, reward, q, term_logit, losses, step_means) and an entry at
B = 130 ("b130.<field>": reward, q, term_logit, losses, step_means only).  c4 (widths of 4096) is stored at B = 8 only -- its
B = 130 run takes minutes on a CPU and adds no new code path.  Inputs are rebuilt from seeds (tests/model_common.py: inputs),
never stored, except td_target ("<entry>.td" [H, B]): the reference's own _td_target output for the batch.  tiny, c2 and tiny_mt also store the reference's encode output
of seeded observations ("obs.z", [H+1, 12, L]) and the losses of the batch built on them ("obs.losses", "obs.td").  tiny_mt, c1_ep
(fused family) and c3 (layered) also store the TARGET ensemble's heads on the same rollout ("tq.q_logits", "tq.q": Q(..., target=True)).

    python tools/make_model_golden.py [case ...]
"""
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import model_common as mc  # noqa: E402


def forward(agent, cfg, z0, actions, next_z, reward, td, terminated, task, dtype):
    """tdmpc2.py:268-304 with the reference's modules; returns the fields of mc.FULL as numpy arrays."""
    from common import math as rmath  # the reference's own module (on sys.path after ref_runner's import)
    import torch.nn.functional as F

    t_ = lambda x: torch.as_tensor(x).to(dtype)
    z0, actions, next_z, reward, td, terminated = map(t_, (z0, actions, next_z, reward, td, terminated))
    task_t = None if task is None else torch.as_tensor(task)
    m = agent.model
    H = actions.shape[0]
    with torch.no_grad():
        zs = [z0]
        step = torch.zeros(4, H, dtype=dtype)
        for t in range(H):                                              # :272-276
            zs.append(m.next(zs[-1], actions[t], task_t))
            step[0, t] = F.mse_loss(zs[-1], next_z[t])
        zs = torch.stack(zs)
        _zs = zs[:-1]                                                   # :279
        qs = m.Q(_zs, actions, task_t, return_type='all')               # :280
        rew = m.reward(_zs, actions, task_t)                            # :281
        term = m.termination(zs, task_t, unnormalized=True) if cfg.episodic else None   # :282-283 (all of zs; the loss uses [1:])
        for t in range(H):                                              # :287-291
            step[1, t] = rmath.soft_ce(rew[t], reward[t], cfg).mean()
            step[2, t] = sum(rmath.soft_ce(qs[i, t], td[t], cfg).mean() for i in range(cfg.num_q)) / cfg.num_q
            if cfg.episodic:
                step[3, t] = F.binary_cross_entropy_with_logits(term[t + 1], terminated[t])
        w = torch.tensor([cfg.rho ** t for t in range(H)], dtype=dtype)
        cons = (step[0] * w).sum() / H                                  # :293
        rl = (step[1] * w).sum() / H                                    # :294
        vl = (step[2] * w).sum() / H                                    # :299 (/ num_q is inside step[2])
        tl = F.binary_cross_entropy_with_logits(term[1:], terminated) if cfg.episodic else torch.zeros((), dtype=dtype)   # :295-298
        total = cfg.consistency_coef * cons + cfg.reward_coef * rl + cfg.termination_coef * tl + cfg.value_coef * vl  # :300-305
        out = {"zs": zs, "reward_logits": rew, "reward": rmath.two_hot_inv(rew, cfg), "q_logits": qs,
               "q": rmath.two_hot_inv(qs, cfg), "losses": torch.stack([cons, rl, vl, tl, total]), "step_means": step}
        if cfg.episodic:
            out["term_logit"] = term
    return {k: v.numpy() for k, v in out.items()}


def run_entry(c, B, fields, obs=False):
    from oracle import ref_runner

    cfg = c["cfg"]
    sd = {k: torch.as_tensor(v) for k, v in c["sd"].items()}
    if cfg.multitask:
        from tdmpc2_amd.config import get_discount
        disc = torch.tensor([get_discount(cfg, L) for L in cfg.episode_lengths])
    else:
        disc = c["discounts"][0]
    inp = mc.inputs(cfg, B)
    res = {}
    agent = ref_runner.build_agent(cfg, sd, disc)
    z0, next_z = inp["z0"], inp["next_z"]
    if obs:
        with torch.no_grad():
            o = torch.as_tensor(mc.obs_inputs(cfg, B))
            tk = None if inp["tasks"] is None else torch.as_tensor(inp["tasks"])
            z_all = torch.stack([agent.model.encode(o[i], tk) for i in range(o.shape[0])]).numpy()
        z0, next_z = z_all[0], z_all[1:]
        res["z"] = z_all
    td = ref_runner.run_reference_td_target(cfg, sd, next_z=next_z, reward=inp["reward"], terminated=inp["terminated"],
                                            task=inp["tasks"], discount=disc, pi_eps=inp["pi_eps"], qidx=inp["qidx"]).numpy()
    res["td"] = td.reshape(td.shape[0], td.shape[1])
    args = (z0, inp["actions"], next_z, inp["reward"], td, inp["terminated"], inp["tasks"])
    f32 = forward(agent, cfg, *args, torch.float32)
    agent.model.double()
    f64 = forward(agent, cfg, *args, torch.float64)
    for k in fields:
        if k not in f32:
            continue
        res[k] = np.ascontiguousarray(f32[k])
        res[k + "_d64"] = np.float64(np.abs(f32[k].astype(np.float64) - f64[k]).max())
    return res


def target_q(agent, cfg, z0, actions, task, dtype):
    """Q(zs[:-1], actions, return_type='all', target=True) on the rollout's latents (world_model.py:186-210 with the target heads)."""
    from common import math as rmath

    z0, actions = torch.as_tensor(z0).to(dtype), torch.as_tensor(actions).to(dtype)
    task_t = None if task is None else torch.as_tensor(task)
    with torch.no_grad():
        zs = [z0]
        for t in range(actions.shape[0] - 1):
            zs.append(agent.model.next(zs[-1], actions[t], task_t))
        qs = agent.model.Q(torch.stack(zs), actions, task_t, return_type='all', target=True)
        return {"q_logits": qs.numpy(), "q": rmath.two_hot_inv(qs, cfg).numpy()}


def run_target_entry(c, B):
    from oracle import ref_runner

    cfg = c["cfg"]
    sd = {k: torch.as_tensor(v) for k, v in c["sd"].items()}
    agent = ref_runner.build_agent(cfg, sd, c["discounts"][0])   # (the discount plays no part in Q)
    inp = mc.inputs(cfg, B)
    f32 = target_q(agent, cfg, inp["z0"], inp["actions"], inp["tasks"], torch.float32)
    agent.model.double()
    f64 = target_q(agent, cfg, inp["z0"], inp["actions"], inp["tasks"], torch.float64)
    res = {}
    for k in f32:
        res[k] = np.ascontiguousarray(f32[k])
        res[k + "_d64"] = np.float64(np.abs(f32[k].astype(np.float64) - f64[k]).max())
    return res


def generate(name):
    from oracle import cases

    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # one thread: the same reduction order on every machine
    try:
        return _generate(name, cases.build_case(name))
    finally:
        torch.set_num_threads(threads)  # (a test process goes on with its own setting)


def _generate(name, c):
    for k, v in (("rho", 0.5), ("consistency_coef", 20.0), ("reward_coef", 0.1), ("value_coef", 0.1), ("termination_coef", 1.0)):
        assert getattr(c["cfg"], k) == v
    b_full, b_small = mc.CASES[name]
    res = {}
    for k, v in run_entry(c, b_full, mc.FULL).items():
        res[f"b{b_full}.{k}"] = v
    if b_small:
        for k, v in run_entry(c, b_small, mc.SMALL).items():
            res[f"b{b_small}.{k}"] = v
    if name in mc.TARGET_CASES:
        for k, v in run_target_entry(c, b_full).items():
            res[f"tq.{k}"] = v
    if name in mc.OBS_CASES:
        for k, v in run_entry(c, b_full, ("losses",), obs=True).items():
            res[f"obs.{k}"] = v
    return res


def write(name):
    res = generate(name)
    buf = io.BytesIO()
    np.savez_compressed(buf, **res)
    with open(mc.path(name), "wb") as f:
        f.write(buf.getvalue())
    print(f"wrote {mc.path(name)}: {len(buf.getvalue())} bytes, {len(res)} arrays")


def main():
    from oracle import ref_runner

    if not ref_runner.available():
        raise SystemExit("the reference tree is not available: nothing to generate")
    for name in (sys.argv[1:] or list(mc.CASES)):
        write(name)


if __name__ == "__main__":
    main()
