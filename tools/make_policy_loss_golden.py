"""Generator of tests/golden/policy_loss_<case>.npz: the forward of TDMPC2.update_pi (tdmpc2/tdmpc2.py:208-239) through the
reference's OWN code on the CPU -- WorldModel.pi, WorldModel.Q(return_type='avg', detach=True), RunningScale._positions /
_percentile / update (called unbound on a small host object: the class itself hard-codes cuda:0 buffers) and
math.termination_statistics.  Only the four lines tdmpc2.py:223-228 are restated (marked below).  Every case runs in fp32 and
again in fp64; the fp64 run is stored as ONE number per field, <field>_d64 = max |fp32 - fp64|.

Per case: per-row fields at B = 12 ("b12.<field>": action, q, entropy, scaled_entropy) and, at B = 12 and B = 130 and a start
scale of 1.0 and 7.5, "b<B>.s<scale>.<field>": loss [4] (pi_loss, mean entropy, mean scaled_entropy, scale after), step_means
[3, H+1], percentiles [2].  Inputs are rebuilt from seeds (tests/policy_loss_common.py: inputs), never stored.  `tiny` also carries
the table of RunningScale.update alone ("scale.<kind>.<n>" = p5, p95, value after; "scale.nan.<n>"), `c1_ep` the termination
statistics of seeded logits ("term.stats").

    python tools/make_policy_loss_golden.py [case ...]
"""
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import policy_loss_common as pc  # noqa: E402


def host_scale(cfg, s0, dtype):
    """A host object carrying the reference's unbound RunningScale methods and its two buffers on the CPU."""
    from common.scale import RunningScale  # the reference's own module (importable after ref_runner's import)

    class Host:
        pass

    for m in ("_positions", "_percentile", "update"):
        setattr(Host, m, getattr(RunningScale, m))
    h = Host()
    h.cfg = cfg
    h.value = torch.full((1,), s0, dtype=dtype)
    h._percentiles = torch.tensor([5, 95], dtype=torch.float32)
    return h


def forward(agent, cfg, inp, s0, dtype):
    zs = torch.as_tensor(inp["zs"]).to(dtype)
    task = None if inp["tasks"] is None else torch.as_tensor(inp["tasks"])
    saved = (torch.randn_like, torch.randperm)

    def randn_like(x, **kw):
        return torch.as_tensor(inp["pi_eps"]).to(x.dtype).clone()

    def randperm(n, **kw):
        first = torch.as_tensor(inp["qidx"]).long()
        return torch.cat([first, torch.tensor([i for i in range(n) if i not in first.tolist()], dtype=torch.long)])

    torch.randn_like, torch.randperm = randn_like, randperm
    try:
        with torch.no_grad():
            action, info = agent.model.pi(zs, task)                                    # :221
            q = agent.model.Q(zs, action, task, return_type='avg', detach=True)        # :222
    finally:
        torch.randn_like, torch.randperm = saved
    scale = host_scale(cfg, s0, dtype)
    pct = scale._percentile(q[0])
    scale.update(q[0])                                                                 # :223
    qs = q / scale.value                                                               # :224 (RunningScale.forward)
    rho = torch.pow(cfg.rho, torch.arange(len(qs))).to(dtype)                          # :227
    pi_loss = (-(cfg.entropy_coef * info["scaled_entropy"] + qs).mean(dim=(1, 2)) * rho).mean()   # :228
    loss = torch.stack([pi_loss, info["entropy"].mean(), info["scaled_entropy"].mean(), scale.value[0]])
    sm = torch.stack([qs.mean(dim=(1, 2)), info["scaled_entropy"].mean(dim=(1, 2)), info["entropy"].mean(dim=(1, 2))])
    out = dict(action=action, q=q, entropy=info["entropy"], scaled_entropy=info["scaled_entropy"], loss=loss, step_means=sm,
               percentiles=pct.reshape(2))
    return {k: v.numpy() for k, v in out.items()}


def scale_rows(x, cfg):
    s = host_scale(cfg, 1.0, torch.float32)
    xt = torch.as_tensor(x).reshape(-1, 1)
    pct = s._percentile(xt).reshape(2)
    s.update(xt)
    return np.array([pct[0].item(), pct[1].item(), s.value[0].item()], np.float32)


def generate(name):
    from oracle import cases

    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # one thread: the same reduction order on every machine
    try:
        return _generate(name, cases.build_case(name))
    finally:
        torch.set_num_threads(threads)


def _generate(name, c):
    from oracle import ref_runner

    cfg = c["cfg"]
    assert (cfg.rho, cfg.entropy_coef, cfg.tau) == (0.5, 1e-4, pc.TAU)
    sd = {k: torch.as_tensor(v) for k, v in c["sd"].items()}
    res = {}
    for B in (pc.B_FULL, pc.B_SMALL):
        inp = pc.inputs(cfg, B)
        for s0 in pc.SCALES0:
            agent = ref_runner.build_agent(cfg, sd, c["discounts"][0])
            f32 = forward(agent, cfg, inp, s0, torch.float32)
            agent.model.double()
            f64 = forward(agent, cfg, inp, s0, torch.float64)
            fields = pc.SCALAR_FIELDS + (pc.ROW_FIELDS if (B == pc.B_FULL and s0 == pc.SCALES0[0]) else ())
            for k in fields:
                key = f"b{B}.{k}" if k in pc.ROW_FIELDS else f"b{B}.s{s0}.{k}"
                res[key] = np.ascontiguousarray(f32[k].astype(np.float32))
                res[key + "_d64"] = np.float64(np.abs(f32[k].astype(np.float64) - f64[k]).max())
    if name == pc.SCALE_CASE:
        ref_runner.build_agent(cfg, sd, c["discounts"][0])
        for kind in pc.SCALE_KINDS:
            for n in pc.SCALE_NS:
                res[f"scale.{kind}.{n}"] = scale_rows(pc.scale_input(n, kind), cfg)
        for n in (16, 256):
            res[f"scale.nan.{n}"] = scale_rows(pc.nan_input(n), cfg)
    if name == pc.TERM_CASE:
        from common import math as rmath

        x, y = pc.term_input()
        st = rmath.termination_statistics(torch.sigmoid(torch.as_tensor(x)).unsqueeze(-1), torch.as_tensor(y).unsqueeze(-1))
        res["term.stats"] = np.array([st["termination_rate"].item(), st["termination_f1"].item()], np.float32)
    return res


def write(name):
    res = generate(name)
    buf = io.BytesIO()
    np.savez_compressed(buf, **res)
    with open(pc.path(name), "wb") as f:
        f.write(buf.getvalue())
    print(f"wrote {pc.path(name)}: {len(buf.getvalue())} bytes, {len(res)} arrays")


def main():
    from oracle import ref_runner

    if not ref_runner.available():
        raise SystemExit("the reference tree is not available: nothing to generate")
    for name in (sys.argv[1:] or list(pc.CASES)):
        write(name)


if __name__ == "__main__":
    main()
