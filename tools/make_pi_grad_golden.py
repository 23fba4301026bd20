"""Generator of tests/golden/pi_grad.npz: update_pi between its layers (tdmpc2/tdmpc2.py:219-226) through the reference's OWN code on
the CPU under torch autograd -- WorldModel.pi (math.log_std / gaussian_logprob / squash and the entropy scale) and WorldModel.Q(...,
'avg', detach=True) (math.two_hot_inv of the two drawn heads), run on a small host object whose `_pi` and `_detach_Qs` hand back the
fixture's pi_out and q_logits as autograd leaves.  Only the lines tdmpc2.py:222, 225-226 (qs / scale, rho, pi_loss) are restated,
marked below.  Every case runs in fp64 and in fp32, at the scales 1.0 and 37.5, with one thread.

Per case ("single", "multi"; tests/pi_grad_common.py: FIXTURE_CASES, fixture_inputs): "<case>.<input>" the fp32 inputs and
"<case>.s<scale>.<field>.f64" / ".f32" every output of the five library calls: action, entropy, scaled_entropy, q, losses [3],
step_means [T], d_scaled_entropy, d_q_logits and d_pi_out -- the gradient of pi_out for the incoming d_action of the inputs and the
loss's own seed of scaled_entropy, as update_pi chains them.  The generator asserts the fixture's condition: every row has
|log_prob + 1e-8| >= 1.

    python tools/make_pi_grad_golden.py
"""
import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import pi_grad_common as pc  # noqa: E402


class _Const(torch.nn.Module):
    """Stands where an MLP stands and hands back one tensor."""

    def __init__(self, value):
        super().__init__()
        self.value = value

    def forward(self, x):
        return self.value


def run(ref, case, x, h, scale, dtype):
    T, B, A, NB = case["T"], case["B"], case["A"], case["NB"]
    cfg = types.SimpleNamespace(multitask=x["mask"] is not None, num_q=2, num_bins=NB, vmin=h["vmin"], vmax=h["vmax"], rho=h["rho"],
                                entropy_coef=h["entropy_coef"], task_dim=0)
    y = torch.tensor(x["pi_out"], dtype=dtype, requires_grad=True)
    ql = torch.tensor(x["q_logits"], dtype=dtype, requires_grad=True)
    eps = torch.tensor(x["eps"], dtype=dtype)

    class Host(torch.nn.Module):
        pass

    Host.pi, Host.Q = ref.WorldModel.pi, ref.WorldModel.Q
    Host.task_emb = lambda self, z, task: z  # (the fixture starts after the embedding and the MLP)
    m = Host()
    m.cfg = cfg
    m._pi, m._detach_Qs = _Const(y), _Const(ql)
    m.log_std_min = torch.tensor(h["log_std_min"], dtype=dtype)
    m.log_std_dif = torch.tensor(h["log_std_dif"], dtype=dtype)
    task = None
    if cfg.multitask:
        live = case["live"]
        m._action_masks = torch.zeros(len(live), A, dtype=dtype)
        for i, n in enumerate(live):
            m._action_masks[i, :n] = 1.0
        task = torch.tensor([b % len(live) for b in range(B)])
    saved = (torch.randn_like, torch.randperm)
    torch.randn_like = lambda t, **kw: eps.clone()
    torch.randperm = lambda n, **kw: torch.arange(n)
    try:
        zs = torch.zeros(T, B, 1, dtype=dtype)
        action, info = m.pi(zs, task)                                                   # :219
        q = m.Q(zs, action, task, return_type="avg", detach=True)                       # :220
    finally:
        torch.randn_like, torch.randperm = saved
    lp = -info["entropy"].detach()
    assert float((lp + 1e-8).abs().min()) >= 1.0, "fixture condition: |log_prob + 1e-8| >= 1 in every row (change the inputs)"
    se = info["scaled_entropy"].detach().requires_grad_(True)
    qs = q / torch.tensor(scale, dtype=dtype)                                           # :222 (RunningScale.forward)
    rho = torch.pow(torch.tensor(cfg.rho, dtype=dtype), torch.arange(len(qs)))          # :225
    pi_loss = (-(cfg.entropy_coef * se + qs).mean(dim=(1, 2)) * rho).mean()             # :226
    pi_loss.backward()
    torch.autograd.backward([action, info["scaled_entropy"]], [torch.tensor(x["d_action"], dtype=dtype), se.grad])
    sm = (cfg.entropy_coef * se + qs).mean(dim=(1, 2))
    n = lambda v: v.detach().numpy().copy()  # noqa: E731
    return dict(action=n(action), entropy=n(info["entropy"])[..., 0], scaled_entropy=n(se)[..., 0], q=n(q)[..., 0],
                losses=np.stack([n(pi_loss), n(info["entropy"].mean()), n(se.mean())]), step_means=n(sm),
                d_scaled_entropy=n(se.grad)[..., 0], d_q_logits=n(ql.grad), d_pi_out=n(y.grad))


def generate():
    from oracle import ref_runner

    ref = ref_runner._import_reference()
    h = pc.hyper()
    res = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # one thread: the same reduction order on every machine
    try:
        for name, case in pc.FIXTURE_CASES.items():
            x = pc.fixture_inputs(name)
            for k in pc.INPUTS:
                if x[k] is not None:
                    res[f"{name}.{k}"] = x[k]
            for scale in pc.SCALES:
                for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
                    out = run(ref, case, x, h, scale, dtype)
                    for k, v in out.items():
                        res[f"{name}.s{scale}.{k}.{tag}"] = np.ascontiguousarray(v)
    finally:
        torch.set_num_threads(threads)
    return res


def main():
    from oracle import ref_runner

    if not ref_runner.available():
        raise SystemExit("the reference tree is not available: nothing to generate")
    res = generate()
    buf = io.BytesIO()
    np.savez_compressed(buf, **res)
    with open(pc.GOLDEN, "wb") as f:
        f.write(buf.getvalue())
    print(f"wrote {pc.GOLDEN}: {len(buf.getvalue())} bytes, {len(res)} arrays")


if __name__ == "__main__":
    main()
