"""Generator of tests/golden/loss_seeds.npz: the four losses of TDMPC2._update and the gradients of their total, from the
reference's OWN common.math (soft_ce, two_hot; imported at run time through oracle/ref_runner.py) under torch autograd on the CPU,
in fp64 and again in fp32.  Only the loop around it (tdmpc2/tdmpc2.py:272-304: mse per step, soft_ce per step and head, the
binary cross-entropy, the rho weights, the coefficients) is restated here, on tensors that stand for the layers' outputs.

Stored: the inputs (tests/loss_grad_common.py: make_inputs of FIXTURE_CASE: T = 2, B = 9, L = 16, 101 bins, 3 heads, episodic;
targets with 0, +-1e5, bin boundaries +-expm1(k bin_size) and 1e-30; no NaN), the eight hyperparameters as the doubles their fp32
values stand for, and per precision losses [5], step_means [4, T] and the four gradients ("<name>_64", "<name>_32").

    python tools/make_loss_golden.py
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import loss_grad_common as lc  # noqa: E402


def run(rmath, x, case, h, dtype):
    cfg = types.SimpleNamespace(num_bins=case["NB"], vmin=h["vmin"], vmax=h["vmax"], bin_size=h["bin_size"])
    T, Q = case["T"], case["Q"]
    t = {k: torch.tensor(v, dtype=dtype) for k, v in x.items()}
    leaves = ("z_pred", "reward_logits", "q_logits", "term_logit")
    for k in leaves:
        t[k].requires_grad_(True)
    col = lambda v: v.unsqueeze(-1)  # noqa: E731  (the reference's targets are [B, 1])
    cons = rew = val = 0
    steps = np.zeros((4, T))
    for s in range(T):
        w = h["rho"] ** s
        c_s = F.mse_loss(t["z_pred"][s], t["next_z"][s])
        r_s = rmath.soft_ce(t["reward_logits"][s], col(t["reward"][s]), cfg).mean()
        cons, rew = cons + c_s * w, rew + r_s * w
        v_s = 0
        for q in range(Q):
            v_q = rmath.soft_ce(t["q_logits"][q, s], col(t["td_target"][s]), cfg).mean()
            val, v_s = val + v_q * w, v_s + v_q
        steps[:, s] = (float(c_s.detach()), float(r_s.detach()), float(v_s.detach()) / Q,
                       float(F.binary_cross_entropy_with_logits(t["term_logit"][s], t["terminated"][s]).detach()))
    cons, rew, val = cons / T, rew / T, val / (T * Q)
    term = F.binary_cross_entropy_with_logits(t["term_logit"], t["terminated"])
    total = h["consistency_coef"] * cons + h["reward_coef"] * rew + h["termination_coef"] * term + h["value_coef"] * val
    total.backward()
    out = dict(losses=np.asarray([float(v.detach()) for v in (cons, rew, val, term, total)]), step_means=steps)
    for k in leaves:
        out["d_" + k] = t[k].grad.numpy().copy()
    return out


def main():
    from oracle import ref_runner

    rmath = ref_runner._import_reference().math
    case = lc.FIXTURE_CASE
    h = lc.hyper(case["NB"])
    x = lc.make_inputs(case, seed=77)
    assert not any(np.isnan(v).any() for v in x.values())
    data = {k: v for k, v in x.items()}
    data["hyper"] = np.asarray([h[k] for k in lc.HYPER_KEYS], np.float64)
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        for k, v in run(rmath, x, case, h, dtype).items():
            data[f"{k}_{tag}"] = v
    np.savez_compressed(lc.GOLDEN, **data)
    print(f"wrote {lc.GOLDEN}: {os.path.getsize(lc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
