"""CPU: the arithmetic of the optimiser step as tests/optim_common.py restates it.
  - the fp64 emulation equals clip_grad_norm_ + torch.optim.Adam in fp64 to 1e-12 relative: 3 steps, both clip regimes, two lr groups
    (torch forms its bias corrections with pow, the emulation by repeated product: a few 1e-16);
  - the fp32 emulation (= the library's arithmetic) errs against fp64 within the measured gate e <= 4 max(e_torch32, 2^-23) per
    tensor, e_torch32 = torch's own fp32 clip + Adam on the CPU, all three on the widened fp32 hyperparameters;
  - all-zero gradients leave the parameters bit-unchanged."""
import numpy as np
import pytest
import torch

from tests import optim_common as oc

COUNTS, GROUPS, LRS = [5, 64, 257, 1025], [0, 1, 0, 1], [3e-4, 9e-5]
STEPS = 3


def _data(seed=0):
    params = oc.make_values(COUNTS, seed, 1e-3, 10.0)
    grads = [oc.make_values(COUNTS, seed + 1 + s) for s in range(STEPS)]
    return params, grads


def _emulate(params0, grads, dtype, lrs, beta1, beta2, eps, max_norm):
    st = oc.new_state(COUNTS, dtype)
    ps = [p.astype(dtype) for p in params0]
    norms = []
    for gs in grads:
        norms.append(float(oc.emulate_step(st, ps, [g.astype(dtype) for g in gs], GROUPS, lrs, beta1, beta2, eps, max_norm, dtype)))
    return ps, st["m"], st["v"], norms


@pytest.mark.parametrize("regime", sorted(oc.REGIMES))
def test_fp64_emulation_equals_torch_fp64(regime):
    params0, grads = _data()
    h = oc.HYPER
    got = _emulate(params0, grads, np.float64, LRS, h["beta1"], h["beta2"], h["eps"], oc.REGIMES[regime])
    ref = oc.torch_steps(params0, grads, GROUPS, LRS, h["beta1"], h["beta2"], h["eps"], oc.REGIMES[regime], torch.float64)
    assert all((n > oc.REGIMES[regime]) == (regime == "clip") for n in ref[3])  # the regime is the one the name says
    for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), got[:3], ref[:3]):
        for x, y in zip(a, b):
            assert np.abs(x - y).max() <= 1e-12 * np.abs(y).max(), name
    assert np.allclose(got[3], ref[3], rtol=1e-12, atol=0)


@pytest.mark.parametrize("regime", sorted(oc.REGIMES))
def test_fp32_emulation_within_the_measured_gate(regime):
    params0, grads = _data(7)
    lrs = [oc.widen(v) for v in LRS]
    b1, b2, eps, mn = [oc.widen(oc.HYPER[k]) for k in ("beta1", "beta2", "eps")] + [oc.widen(oc.REGIMES[regime])]
    ref = _emulate(params0, grads, np.float64, lrs, b1, b2, eps, mn)
    got = _emulate(params0, grads, np.float32, lrs, b1, b2, eps, mn)
    t32 = oc.torch_steps(params0, grads, GROUPS, lrs, b1, b2, eps, mn, torch.float32)
    for name, a, t, r in zip(("p", "exp_avg", "exp_avg_sq"), got[:3], t32[:3], ref[:3]):
        for i, (x, y, z) in enumerate(zip(a, t, r)):
            e, et = oc.rel_err(x, z), oc.rel_err(y, z)
            print(regime, name, COUNTS[i], "e", e, "e_torch32", et, "ratio", e / max(et, oc.FLOOR))
            assert e <= oc.MARGIN * max(et, oc.FLOOR), (name, COUNTS[i], e, et)


def test_zero_gradients_leave_the_parameters_bit_unchanged():
    params0, _ = _data(3)
    st = oc.new_state(COUNTS, np.float32)
    ps = [p.copy() for p in params0]
    zeros = [np.zeros(c, np.float32) for c in COUNTS]
    norm = oc.emulate_step(st, ps, zeros, GROUPS, [oc.widen(v) for v in LRS], oc.widen(0.9), oc.widen(0.999), oc.widen(1e-8), 1.0, np.float32)
    assert norm == 0
    for p, q in zip(ps, params0):
        assert p.tobytes() == q.tobytes()
    assert all((m == 0).all() for m in st["m"]) and all((v == 0).all() for v in st["v"])
