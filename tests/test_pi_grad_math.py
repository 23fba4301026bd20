"""CPU: the arithmetic of the policy-loss unit against tests/golden/pi_grad.npz -- the reference's own WorldModel.pi and Q(..., 'avg',
detach=True) under torch autograd in fp64 and fp32 (tools/make_pi_grad_golden.py).  The fp64 numpy closed form of every forward value
and every seed equals the fixture's fp64 arrays to 1e-12 of each tensor's maximum; the fp32 restatement of the library's arithmetic
stays within the project's measured gate e <= 4 max(e_torch32, 2^-23)."""
import os

import numpy as np
import pytest

from tests import pi_grad_common as pc

CASES = [(name, s) for name in pc.FIXTURE_CASES for s in pc.SCALES]


@pytest.fixture(scope="module")
def golden():
    return np.load(pc.GOLDEN)


def _inputs(g, name):
    return {k: (g[f"{name}.{k}"] if f"{name}.{k}" in g.files else None) for k in pc.INPUTS}


def test_the_fixture_holds_arrays_only_and_its_inputs_are_the_generated_ones(golden):
    assert os.path.getsize(pc.GOLDEN) < 1 << 20
    for name, case in pc.FIXTURE_CASES.items():
        x, want = _inputs(golden, name), pc.fixture_inputs(name)
        for k in pc.INPUTS:
            assert (x[k] is None) == (want[k] is None), (name, k)
            if x[k] is not None:
                assert x[k].dtype == np.float32 and x[k].tobytes() == want[k].tobytes(), (name, k)
        for s in pc.SCALES:
            for k in pc.FORWARD + pc.SEEDS:
                assert golden[f"{name}.s{s}.{k}.f64"].dtype == np.float64 and golden[f"{name}.s{s}.{k}.f32"].dtype == np.float32


def test_the_fixture_carries_the_edges(golden):
    h = pc.hyper()
    for name, case in pc.FIXTURE_CASES.items():
        x = _inputs(golden, name)
        A, NB = case["A"], case["NB"]
        raw, mean = x["pi_out"][..., A:], x["pi_out"][..., :A]
        assert {0.0, 6.0, -6.0, 20.0, -20.0} <= set(raw.reshape(-1).tolist())
        assert {12.0, -12.0} <= set(mean.reshape(-1).tolist()) and {0.0, 4.0, -4.0} <= set(x["eps"].reshape(-1).tolist())
        assert np.float32(np.tanh(np.float32(12.0))) == 1.0 and 1.0 - np.tanh(np.float32(20.0)) ** 2 == 0.0
        rows = x["q_logits"].reshape(-1, NB)
        assert (rows[0] == rows[0, 0]).all() and (rows.max(-1) == 1e4).sum() >= rows.shape[0] - 1
        assert rows[1].argmax() == NB // 2 and rows[2].argmax() == NB - 1 and np.count_nonzero(rows[1]) == 1
        for s in pc.SCALES:
            ent = golden[f"{name}.s{s}.entropy.f64"]
            assert (np.abs(-ent + 1e-8) >= 1.0).all()  # the fixture's condition: entropy_scale is well conditioned in every row
            seed = golden[f"{name}.s{s}.d_q_logits.f64"].reshape(-1, NB)
            assert not seed[1].any()  # one-hot on the centre bin: x == 0 exactly, the seed exactly 0
            assert seed[0].any() and h["vmax"] == 10.0  # the all-equal row is off the x == 0 discontinuity in fp64
        if x["mask"] is not None:
            assert sorted(set(x["mask"].sum(-1).tolist())) == [1.0, 3.0, 6.0]


@pytest.mark.parametrize("name,scale", CASES)
def test_fp64_closed_form_equals_the_fixture(golden, name, scale):
    h, case = pc.hyper(), pc.FIXTURE_CASES[name]
    got = pc.closed_form(_inputs(golden, name), case, h, scale, np.float64)
    for k in pc.FORWARD + pc.SEEDS:
        e = pc.rel_err(got[k], golden[f"{name}.s{scale}.{k}.f64"])
        print(name, scale, k, e)
        assert e <= 1e-12, (k, e)


@pytest.mark.parametrize("name,scale", CASES)
def test_fp32_restatement_is_inside_the_measured_gate(golden, name, scale):
    h, case = pc.hyper(), pc.FIXTURE_CASES[name]
    got = pc.closed_form(_inputs(golden, name), case, h, scale, np.float32)
    for k in pc.FORWARD + pc.SEEDS:
        e, bound = pc.gate(got[k], golden[f"{name}.s{scale}.{k}.f64"], golden[f"{name}.s{scale}.{k}.f32"])
        print(name, scale, k, e, bound)
        assert e <= bound, (k, e, bound)


def test_grad_total_is_one_factor_and_masked_columns_are_zero(golden):
    h, case = pc.hyper(), pc.FIXTURE_CASES["multi"]
    x = _inputs(golden, "multi")
    one, two = (pc.closed_form(x, case, h, 37.5, np.float32, g=g) for g in (1.0, 2.0))
    for k in ("d_scaled_entropy", "d_q_logits"):
        assert (np.float32(2) * one[k]).tobytes() == two[k].tobytes(), k
    A = case["A"]
    dead = np.broadcast_to(x["mask"][None] == 0, one["d_pi_out"][..., :A].shape)
    assert not one["d_pi_out"][..., :A][dead].any() and not one["d_pi_out"][..., A:][dead].any()
    zero = pc.closed_form(x, case, dict(h, entropy_coef=0.0), 1.0, np.float32)
    assert not zero["d_scaled_entropy"].any()


def test_the_torch_restatement_of_the_port_agrees_with_the_reference(golden):
    """`torch_ref` (the port's _pi_tail / two_hot_inv, the yardstick of the GPU shape tests) on the fixture's inputs."""
    import torch

    h = pc.hyper()
    for name, case in pc.FIXTURE_CASES.items():
        x = _inputs(golden, name)
        threads = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            got = pc.torch_ref(x, case, h, 37.5, torch.float64)
        finally:
            torch.set_num_threads(threads)
        for k in pc.FORWARD + pc.SEEDS:
            assert pc.rel_err(got[k], golden[f"{name}.s37.5.{k}.f64"]) <= 1e-12, (name, k)
