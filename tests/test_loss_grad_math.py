"""CPU: the closed form of the loss seeds (include/tdmpc2_plan.h: tdmpc2_loss_*; tests/loss_grad_common.py) against the fixture
that the reference's own soft_ce / two_hot produced under torch autograd (tools/make_loss_golden.py), and its fp32 restatement
against torch's own fp32 autograd of the same expression.

Gates.  fp64 closed form against the fixture's fp64: 1e-12 of each tensor's largest magnitude (two fp64 evaluations of one formula).
fp32 restatement: e <= MARGIN * max(e_torch32, FLOOR) per tensor, e = max |T - T64| / max |T64| (tests/optim_common.py).  The
logit seeds' error (about 8e-6 at 101 bins) is the fp32 rounding of `off` at u near 100, which torch has too."""
import numpy as np
import pytest

from tests import loss_grad_common as lc

TENSORS = ("losses", "step_means") + lc.SEEDS


@pytest.fixture(scope="module")
def fixture():
    z = np.load(lc.GOLDEN)
    h = dict(zip(lc.HYPER_KEYS, (float(v) for v in z["hyper"])))
    x = {k: z[k] for k in lc.INPUTS}
    return z, h, x


def test_fixture_is_what_the_issue_asks_for(fixture):
    z, h, x = fixture
    c = lc.FIXTURE_CASE
    assert x["q_logits"].shape == (c["Q"], c["T"], c["B"], c["NB"]) == (3, 2, 9, 101) and x["z_pred"].shape == (2, 9, 16)
    assert h == lc.hyper(c["NB"])
    assert not any(np.isnan(v).any() for v in x.values())
    edges = lc.target_edges(h, c["NB"])
    for k in ("reward", "td_target"):
        assert set(edges.tolist()) <= set(x[k].reshape(-1).tolist()), k
    for k, v in lc.make_inputs(c, seed=77).items():
        assert np.array_equal(v, x[k]), k


def test_fp64_closed_form_equals_the_fixture(fixture):
    z, h, x = fixture
    got = lc.closed_form(x, lc.FIXTURE_CASE, h, np.float64)
    for k in TENSORS:
        e = lc.rel_err(got[k], z[k + "_64"])
        print(f"{k}: {e:.3e}")
        assert e <= 1e-12, (k, e)


def test_torch_restatement_equals_the_fixture(fixture):
    """The expression written out in loss_grad_common.torch_total is the one the reference's math computes."""
    import torch

    z, h, x = fixture
    got = lc.torch_ref(x, lc.FIXTURE_CASE, h, torch.float64)
    for k in TENSORS:
        assert lc.rel_err(got[k], z[k + "_64"]) <= 1e-12, k


def test_fp32_restatement_within_the_measured_gate_on_the_fixture(fixture):
    z, h, x = fixture
    got = lc.closed_form(x, lc.FIXTURE_CASE, h, np.float32)
    for k in TENSORS:
        e, bound = lc.gate(got[k], z[k + "_64"], z[k + "_32"])
        print(f"{k}: e {e:.3e} bound {bound:.3e}")
        assert got[k].dtype == np.float32 and e <= bound, (k, e, bound)


@pytest.mark.parametrize("name", [c["name"] for c in lc.CASE_LIST])
def test_fp32_restatement_within_the_measured_gate_on_the_case_table(name):
    import torch

    case = lc.CASES[name]
    h = lc.hyper(case["NB"])
    x = lc.make_inputs(case)
    ref = lc.closed_form(x, case, h, np.float64)
    t64 = lc.torch_ref(x, case, h, torch.float64)
    yard = lc.torch_ref(x, case, h, torch.float32)
    got = lc.closed_form(x, case, h, np.float32)
    for k in TENSORS:
        if k not in ref:
            continue
        assert lc.rel_err(ref[k], t64[k]) <= 1e-12, k  # the closed form IS the autograd of the expression
        e, bound = lc.gate(got[k], ref[k], yard[k])
        print(f"{name} {k}: e {e:.3e} bound {bound:.3e}")
        assert e <= bound, (name, k, e, bound)


def test_grad_total_scales_and_zero_coefficients():
    case = lc.CASES["flag"]
    h = lc.hyper(case["NB"])
    x = lc.make_inputs(case)
    one, two = lc.closed_form(x, case, h, np.float32), lc.closed_form(x, case, h, np.float32, g=2.0)
    for k in lc.SEEDS:
        assert np.array_equal(two[k], np.float32(2) * one[k]), k
    h0 = dict(h, reward_coef=0.0)
    z = lc.closed_form(x, case, h0, np.float32)
    assert not z["d_reward_logits"].any() and np.array_equal(z["d_q_logits"], one["d_q_logits"])


def test_nan_target_poisons_its_row_only():
    case = lc.CASES["mid"]
    h = lc.hyper(case["NB"])
    x = lc.make_inputs(case)
    clean = lc.closed_form(x, case, h, np.float32)
    x2 = {k: v.copy() for k, v in x.items()}
    x2["reward"][1, 7] = np.nan
    bad = lc.closed_form(x2, case, h, np.float32)
    assert np.isnan(bad["d_reward_logits"][1, 7]).all()
    keep = np.ones(x["reward"].shape, bool)
    keep[1, 7] = False
    assert np.array_equal(bad["d_reward_logits"][keep], clean["d_reward_logits"][keep])
    assert np.isnan(bad["losses"][[1, 4]]).all() and np.array_equal(bad["losses"][[0, 2, 3]], clean["losses"][[0, 2, 3]])
    for k in ("d_z_pred", "d_q_logits", "d_term_logit"):
        assert np.array_equal(bad[k], clean[k]), k
