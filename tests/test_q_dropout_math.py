"""CPU: the Q ensemble's first-layer dropout in torch (`layers.QEnsemble.apply_params(p, x, mask)`) against tests/golden/q_dropout.npz,
the reference's own members run with pinned masks (tools/make_q_dropout_golden.py): logits and every gradient in fp64 to 1e-12; with
mask=None the function is bit for bit what it was.  And the frequency check of the numpy restatement of the mask kernel
(tests/dropout_common.py) at the seeds the GPU test uses, where the kernel then only has to match the restatement."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dropout_common as dc


def _old_apply_params(p, x):
    """QEnsemble.apply_params as it was before it took a mask, line for line."""
    h = x.unsqueeze(0).expand(p.n, *x.shape)
    for i in (0, 1):
        l = p.layer(i)
        h = torch.baddbmm(l.bias.unsqueeze(1), h, l.weight.transpose(1, 2))
        h = F.layer_norm(h, (h.shape[-1],), None, None, 1e-5) * l.ln.weight.unsqueeze(1) + l.ln.bias.unsqueeze(1)
        h = F.mish(h)
    l = p.layer(2)
    return torch.baddbmm(l.bias.unsqueeze(1), h, l.weight.transpose(1, 2))


def test_the_fixture_is_what_the_generator_pins():
    g = dc.golden()
    x = dc.fixture_inputs()
    for k, v in x.items():
        assert g[k].dtype == np.float32 and g[k].tobytes() == v.tobytes(), k
    m = g["mask"]
    assert m.tobytes() == dc.fixture_masks().tobytes() and m.shape == (3, 2, 5, 16)
    keep = dc.keep_of(dc.FIX["p"])
    assert (m[dc.DROPPED_ROW] == 0).all() and (m[dc.KEPT_ROW] == keep).all() and set(np.unique(m).tolist()) == {0.0, float(keep)}
    assert 0.1 < (m == 0).mean() < 0.4  # p = 0.25 over 480 elements
    assert all(g[f"{k}.f64"].dtype == np.float64 and g[f"{k}.f32"].dtype == np.float32 for k in ("logits", "d_x", "d_w0", "d_b2"))


def test_apply_params_with_a_mask_equals_the_reference_in_fp64():
    from tdmpc2_amd import layers

    g = dc.golden()
    f = dc.FIX
    R = f["T"] * f["B"]
    params, leaves = dc.stacked_params(g, torch.float64)
    x = torch.tensor(g["x"], dtype=torch.float64).reshape(R, f["K"]).requires_grad_(True)
    mask = torch.tensor(g["mask"]).reshape(f["G"], R, f["hidden"])  # (fp32: the function widens it)
    out = layers.QEnsemble.apply_params(params, x, mask)
    assert out.shape == (f["G"], R, f["out"])
    (out * torch.tensor(g["cot"], dtype=torch.float64).reshape(out.shape)).sum().backward()
    worst = {}
    for name, got in [("logits", out), ("d_x", x.grad)] + [("d_" + k, leaves[k].grad) for k in dc.PARAMS]:
        ref = g[name + ".f64"]
        worst[name] = float(np.abs(got.detach().numpy().reshape(ref.shape) - ref).max() / max(np.abs(ref).max(), 1e-300))
    print(worst)
    assert max(worst.values()) <= 1e-12, worst
    # the all-dropped row: pre is exactly 0, so the forward is Mish(ln_b) through the rest, and no gradient reaches the Linear
    gi, ti, bi = dc.DROPPED_ROW
    r = ti * f["B"] + bi
    l0, l1, l2 = params.layer(0), params.layer(1), params.layer(2)
    h = F.mish(l0.ln.bias[gi])
    h = h @ l1.weight[gi].T + l1.bias[gi]
    h = F.mish(F.layer_norm(h, (h.shape[-1],), None, None, 1e-5) * l1.ln.weight[gi] + l1.ln.bias[gi])
    want = h @ l2.weight[gi].T + l2.bias[gi]
    assert torch.allclose(out[gi, r], want, rtol=1e-13, atol=1e-13)
    # ... and the mask is seen: without it the row is another
    assert np.abs(g["logits.f64"][gi, ti, bi] - _old_apply_params(params, x).detach().numpy()[gi, r]).max() > 1e-3


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32))
def test_apply_params_without_a_mask_is_bit_for_bit_the_old_function(dtype):
    from tdmpc2_amd import layers

    g = dc.golden()
    params, _ = dc.stacked_params(g, dtype)
    x = torch.tensor(g["x"], dtype=dtype).reshape(-1, dc.FIX["K"])
    new, old = layers.QEnsemble.apply_params(params, x), _old_apply_params(params, x)
    assert torch.equal(new, old) and torch.equal(layers.QEnsemble.apply_params(params, x, None), old)
    ones = torch.ones(dc.FIX["G"], x.shape[0], dc.FIX["hidden"])
    assert torch.equal(layers.QEnsemble.apply_params(params, x, ones), old)  # multipliers of exactly 1 change nothing


@pytest.mark.parametrize("seed", dc.FREQ_SEEDS)
def test_frequency_of_the_restatement_at_the_gpu_test_s_seeds(seed):
    n, G, p = dc.FREQ_N, dc.FREQ_G, dc.FREQ_P
    q = dc.thr_of(p) / 2.0 ** 32
    masks = [dc.mask_model(n, p, seed, call) for call in (0, 1, 2)]
    for m in masks:
        dropped = m == 0
        assert set(np.unique(m).tolist()) == {0.0, float(dc.keep_of(p))}
        assert abs(float(dropped.sum()) - n * q) <= 5.0 * np.sqrt(n * q * (1.0 - q)), dropped.sum()
        per = dropped.reshape(G, -1)
        ng = n // G
        for gi in range(G):  # the same per member
            assert abs(float(per[gi].sum()) - ng * q) <= 5.0 * np.sqrt(ng * q * (1.0 - q)), (gi, per[gi].sum())
        assert all(not np.array_equal(per[a], per[b]) for a in range(G) for b in range(a + 1, G))  # no two members' masks are equal
    assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[1], masks[2]) and not np.array_equal(masks[0], masks[2])
    # the mean of the multipliers is 1 to sampling accuracy: the mask is unbiased
    assert abs(float(masks[0].astype(np.float64).mean()) - 1.0) <= 5.0 * float(dc.keep_of(p)) * np.sqrt(q * (1.0 - q) / n) + 2.0 ** -22
