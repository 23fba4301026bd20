"""CPU: the backward of the pixel encoder (include/tdmpc2_pixel_grad.h, tests/pixel_grad_common.py).  In fp64 the closed form equals
torch's fp64 autograd of tdmpc2_amd.layers.conv (after ShiftAug, on the table-resampled frame: pixel_common.module_tail_fp64)
within 1e-12 of each tensor's max.  In fp32 with the documented orders of dW / db (chunks of 256 rows, folds of 32) and da (chains
of 256 terms) its error against fp64 stays within 2.5 x that of torch's CPU fp32 torch.nn.grad on the same activations and masks,
floor 2^-23: at the edge shapes for every tensor, and for dW_0 / db_0 at the workload's length (n = 256, cin = 9, C = 32: 215 296
rows) on a few dozen output elements."""
import numpy as np
import pytest
import torch

from tests import pixel_common as pc
from tests import pixel_grad_common as pg

FLOOR, RATIO = 2.0 ** -23, 2.5


@pytest.mark.parametrize("C,cin", pg.EDGE_SHAPES)
def test_closed_form_equals_fp64_autograd_of_the_module(C, cin):
    case = pg.grad_case(C, cin)
    m = pc.module(case, torch.float64)
    raw = torch.stack([pc.resample64(img, dx, dy)[0] for img, (dx, dy) in zip(case["obs"], case["shifts"])])
    x, keep = raw, {}
    for i in range(1, len(m)):
        x = m[i](x)
        keep[i] = x
    (x * case["G"]).sum().backward()
    x0, acts = keep[1].detach(), [keep[i].detach() for i in (3, 5, 7)]
    got = pg.closed_form(x0, acts, x.detach(), case["G"], [w.double() for w in case["Ws"]])
    for l, i in enumerate((2, 4, 6, 8)):
        assert pg.rel_err(got["dW"][l], m[i].weight.grad) <= 1e-12, l
        if l < 3:
            assert pg.rel_err(got["db"][l], m[i].bias.grad) <= 1e-12, l
        else:
            # SimNorm is invariant under a shift of a group's logits and a channel's 16 pixels are two whole groups: db_3 is zero in
            # exact arithmetic and both sides hold rounding noise.  It is held to 1e-12 of the sum it cancels from.
            scale = float(got["dy"][3].abs().sum())
            assert float((got["db"][3] - m[i].bias.grad).abs().max()) <= 1e-12 * scale
    # the reference forward the GPU tests build on gives the same saved tensors
    rx, ra, rz = pg.saved_of(case)
    assert pg.rel_err(rx, x0) <= 1e-12 and pg.rel_err(rz, x.detach()) <= 1e-12
    assert all(pg.rel_err(a, b) <= 1e-12 for a, b in zip(ra, acts))


def test_the_preact_seed_skips_simnorm():
    case = pg.grad_case(8, 1)
    x0, acts, z = pg.saved_of(case)
    Wd = [w.double() for w in case["Ws"]]
    a = pg.closed_form(x0, acts, z, case["G"], Wd, preact=True)
    assert torch.equal(a["dy"][3], case["G"].reshape(3, 8, 4, 4))
    b = pg.closed_form(x0, acts, z, pg.seed_grad(z, case["G"], False).reshape(3, -1), Wd, preact=True)
    c = pg.closed_form(x0, acts, z, case["G"], Wd)
    assert all(torch.equal(p, q) for p, q in zip(b["dW"], c["dW"]))


@pytest.mark.parametrize("C,cin", pg.EDGE_SHAPES)
def test_fp32_order_emulation_stays_within_torch_fp32(C, cin):
    """Every stage on its own fp32 inputs (the yardstick's dy_l, so that one stage's error does not enter the next comparison):
    e(emulation) <= 2.5 max(e(torch fp32), 2^-23) against that stage in fp64."""
    case = pg.grad_case(C, cin)
    x0, acts, z = pg.saved_of(case)
    Wd = [w.double() for w in case["Ws"]]
    y32 = pg.torch32(x0, acts, z, case["G"], Wd)
    ins = [x0, *acts]
    ratios = {}
    for l in range(4):
        dy32 = y32["dy"][l]                       # fp32, shared by all three sides
        x32 = ins[l].float()
        cols = torch.nn.functional.unfold(x32.double(), pg.KERNEL[l], stride=pg.STRIDE[l])
        g64 = dy32.double().flatten(2)
        dW64 = torch.einsum("nch,nkh->ck", g64, cols).reshape(Wd[l].shape)
        db64 = g64.sum((0, 2))
        dW32 = torch.nn.grad.conv2d_weight(x32, Wd[l].shape, dy32, stride=pg.STRIDE[l])
        db32 = dy32.sum((0, 2, 3))
        dWe, dbe = pg.emulate_dw_full(x32.numpy(), dy32.numpy(), l)
        ratios[f"dW{l}"] = pg.rel_err(dWe, dW64) / max(pg.rel_err(dW32, dW64), FLOOR)
        ratios[f"db{l}"] = pg.rel_err(dbe, db64) / max(pg.rel_err(db32, db64), FLOOR)
        if l > 0:
            W32 = case["Ws"][l]
            da64 = torch.nn.functional.fold(torch.einsum("ck,nch->nkh", W32.double().reshape(C, -1), g64), pg.SIDE[l], pg.KERNEL[l],
                                            stride=pg.STRIDE[l])
            da32 = torch.nn.grad.conv2d_input(x32.shape, W32, dy32, stride=pg.STRIDE[l])
            dae = pg.emulate_da(dy32.numpy(), W32.numpy(), l)
            ratios[f"da{l - 1}"] = pg.rel_err(dae, da64) / max(pg.rel_err(da32, da64), FLOOR)
    print((C, cin), {k: round(v, 2) for k, v in ratios.items()})
    for k, r in ratios.items():
        assert r <= RATIO, (k, r)


def test_dw0_and_db0_at_the_workload_length():
    """n = 256, cin = 9, C = 32: 215 296 rows, 841 chunks, 27 groups.  48 elements of dW_0 (first and last tap and channel among
    them) and their channels' db_0 in the documented order against torch fp32 on the whole tensor."""
    n, cin, C = 256, 9, 32
    g = torch.Generator().manual_seed(3)
    x0 = (torch.randint(0, 256, (n, cin, 64, 64), generator=g).float() / 255.0 - 0.5)
    dy = torch.randn(n, C, 29, 29, generator=g) * (torch.rand(n, C, 29, 29, generator=g) < 0.5)  # a ReLU mask's share of zeros
    dy = (dy + 0.05).float() * (dy != 0)                                                          # and a mean, as a bias gradient has
    dW32 = torch.nn.grad.conv2d_weight(x0, (C, cin, 7, 7), dy, stride=2)
    db32 = dy.sum((0, 2, 3))
    dW64 = torch.nn.grad.conv2d_weight(x0.double(), (C, cin, 7, 7), dy.double(), stride=2)
    db64 = dy.double().sum((0, 2, 3))
    rng = np.random.default_rng(0)
    elems = [(0, 0, 0, 0), (C - 1, cin - 1, 6, 6), (0, cin - 1, 0, 6), (C - 1, 0, 6, 0)]
    elems += [(int(rng.integers(C)), int(rng.integers(cin)), int(rng.integers(7)), int(rng.integers(7))) for _ in range(44)]
    dWe, dbe = pg.emulate_dw(x0.numpy(), dy.numpy(), 0, elems)
    idx = tuple(np.array(elems).T)
    cos = idx[0]
    den_w, den_b = float(dW64.abs().max()), float(db64.abs().max())
    e_w = float(np.abs(dWe.astype(np.float64) - dW64.numpy()[idx]).max()) / den_w
    e_b = float(np.abs(dbe.astype(np.float64) - db64.numpy()[cos]).max()) / den_b
    t_w = float(np.abs(dW32.double().numpy()[idx] - dW64.numpy()[idx]).max()) / den_w
    t_b = float(np.abs(db32.double().numpy()[cos] - db64.numpy()[cos]).max()) / den_b
    print(f"dW0: emulation {e_w:.3e} torch32 {t_w:.3e}; db0: emulation {e_b:.3e} torch32 {t_b:.3e}")
    assert e_w <= RATIO * max(t_w, FLOOR), (e_w, t_w)
    assert e_b <= RATIO * max(t_b, FLOOR), (e_b, t_b)
