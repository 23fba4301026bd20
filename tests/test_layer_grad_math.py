"""CPU: the closed-form backward of the trainable layer (include/tdmpc2_plan.h, tests/layer_grad_common.closed_form).
In fp64 it equals torch's fp64 autograd of tdmpc2_amd.layers.NormedLinear / mlp / QEnsemble.apply_params within 1e-12 of each
tensor's max; in fp32 with the library's k-ordered fmaf chains as contractions (what the MFMA computes) its error against fp64 stays within 2.5 x that of
torch's own fp32 autograd on the cases of the GPU test's measured gate."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tdmpc2_amd import layers
from tests import layer_grad_common as lg

TOL64 = 1e-12


def _close(got, ref, what):
    assert lg.rel_err(np.asarray(got, np.float64), np.asarray(ref, np.float64)) <= TOL64, what


@pytest.mark.parametrize("mask", (False, True))
@pytest.mark.parametrize("kind", (lg.LINEAR, lg.MISH, lg.SIMNORM))
def test_closed_form_equals_fp64_autograd_of_the_modules(kind, mask):
    """One layer: nn.Linear / NormedLinear (Mish, SimNorm), the mask applied where nn.Dropout applies it."""
    shape = (1, False, 33, 31, 40)
    c = lg.make_case(kind, shape, "trained", mask)
    ref = lg.closed_form(c)
    G, _, R, K, N = shape
    if kind == lg.LINEAR:
        m = torch.nn.Linear(K, N)
    else:
        m = layers.NormedLinear(K, N, act=layers.SimNorm(8) if kind == lg.SIMNORM else None)
    m = m.double()
    with torch.no_grad():
        m.weight.copy_(torch.tensor(c["w"][0]))
        m.bias.copy_(torch.tensor(c["b"][0]))
        if kind != lg.LINEAR:
            m.ln.weight.copy_(torch.tensor(c["ln_w"][0]))
            m.ln.bias.copy_(torch.tensor(c["ln_b"][0]))
    x = torch.tensor(c["x"][0], dtype=torch.float64, requires_grad=True)
    if mask:  # NormedLinear.forward with its dropout replaced by the case's multipliers
        h = F.linear(x, m.weight, m.bias) * torch.tensor(c["mask"][0], dtype=torch.float64)
        y = h if kind == lg.LINEAR else m.act(m.ln(h))
    else:
        y = m(x)
    y.backward(torch.tensor(c["dy"][0], dtype=torch.float64))
    _close(y.detach().numpy(), ref["y"][0], "y")
    _close(x.grad.numpy(), ref["dx"][0], "dx")
    _close(m.weight.grad.numpy(), ref["dw"][0], "dw")
    _close(m.bias.grad.numpy(), ref["db"][0], "db")
    if kind != lg.LINEAR:
        _close(m.ln.weight.grad.numpy(), ref["dln_w"][0], "dln_w")
        _close(m.ln.bias.grad.numpy(), ref["dln_b"][0], "dln_b")
    # the functional restatement the fp32 yardstick uses is the same function
    t64 = lg.torch_grads(c, torch.float64)
    for k in t64:
        _close(t64[k], ref[k], k)


def _chain(cases, x, dy_last):
    """Layers applied one after another with the closed form: forward through all, then backward from dy_last."""
    outs, h = [], x
    for c in cases:
        c["x"] = h
        c["dy"] = np.zeros((c["G"], c["R"], c["N"]))
        f = lg.closed_form(c)
        outs.append(f)
        h = f["y"]
    dy = dy_last
    grads = []
    for c in reversed(cases):
        c["dy"] = dy
        g = lg.closed_form(c)
        grads.append(g)
        dy = g["dx"]
    return outs[-1]["y"], list(reversed(grads))


def test_closed_form_equals_fp64_autograd_of_mlp():
    """layers.mlp(): two NormedLinear (Mish) and a SimNorm NormedLinear, chained."""
    torch.manual_seed(3)
    R, dims = 17, (11, 24, 24, 16)
    seq = layers.mlp(dims[0], [dims[1], dims[2]], dims[3], act=layers.SimNorm(8)).double()
    with torch.no_grad():
        for p in seq.parameters():
            p.copy_(torch.randn_like(p) * (0.5 if p.dim() == 2 else 1.0) + (1.0 if p.dim() == 1 else 0.0))
    rng = np.random.default_rng(5)
    x, dy = rng.standard_normal((1, R, dims[0])), rng.standard_normal((1, R, dims[3]))
    cases = []
    for i, m in enumerate(seq):
        kind = lg.SIMNORM if i == 2 else lg.MISH
        cases.append(dict(kind=kind, G=1, R=R, K=dims[i], N=dims[i + 1], shared=False, sd=8 if kind == lg.SIMNORM else 0, eps=m.ln.eps,
                          w=m.weight.detach().numpy()[None], b=m.bias.detach().numpy()[None], ln_w=m.ln.weight.detach().numpy()[None],
                          ln_b=m.ln.bias.detach().numpy()[None], mask=None))
    y, grads = _chain(cases, x, dy)
    xt = torch.tensor(x[0], requires_grad=True)
    yt = seq(xt)
    yt.backward(torch.tensor(dy[0]))
    _close(yt.detach().numpy(), y[0], "y")
    _close(xt.grad.numpy(), grads[0]["dx"][0], "dx")
    for i, m in enumerate(seq):
        _close(m.weight.grad.numpy(), grads[i]["dw"][0], f"dw{i}")
        _close(m.bias.grad.numpy(), grads[i]["db"][0], f"db{i}")
        _close(m.ln.weight.grad.numpy(), grads[i]["dln_w"][0], f"dln_w{i}")
        _close(m.ln.bias.grad.numpy(), grads[i]["dln_b"][0], f"dln_b{i}")


def test_closed_form_equals_fp64_autograd_of_the_ensemble():
    """QEnsemble.apply_params: shared_x on the first layer (dx summed over the members), stacked Mish, stacked Linear."""
    torch.manual_seed(4)
    G, R, K, M, O = 3, 13, 10, 24, 7
    p = layers.StackedMLPParams(G, K, M, O).double()
    with torch.no_grad():
        for t in p.parameters():
            t.copy_(torch.randn_like(t) * (0.5 if t.dim() == 3 else 1.0) + (1.0 if t.dim() == 2 else 0.0))
    rng = np.random.default_rng(6)
    x, dy = rng.standard_normal((R, K)), rng.standard_normal((G, R, O))
    dims = (K, M, M, O)
    cases = []
    for i in range(3):
        l = p.layer(i)
        ln = i < 2
        cases.append(dict(kind=lg.MISH if ln else lg.LINEAR, G=G, R=R, K=dims[i], N=dims[i + 1], shared=i == 0, sd=0, eps=1e-5,
                          w=l.weight.detach().numpy(), b=l.bias.detach().numpy(), ln_w=l.ln.weight.detach().numpy() if ln else None,
                          ln_b=l.ln.bias.detach().numpy() if ln else None, mask=None))
    y, grads = _chain(cases, x, dy)
    xt = torch.tensor(x, requires_grad=True)
    yt = layers.QEnsemble.apply_params(p, xt)
    yt.backward(torch.tensor(dy))
    _close(yt.detach().numpy(), y, "y")
    _close(xt.grad.numpy(), grads[0]["dx"], "dx")
    for i in range(3):
        l = p.layer(i)
        _close(l.weight.grad.numpy(), grads[i]["dw"], f"dw{i}")
        _close(l.bias.grad.numpy(), grads[i]["db"], f"db{i}")
        if i < 2:
            _close(l.ln.weight.grad.numpy(), grads[i]["dln_w"], f"dln_w{i}")
            _close(l.ln.bias.grad.numpy(), grads[i]["dln_b"], f"dln_b{i}")


@pytest.mark.parametrize("key", lg.measured_cases(), ids=lg.case_id)
def test_fp32_chain_emulation_stays_within_torch_fp32(key):
    """The closed form in fp32 with the library's k-ordered fmaf chains in its contractions: e(T) <= 2.5 x torch's CPU fp32 autograd, for every
    output tensor of every case of the GPU test's measured gate (which allows the library 4 x: the headroom stays visible)."""
    c, ref, e_torch = lg.measured_reference(*key)
    emu = lg.closed_form(c, np.float32, lg.chain_gemm)
    # torch's error is floored at 2^-23 of the tensor's max, as in the GPU gate: below one fp32 ulp of the largest element a tensor's
    # worst error is a single rounding either way, and the ratio of two such numbers measures luck, not arithmetic
    ratios = {k: lg.rel_err(emu[k], ref[k]) / max(e_torch[k], 2.0 ** -23) for k in e_torch}
    print(lg.case_id(key), {k: round(v, 2) for k, v in ratios.items()})
    for k, r in ratios.items():
        assert r <= 2.5, (k, r, e_torch[k])
