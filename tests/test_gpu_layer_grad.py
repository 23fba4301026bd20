"""GPU: tdmpc2_layer_forward / tdmpc2_layer_backward against the fp64 closed form (tests/layer_grad_common.py).
  exact     Linear with small-integer operands: every sum stays below 2^24, so y, dx, dw, db equal fp64 bit for bit whatever the
            summation order -- indexing and coverage at every shape
  derived   Linear with random operands: each element within (L + 1) 2^-24 sum |a| |b| of fp64 (the a-priori bound of an fmaf
            chain of length L; partial chains only lower it), plus 2^-24 |b| for the bias
  measured  Mish / SimNorm, plain and trained-like weights: e(T) = max |T - T64| / max |T64| <= 4 max(e_torch32, 2^-23) per tensor,
            e_torch32 = torch's CPU fp32 autograd on the same inputs.  TDMPC2_LAYER_GRAD_JSON=<file> merges the worst ratio per
            tensor and case into that file (profiles/layer_grad_edges.json)
and the behaviour of the call: repeatable bit for bit, rows independent of the other rows, NULL outputs, masks, hipGraph capture,
LayerFn / mlp_apply / ensemble_apply / WorldModel.native_autograd against the torch modules' autograd."""
import json
import os

import numpy as np
import pytest
import torch

from tests import layer_grad_common as lg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MARGIN = 4.0
FLOOR = 2.0 ** -23


def _dev(v):
    return None if v is None else torch.tensor(v, dtype=torch.float32, device=DEV)


def hip_layer(c, dx=True, params=True, outs=None):
    """One forward + backward through the C ABI -> dict of numpy arrays (y, pre, stat, dx, dw, db, dln_w, dln_b as asked for).
    outs: pre-filled output tensors to use instead of fresh ones (the NULL-argument tests)."""
    from tdmpc2_amd import native

    ln = c["kind"] != lg.LINEAR
    G, R, K, N = c["G"], c["R"], c["K"], c["N"]
    d = native.layer_desc(c["kind"], G, R, K, N, c["shared"], c["sd"], c["eps"])
    t = {k: _dev(c[k]) for k in ("x", "w", "b", "dy", "mask")}
    t["ln_w"], t["ln_b"] = (_dev(c["ln_w"]), _dev(c["ln_b"])) if ln else (None, None)
    new = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)  # noqa: E731
    o = dict(outs or {})
    o.setdefault("y", new(G, R, N))
    if ln:
        o.setdefault("pre", new(G, R, N))
        o.setdefault("stat", new(G, R, 2))
    if dx:
        o.setdefault("dx", new(*t["x"].shape))
    if params:
        o.setdefault("dw", new(G, N, K))
        o.setdefault("db", new(G, N))
        if ln:
            o.setdefault("dln_w", new(G, N))
            o.setdefault("dln_b", new(G, N))
    native.layer_forward(d, t["x"], t["w"], t["b"], t["ln_w"], t["ln_b"], t["mask"], o["y"], o.get("pre"), o.get("stat"))
    ws = torch.empty(native.layer_workspace_bytes(d), dtype=torch.uint8, device=DEV)
    native.layer_backward(d, t["x"], t["w"], t["ln_w"], t["ln_b"], o.get("pre"), o.get("stat"), t["mask"], t["dy"],
                          o["dx"] if dx else None, *(o.get(k) if params else None for k in ("dw", "db", "dln_w", "dln_b")), ws)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


LINEAR_SHAPES = lg.all_shapes(lg.LINEAR)


@pytest.mark.parametrize("mask", (False, True), ids=("nomask", "mask"))
@pytest.mark.parametrize("shape", LINEAR_SHAPES, ids=lg.shape_id)
def test_exact_integer_linear(shape, mask):
    c = lg.make_case(lg.LINEAR, shape, mask=mask, integer=True)
    ref = lg.closed_form(c)
    got = hip_layer(c)
    for k in ("y", "dx", "dw", "db"):
        assert np.abs(ref[k]).max() < 2 ** 24
        assert np.array_equal(got[k].astype(np.float64), ref[k]), (k, int((got[k] != ref[k]).sum()), "elements differ")


@pytest.mark.parametrize("shape", LINEAR_SHAPES, ids=lg.shape_id)
def test_derived_bound_linear(shape):
    G, sh, R, K, N = shape
    c = lg.make_case(lg.LINEAR, shape, mask=R % 2 == 0)
    ref = lg.closed_form(c, want_abs=True)
    got = hip_layer(c)
    m = 1.0 if c["mask"] is None else c["mask"].astype(np.float64)
    # y = (chain + b) * mask: the chain's bound, one rounding of the sum with b, one of the product with the mask
    extra = 0 if c["mask"] is None else 1
    bound_y = ((K + 1) * lg.U * ref["abs_y"] + lg.U * np.abs(c["b"].astype(np.float64))[:, None, :]) * m + extra * lg.U * np.abs(ref["y"])
    # dlin = dy * mask is one rounding of its own before the chains: (L + 2) in place of (L + 1) where there is a mask
    bounds = {"y": bound_y, "dx": ((G if sh else 1) * N + 1 + extra) * lg.U * ref["abs_dx"], "dw": (R + 1 + extra) * lg.U * ref["abs_dw"]}
    for k, b in bounds.items():
        err = np.abs(got[k].astype(np.float64) - ref[k])
        worst = float((err / np.maximum(b, 1e-300)).max())
        print(k, "worst err / bound", round(worst, 3))
        assert (err <= b).all(), (k, worst)
    # db: a sum of R terms in the fixed order of the column kernel
    absdl = np.abs(c["dy"].astype(np.float64) * m).sum(1)
    assert (np.abs(got["db"].astype(np.float64) - ref["db"]) <= (R + 1 + extra) * lg.U * absdl).all()


def _merge_json(case, ratios):
    path = os.environ.get("TDMPC2_LAYER_GRAD_JSON")
    if not path:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.setdefault("gate", "e_hip <= 4 * max(e_torch32, 2^-23), e(T) = max|T - T64| / max|T64|")
    doc.setdefault("cases", {})[case] = {k: round(v, 3) for k, v in ratios.items()}
    worst = {}
    for r in doc["cases"].values():
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    doc["worst_ratio_per_tensor"] = worst
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def _gate3(got, ref, e_torch, what):
    ratios = {k: lg.rel_err(got[k], ref[k]) / max(e_torch[k], FLOOR) for k in e_torch}
    print(what, {k: round(v, 2) for k, v in ratios.items()})
    return ratios


@pytest.mark.parametrize("key", lg.measured_cases(), ids=lg.case_id)
def test_measured_against_torch_fp32(key):
    c, ref, e_torch = lg.measured_reference(*key)
    got = hip_layer(c)
    ratios = _gate3(got, ref, e_torch, lg.case_id(key))
    _merge_json(lg.case_id(key), ratios)
    # stat = (mean, rstd) is saved for backward: it is the reference's to fp32 accuracy
    assert lg.rel_err(got["stat"], ref["stat"]) < 1e-5
    for k, r in ratios.items():
        assert r <= MARGIN, (k, r, e_torch[k])
    # the rows that sit past the softplus threshold / at +-50 logits are finite and right
    assert all(np.isfinite(v).all() for v in got.values())


BEHAVIOUR = [(lg.LINEAR, (2, True, 33, 31, 33), True), (lg.MISH, (5, True, 65, 33, 40), False), (lg.SIMNORM, (2, False, 33, 70, 72), True),
             (lg.MISH, (1, False, 31, 3, 24), True)]
BEHAVIOUR_IDS = [f"{lg.KIND_NAMES[k]}-{lg.shape_id(s)}" for k, s, _ in BEHAVIOUR]


@pytest.mark.parametrize("kind,shape,mask", BEHAVIOUR, ids=BEHAVIOUR_IDS)
def test_repeatable_and_null_outputs(kind, shape, mask):
    c = lg.make_case(kind, shape, "trained", mask)
    a, b = hip_layer(c), hip_layer(c)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # NULL dx leaves the parameter gradients unchanged; NULL parameter gradients leave dx unchanged
    p_only, x_only = hip_layer(c, dx=False), hip_layer(c, params=False)
    assert "dx" not in p_only and "dw" not in x_only
    for k in a:
        if k in p_only:
            assert np.array_equal(a[k], p_only[k]), k
        if k in x_only:
            assert np.array_equal(a[k], x_only[k]), k
    # backward overwrites: outputs pre-filled with garbage come out the same
    G, sh, R, K, N = shape
    junk = {"dx": torch.full((R, K) if sh else (G, R, K), 7.0, device=DEV), "dw": torch.full((G, N, K), -3.0, device=DEV),
            "db": torch.full((G, N), 1e30, device=DEV)}
    o = hip_layer(c, outs=junk)
    for k in a:
        assert np.array_equal(a[k], o[k]), k


@pytest.mark.parametrize("kind,shape,mask", BEHAVIOUR, ids=BEHAVIOUR_IDS)
def test_rows_do_not_depend_on_the_other_rows(kind, shape, mask):
    """The case's rows tiled three times over: y and dx repeat bit for bit (the parameter gradients sum three times as much)."""
    G, sh, R, K, N = shape
    c = lg.make_case(kind, shape, "plain", mask)
    a = hip_layer(c)
    big = dict(c, R=3 * R)
    tile = lambda v, ax: None if v is None else np.concatenate([v] * 3, axis=ax)  # noqa: E731
    big["x"] = tile(c["x"], 0 if sh else 1)
    big["dy"], big["mask"] = tile(c["dy"], 1), tile(c["mask"], 1)
    b = hip_layer(big)
    assert np.array_equal(b["y"], tile(a["y"], 1))
    assert np.array_equal(b["dx"], tile(a["dx"], 0 if sh else 1))


@pytest.mark.parametrize("kind,shape,mask", BEHAVIOUR[:3], ids=BEHAVIOUR_IDS[:3])
def test_mask_of_ones_equals_no_mask(kind, shape, mask):
    c = lg.make_case(kind, shape, "plain", False)
    a = hip_layer(c)
    b = hip_layer(dict(c, mask=np.ones((c["G"], c["R"], c["N"]), np.float32)))
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_captured_forward_and_backward_replay_equal_to_eager():
    from tdmpc2_amd import native

    c = lg.make_case(lg.SIMNORM, (5, True, 33, 31, 40), "trained", True)
    eager = hip_layer(c)
    G, R, K, N = c["G"], c["R"], c["K"], c["N"]
    d = native.layer_desc(c["kind"], G, R, K, N, c["shared"], c["sd"], c["eps"])
    t = {k: _dev(c[k]) for k in ("x", "w", "b", "ln_w", "ln_b", "mask", "dy")}
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV)  # noqa: E731
    o = dict(y=z(G, R, N), pre=z(G, R, N), stat=z(G, R, 2), dx=z(R, K), dw=z(G, N, K), db=z(G, N), dln_w=z(G, N), dln_b=z(G, N))
    ws = torch.empty(native.layer_workspace_bytes(d), dtype=torch.uint8, device=DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):  # nothing allocates, nothing synchronises: the two calls capture as they are
        native.layer_forward(d, t["x"], t["w"], t["b"], t["ln_w"], t["ln_b"], t["mask"], o["y"], o["pre"], o["stat"])
        native.layer_backward(d, t["x"], t["w"], t["ln_w"], t["ln_b"], o["pre"], o["stat"], t["mask"], t["dy"], o["dx"], o["dw"], o["db"],
                              o["dln_w"], o["dln_b"], ws)
    for v in o.values():
        v.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for k, v in o.items():
        assert np.array_equal(v.cpu().numpy(), eager[k]), k
    # new inputs in the same tensors: the replay computes them
    t["x"].mul_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    again = hip_layer(dict(c, x=t["x"].cpu().numpy()))
    for k, v in o.items():
        assert np.array_equal(v.cpu().numpy(), again[k]), k


# ---------------------------------------------------------------- autograd: LayerFn, mlp_apply, ensemble_apply, WorldModel
def _grads_of(loss_fn, params, inputs):
    for p in list(params) + list(inputs):
        p.grad = None
    loss_fn().backward()
    return [p.grad.detach().cpu().numpy().copy() for p in list(inputs) + list(params)]


def _run(made, lib=False):
    return _grads_of(made[1] if lib else made[0], made[2], made[3])


def _compare_with_modules(make, names, what):
    """make(dtype, device) -> (loss_fn_torch, loss_fn_lib, params, inputs).  fp64 torch autograd on the CPU is the reference; the
    library and torch's CPU fp32 autograd are measured against it per tensor, inside the measured gate."""
    ref, t32, got = _run(make(torch.float64, "cpu")), _run(make(torch.float32, "cpu")), _run(make(torch.float32, DEV), lib=True)
    torch.cuda.synchronize()
    for n, g, t, r in zip(names, got, t32, ref):
        ratio = lg.rel_err(g, r) / max(lg.rel_err(t, r), FLOOR)
        print(what, n, round(ratio, 2))
        assert ratio <= MARGIN, (what, n, ratio)


def test_layerfn_on_a_three_layer_mlp_with_a_dropout_mask():
    from tdmpc2_amd import autograd, layers

    R, dims = 37, (19, 40, 40, 24)
    rng = np.random.default_rng(11)
    x0, dy0 = rng.standard_normal((R, dims[0])), rng.standard_normal((R, dims[3]))
    mask0 = (rng.random((R, dims[1])) >= 0.25) / 0.75
    torch.manual_seed(5)
    proto = layers.mlp(dims[0], [dims[1], dims[2]], dims[3], act=layers.SimNorm(8), dropout=0.25)
    with torch.no_grad():
        for p in proto.parameters():
            p.copy_(torch.randn_like(p) * (0.3 if p.dim() == 2 else 0.2) + (1.0 if p.dim() == 1 else 0.0))
    state = proto.state_dict()

    def make(dtype, device):
        seq = layers.mlp(dims[0], [dims[1], dims[2]], dims[3], act=layers.SimNorm(8), dropout=0.25)
        seq.load_state_dict(state)
        seq = seq.to(dtype=dtype, device=device).train()
        x = torch.tensor(x0, dtype=dtype, device=device, requires_grad=True)
        dy, mask = torch.tensor(dy0, dtype=dtype, device=device), torch.tensor(mask0, dtype=dtype, device=device)

        def torch_loss():  # NormedLinear.forward with the first layer's dropout replaced by the same mask tensor
            m0 = seq[0]
            h = m0.act(m0.ln(torch.nn.functional.linear(x, m0.weight, m0.bias) * mask))
            return (seq[2](seq[1](h)) * dy).sum()

        def lib_loss():
            h = autograd.normed_linear_apply(seq[0], x, mask=mask)
            return (autograd.mlp_apply(seq[1:], h) * dy).sum()

        return torch_loss, lib_loss, list(seq.parameters()), [x]

    _compare_with_modules(make, ["x"] + [n for n, _ in proto.named_parameters()], "mlp")


def test_mlp_apply_draws_its_dropout_mask_as_nn_dropout_does():
    from tdmpc2_amd import autograd, layers

    torch.manual_seed(2)
    seq = layers.mlp(9, [24, 24], 5, dropout=0.5).to(DEV).train()
    x = torch.randn(33, 9, device=DEV)
    torch.manual_seed(7)
    want = seq(x)
    torch.manual_seed(7)
    got = autograd.mlp_apply(seq, x)  # F.dropout(ones) consumes the generator exactly as nn.Dropout does on [33, 24]
    assert (got - want).abs().max().item() <= 1e-4 * want.abs().max().item()  # (another mask moves y by its own size)
    seq.eval()
    assert (autograd.mlp_apply(seq, x) - seq(x)).abs().max().item() <= 1e-4 * want.abs().max().item()


def test_layerfn_on_the_ensemble():
    from tdmpc2_amd import autograd, layers

    G, R, K, M, O = 5, 37, 19, 40, 11
    rng = np.random.default_rng(12)
    x0, dy0 = rng.standard_normal((R, K)), rng.standard_normal((G, R, O))
    torch.manual_seed(6)
    proto = layers.StackedMLPParams(G, K, M, O)
    with torch.no_grad():
        for p in proto.parameters():
            p.copy_(torch.randn_like(p) * (0.3 if p.dim() == 3 else 0.2) + (1.0 if p.dim() == 2 else 0.0))
    state = proto.state_dict()

    def make(dtype, device):
        p = layers.StackedMLPParams(G, K, M, O)
        p.load_state_dict(state)
        p = p.to(dtype=dtype, device=device)
        x = torch.tensor(x0, dtype=dtype, device=device, requires_grad=True)
        dy = torch.tensor(dy0, dtype=dtype, device=device)
        return (lambda: (layers.QEnsemble.apply_params(p, x) * dy).sum(), lambda: (autograd.ensemble_apply(p, x) * dy).sum(),
                list(p.parameters()), [x])

    _compare_with_modules(make, ["x"] + [n for n, _ in proto.named_parameters()], "ensemble")


def test_layerfn_passes_null_for_what_needs_no_gradient():
    """Frozen Q networks (update_pi): only dx is asked for; a first layer whose input needs no gradient: only the parameters."""
    from tdmpc2_amd import autograd, layers

    torch.manual_seed(8)
    p = layers.StackedMLPParams(3, 10, 24, 5).to(DEV)
    with torch.no_grad():
        for t in p.parameters():
            t.add_(torch.randn_like(t) * 0.2)
    x = torch.randn(17, 10, device=DEV, requires_grad=True)
    full = autograd.ensemble_apply(p, x).square().sum()
    gx, = torch.autograd.grad(full, [x])
    p.requires_grad_(False)
    gx_frozen, = torch.autograd.grad(autograd.ensemble_apply(p, x).square().sum(), [x])
    assert torch.equal(gx, gx_frozen)
    p.requires_grad_(True)
    gp = torch.autograd.grad(autograd.ensemble_apply(p, x.detach()).square().sum(), list(p.parameters()))
    gp_full = torch.autograd.grad(autograd.ensemble_apply(p, x).square().sum(), list(p.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(gp, gp_full))


@pytest.mark.parametrize("episodic", (False, True), ids=("plain", "episodic"))
def test_world_model_native_autograd_matches_the_modules(episodic):
    """A tiny WorldModel: the gradients of one scalar loss over next, reward, Q(return_type='all'), pi (and the termination head of
    an episodic model) with the flag on against fp64 autograd of the modules, per parameter, inside the measured gate; with the
    flag off no library layer call is made."""
    from tdmpc2_amd import native
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.world_model import WorldModel

    cfg = named_config("tiny", episodic=episodic)
    torch.manual_seed(9)
    proto = WorldModel(cfg)
    with torch.no_grad():  # away from the init's zero biases and unit gains
        for n, p in proto.named_parameters():
            p.add_(torch.randn_like(p) * (0.1 if n.endswith("weight") and p.dim() >= 2 else 0.2))
    rng = np.random.default_rng(13)
    B = 33
    obs0, a0 = rng.standard_normal((B, cfg.obs_shape["state"][0])), np.tanh(rng.standard_normal((B, cfg.action_dim)))
    eps0 = rng.standard_normal((B, cfg.action_dim))

    def make(dtype, device, flag=False):
        m = WorldModel(cfg)
        with torch.no_grad():
            for (_, p), (_, q) in zip(m.named_parameters(), proto.named_parameters()):
                p.copy_(q)
        m = m.to(dtype=dtype, device=device)
        m.native_autograd = flag
        obs, a = torch.tensor(obs0, dtype=dtype, device=device), torch.tensor(a0, dtype=dtype, device=device)
        eps = torch.tensor(eps0, dtype=dtype, device=device)

        def loss():
            z = m.encode(obs, None)
            zn = m.next(z, a, None)
            r = m.reward(z, a, None)
            q = m.Q(zn, a, None, return_type="all")
            randn_like = torch.randn_like
            torch.randn_like = lambda t: eps  # pi's noise: the same tensor in every run
            try:
                act, info = m.pi(zn, None)
            finally:
                torch.randn_like = randn_like
            out = zn.square().sum() + r.sin().sum() + q.cos().sum() + act.sum() + info["entropy"].sum() * 0.1
            return out + m.termination(zn, None, unnormalized=True).sum() if episodic else out

        return loss, loss, list(m.parameters()), []

    names = [n for n, _ in proto.named_parameters()]
    ref, t32 = _run(make(torch.float64, "cpu")), _run(make(torch.float32, "cpu"))
    before = native.LAYER_CALLS
    off = _run(make(torch.float32, DEV, False))
    assert native.LAYER_CALLS == before  # flag off: the modules, no library layer call
    on = _run(make(torch.float32, DEV, True))
    torch.cuda.synchronize()
    # encoder 2 + dynamics 3 + reward 3 + Q 3 + pi 3 (+ termination 3) layers, forward and backward
    assert native.LAYER_CALLS - before == 2 * (len(proto._encoder["state"]) + 3 + 3 + 3 + 3 + 3 * episodic)
    for n, g_on, g_off, t, r in zip(names, on, off, t32, ref):
        ratio = lg.rel_err(g_on, r) / max(lg.rel_err(t, r), FLOOR)
        print(n, "lib/torch32", round(ratio, 2), "flag-off", round(lg.rel_err(g_off, r) / max(lg.rel_err(t, r), FLOOR), 2))
        assert ratio <= MARGIN, (n, ratio)
