"""-m gpu: the pixel-gradient unit (include/tdmpc2_pixel_grad.h) on the device.
1 forward identity   z is tdmpc2_plan_encode_pix_batch's bit for bit (uint8 and fp32 frames, n = 1, 2, 17); the saved activations are
                     within pixel_common's gates of the fp64 forward
2 exact probes       seed_is_preact = 1, a one-hot dz, one-hot layers with an open ReLU above the probed layer: every sum at and
                     above that layer has one non-zero term, so the fp64 closed form on the saved fp32 tensors is exact and the
                     library must equal it bit for bit: dW_l is the window of the input, db_l is 1, dy_{l-1} the weight under the mask
3 derived gate       every stage in fp64 on that stage's own fp32 inputs (read from acts / bwd_ws): |err| <= (L + 1) 2^-24 sum |a||b|
                     with L the roundings of the documented order
4 measured gate      the whole backward against the fp64 closed form and torch CPU fp32 (torch.nn.grad) on the same saved activations:
                     rel_err(lib) <= 4 max(rel_err(torch32), 2^-23) per tensor
5 the call           NULL pairs drop their launches and leave the other outputs' bits; two calls give equal bits; a captured
                     forward + backward replays the eager bits; nothing is written outside the reported sizes
TDMPC2_PIXEL_GRAD_JSON=<file>: the worst ratios of 4 are merged into that file (profiles/pixel_grad_edges.json)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import pixel_common as pc
from tests import pixel_grad_common as pg
from tests.test_gpu_layer_grad import FLOOR, MARGIN

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
HW = pg.HW


def _dev():
    return torch.device("cuda", 0)


def _merge_json(case, ratios):
    path = os.environ.get("TDMPC2_PIXEL_GRAD_JSON")
    if not path:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc["gate"] = "rel_err(lib) / max(rel_err(torch CPU fp32), 2^-23) <= 4 per tensor, all sides on the saved activations"
    doc.setdefault("ratios", {})[case] = ratios
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)


class Run:
    """One forward (+ backward) of the unit on a case; the saved tensors and results on the CPU."""

    def __init__(self, case, dz=None, preact=False, want=(True,) * 4, pad=0, fill=float("nan")):
        from tdmpc2_amd import native

        dev = _dev()
        self.case, self.n, self.C, self.cin = case, len(case["obs"]), case["C"], case["cin"]
        n, C = self.n, self.C
        obs = case["obs"].to(dev).contiguous()
        self.desc = native.pixgrad_desc(n, self.cin, C, 0 if obs.dtype == torch.uint8 else 1, preact)
        self.obs, self.shift = obs, torch.tensor(case["shifts"], dtype=torch.int32, device=dev)
        self.tab = native.pixgrad_shift_table(dev)
        self.W = [w.to(dev).contiguous() for w in case["Ws"]]
        self.b = [b.to(dev).contiguous() for b in case["Bs"]]
        self.bytes = native.pixgrad_workspace_bytes(self.desc)
        self.pad = pad
        mk = lambda nbytes: torch.full((nbytes // 4 + 2 * pad,), fill, dtype=torch.float32, device=dev)  # noqa: E731
        self._acts, self._fwd_ws, self._bwd_ws = (mk(x) for x in self.bytes)
        self.want = want
        self._dW = [mk(4 * w.numel()) if k else None for w, k in zip(self.W, want)]
        self._db = [mk(4 * C) if k else None for k in want]
        self.dz = None if dz is None else dz.to(dev, torch.float32).contiguous()

    def _in(self, t):
        return None if t is None else (t[self.pad:t.numel() - self.pad] if self.pad else t)

    def forward(self):
        from tdmpc2_amd import native

        native.pixgrad_forward(self.desc, self.obs, self.shift, self.tab, self.W, self.b, self._in(self._fwd_ws), self._in(self._acts))
        return self

    def backward(self):
        from tdmpc2_amd import native

        native.pixgrad_backward(self.desc, self.obs, self.shift, self.tab, self.W, self._in(self._acts), self.dz, self._in(self._bwd_ws),
                                [self._in(t) for t in self._dW], [self._in(t) for t in self._db])
        return self

    # ---- results (CPU)
    def saved(self):
        n, C = self.n, self.C
        a = self._in(self._acts).cpu()
        per = a[:n * 1046 * C].view(n, 1046 * C)
        acts, off = [], 0
        for l in range(3):
            acts.append(per[:, off:off + C * HW[l]].reshape(n, C, pg.OUT[l], pg.OUT[l]).clone())
            off += C * HW[l]
        return acts, a[n * 1046 * C:].view(n, 16 * C).clone()

    def dys(self):
        n, C = self.n, self.C
        w, out, off = self._in(self._bwd_ws).cpu(), [], 0
        for l in range(4):
            out.append(w[off:off + n * C * HW[l]].view(n, C, pg.OUT[l], pg.OUT[l]).clone())
            off += n * C * HW[l]
        return out

    def grads(self):
        dW = [None if t is None else self._in(t).cpu().view(w.shape) for t, w in zip(self._dW, self.W)]
        return dW, [None if t is None else self._in(t).cpu() for t in self._db]

    def buffers(self):
        return [t for t in (self._acts, self._fwd_ws, self._bwd_ws, *self._dW, *self._db) if t is not None]


def _planner(C, max_envs):
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.native import NativePlanner

    cfg = named_config("c1")
    cfg.latent_dim, cfg.num_channels, cfg.obs = 16 * C, C, "rgb"
    return NativePlanner(cfg, cfg.iterations, _dev(), max_envs=max_envs)


# ------------------------------------------------------------------------------------------------------------ 1 forward identity
@pytest.mark.parametrize("fp32", [False, True], ids=["u8", "fp32"])
@pytest.mark.parametrize("n", [1, 2, 17])
def test_forward_is_the_batch_route_bit_for_bit(n, fp32):
    case = pg.grad_case(32, 9, n=n, fp32=fp32)
    run = Run(case).forward()
    acts, z = run.saved()
    p = _planner(32, 4)
    p.bind_pixel_encoder({k: v.to(_dev()) for k, v in pc.state_dict(case["Ws"], case["Bs"]).items()})
    p.reserve_pix_batch(n)
    zb = p.encode_pix_batch(run.obs, run.shift).cpu()
    assert torch.isfinite(z).all() and torch.equal(z, zb)
    ref = pc.reference(case["obs"], case["shifts"], case["Ws"], case["Bs"])
    for l in range(3):
        assert bool(((acts[l].double() - ref["act"][l]).abs() <= ref["g"][l]).all()), l
    assert bool(((z.double() - ref["z"]).abs() <= ref["gz"]).all())
    # layer 0's input as the backward recomputes it: the numpy restatement of the forward's expression is within the input gate
    x0 = pg.x0_fp32(case["obs"], case["shifts"])
    assert float((x0.double() - ref["x"]).abs().max()) <= U * (7.0 * float(np.abs(np.asarray(case["obs"], np.float64)).max()) / 255.0 + 0.5)


# ---------------------------------------------------------------------------------------------------------------- 2 exact probes
PROBE_SHAPES = [(8, 1), (40, 16), (64, 1), (8, 16), (64, 16), (40, 1)]
PROBE_SHIFTS = [(0, 0), (6, 6), (0, 6), (3, 3)]
FINAL_PX = [(0, 0), (3, 3), (0, 3), (3, 0), (1, 2)]


def _probe_case(L, i):
    """Layer L and the layers below it random (default init, positive biases), one-hot layers with bias 1 (an open ReLU) above it
    whose taps read offset PROBE_RC[L][i]; one channel of layer L - 1 closed by its bias."""
    C, cin = PROBE_SHAPES[(L + i) % len(PROBE_SHAPES)]
    twisted = bool(i % 2)
    r, c = pc.PROBE_RC[L][i]
    ty, tx = pc.downstream_taps(L, r), pc.downstream_taps(L, c)
    Wr, Br = pc.default_weights(cin, C, 300 + 10 * L + i)
    Ws, Bs = [], []
    for l in range(4):
        if l <= L:
            W, b = Wr[l], Br[l] + (3.0 if l == L else 0.5)   # the probed layer's own ReLU mostly open, realistic masks below it
        else:
            W, b = pc.one_hot_layer(l, C, C, (ty[l], tx[l]), twisted, 1.0 if l < 3 else 0.0)
        Ws.append(W.clone())
        Bs.append(b.clone())
    closed = 1 % C
    if L >= 1:
        Bs[L - 1][closed] = -1e4
    obs = pc._images(4, cin, 40 + i, fp32=bool(i % 3 == 2))
    oy, ox = FINAL_PX[i % len(FINAL_PX)]
    c3 = (0, C - 1, C // 2)[i % 3]
    e = i % 4
    dz = torch.zeros(4, 16 * C)
    dz[e, c3 * 16 + 4 * oy + ox] = 1.0
    return dict(obs=obs, shifts=PROBE_SHIFTS, Ws=Ws, Bs=Bs, C=C, cin=cin, stack=False), dz, closed


@pytest.mark.parametrize("L,i", pc.PROBES)
def test_exact_probes(L, i):
    case, dz, closed = _probe_case(L, i)
    C, cin = case["C"], case["cin"]
    run = Run(case, dz=dz, preact=True).forward().backward()
    acts, z = run.saved()
    dW, db = run.grads()
    dys = run.dys()
    x0 = pg.x0_fp32(case["obs"], case["shifts"])
    ref = pg.closed_form(x0.double(), [a.double() for a in acts], z.double(), dz.double(), [w.double() for w in case["Ws"]], preact=True)
    # one non-zero element of dy_l at and above L (a value of 1.0, or nothing when the probed pixel's ReLU is closed)
    for l in range(L, 4):
        nz = dys[l].nonzero()
        assert len(nz) <= 1 and torch.equal(dys[l].double(), ref["dy"][l]), l
        assert len(nz) == 0 or float(dys[l][tuple(nz[0])]) == 1.0
        assert torch.equal(dW[l].double(), ref["dW"][l]) and torch.equal(db[l].double(), ref["db"][l]), l
    assert len(dys[3].nonzero()) == 1
    nz = dys[L].nonzero()
    if len(nz):
        e, co, oy, ox = (int(v) for v in nz[0])
        k, S = pg.KERNEL[L], pg.STRIDE[L]
        x_in = x0 if L == 0 else acts[L - 1]
        # dW_L [co] is the input window the pixel reads, db_L is 1 at co, every other row is zero
        assert torch.equal(dW[L][co], x_in[e, :, S * oy:S * oy + k, S * ox:S * ox + k])
        assert float(db[L][co]) == 1.0 and int(db[L].count_nonzero()) == 1
        assert int(dW[L].count_nonzero()) == int(dW[L][co].count_nonzero())
        if L >= 1:
            # dy_{L-1} is the weight under the mask, placed at the window
            want = torch.zeros_like(dys[L - 1])
            want[e, :, S * oy:S * oy + k, S * ox:S * ox + k] = case["Ws"][L][co]
            want = want * (acts[L - 1] > 0)
            assert torch.equal(dys[L - 1], want) and torch.equal(dys[L - 1].double(), ref["dy"][L - 1])
    if L >= 1:
        # the closed channel of layer L - 1: exact zeros in its output, its gradient and everything its gradient feeds
        assert int(acts[L - 1][:, closed].count_nonzero()) == 0 and int(dys[L - 1][:, closed].count_nonzero()) == 0
        assert int(dW[L - 1][closed].count_nonzero()) == 0 and float(db[L - 1][closed]) == 0.0
    for t in (*dW, *db):
        assert torch.isfinite(t).all()


# ---------------------------------------------------------------------------------------------------------------- 3 derived gate
@pytest.mark.parametrize("C,cin", pc.SWEEP)
def test_every_stage_within_its_derived_bound(C, cin):
    case = pg.grad_case(C, cin, n=3)
    run = Run(case, dz=case["G"]).forward().backward()
    acts, z = run.saved()
    dW, db = run.grads()
    dys = run.dys()
    dz = case["G"].float()
    worst = {}

    def hold(name, got, ref, mag, L):
        ratio = float(((got.double() - ref).abs() / ((L + 1) * U * mag).clamp_min(1e-300)).max())
        worst[name] = round(ratio, 3)
        assert ratio <= 1.0, (name, ratio)

    # the seed: eight fmaf, one subtraction, one product
    zz, dd = z.double().reshape(3, -1, 8), dz.double().reshape(3, -1, 8)
    s, sm = (dd * zz).sum(-1, keepdim=True), (dd * zz).abs().sum(-1, keepdim=True)
    hold("dy3", dys[3].reshape(3, -1, 8), zz * (dd - s), zz * (dd.abs() + sm), 10)
    ins = [pg.x0_fp32(case["obs"], case["shifts"]), *acts]
    for l in range(4):
        x64, g64 = ins[l].double(), dys[l].double()
        rw, rb = pg.stage_dw(x64, g64, l)
        mw, mb = pg.stage_dw(x64.abs(), g64.abs(), l)
        Lr = pg.roundings_dw(3 * HW[l])
        hold(f"dW{l}", dW[l].reshape(C, -1), rw, mw, Lr)
        hold(f"db{l}", db[l], rb, mb, Lr)
        if l >= 1:
            W64 = case["Ws"][l].double()
            mask = (acts[l - 1] > 0).double()
            hold(f"dy{l - 1}", dys[l - 1], pg.stage_da(g64, W64, l) * mask, pg.stage_da(g64.abs(), W64.abs(), l), pg.roundings_da(l, C))
            assert int((dys[l - 1] * (1 - mask)).count_nonzero()) == 0
    print((C, cin), worst)


# --------------------------------------------------------------------------------------------------------------- 4 measured gate
@pytest.mark.parametrize("trained", [False, True], ids=["plain", "trained"])
@pytest.mark.parametrize("n", [2, 17])
def test_whole_backward_against_fp64_and_torch_fp32(n, trained):
    case = pg.grad_case(32, 9, n=n, trained=trained)
    run = Run(case, dz=case["G"]).forward().backward()
    acts, z = run.saved()
    dW, db = run.grads()
    x0 = pg.x0_fp32(case["obs"], case["shifts"])
    Wd = [w.double() for w in case["Ws"]]
    dz = case["G"].float()   # what the library was given
    ref = pg.closed_form(x0.double(), [a.double() for a in acts], z.double(), dz.double(), Wd)
    t32 = pg.torch32(x0, acts, z, dz, Wd)
    ratios = {}
    for l in range(4):
        for name, got, r, t in ((f"dW{l}", dW[l], ref["dW"][l], t32["dW"][l]), (f"db{l}", db[l], ref["db"][l], t32["db"][l])):
            ratios[name] = pg.rel_err(got, r) / max(pg.rel_err(t, r), FLOOR)
    print(n, trained, {k: round(v, 2) for k, v in ratios.items()})
    _merge_json(f"C32 cin9 n{n} {'trained' if trained else 'plain'}", ratios)
    for k, r in ratios.items():
        assert r <= MARGIN, (k, r)


# -------------------------------------------------------------------------------------------------------------------- 5 the call
def test_null_pairs_repeat_calls_and_canaries():
    case = pg.grad_case(24, 3, n=2)
    full = Run(case, dz=case["G"], pad=64, fill=7.25).forward().backward()
    dW, db = full.grads()
    again = Run(case, dz=case["G"]).forward().backward()
    dW2, db2 = again.grads()
    assert all(torch.equal(a, b) for a, b in zip(dW + db, dW2 + db2))            # two calls, equal bits
    assert torch.equal(full._in(full._acts).cpu(), again._acts.cpu())
    again.backward()
    dW3, db3 = again.grads()
    assert all(torch.equal(a, b) for a, b in zip(dW + db, dW3 + db3))
    for t in full.buffers():                                                      # nothing outside the reported sizes
        c = t.cpu()
        assert bool((c[:64] == 7.25).all()) and bool((c[-64:] == 7.25).all())
    from tdmpc2_amd import native
    before = native.PIXEL_GRAD_CALLS
    for want in ((False, False, True, True), (True, False, False, True), (False, False, False, True), (True, True, True, False)):
        part = Run(case, dz=case["G"], want=want, pad=64, fill=7.25).forward().backward()
        pW, pb = part.grads()
        for l, k in enumerate(want):
            assert (pW[l] is None) == (not k)
            if k:
                assert torch.equal(pW[l], dW[l]) and torch.equal(pb[l], db[l]), (want, l)
        lowest = min(l for l, k in enumerate(want) if k)
        dys = part.dys()
        for l in range(lowest):   # nothing below the lowest layer asked for is computed: its dy region keeps the fill
            assert bool((dys[l] == 7.25).all()), (want, l)
        for t in part.buffers():
            c = t.cpu()
            assert bool((c[:64] == 7.25).all()) and bool((c[-64:] == 7.25).all())
    assert native.PIXEL_GRAD_CALLS == before + 8


def test_captured_forward_and_backward_replay_the_eager_bits():
    case = pg.grad_case(32, 9, n=3)
    eager = Run(case, dz=case["G"]).forward().backward()
    dW, db = eager.grads()
    cap = Run(case, dz=case["G"], fill=0.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.forward().backward()                        # warm-up off the default stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one linear stream, no parallel branches
        cap.forward().backward()
    for _ in range(2):
        for t in cap.buffers():
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        gW, gb = cap.grads()
        assert all(torch.equal(a, b) for a, b in zip(dW + db, gW + gb))
        assert torch.equal(cap._acts.cpu(), eager._acts.cpu())
