"""GPU: the draw unit (tdmpc2_draw_noise, autograd.Draws) against the restatement of tests/draw_common.py.

The pair equals the restatement exactly.  The normals agree with the fp64 restatement from the same words within
8 * 2^-24 * max(|x|, 1) (logf, sqrtf and the product at most 1 ulp each, sincospif about 2, doubled): n of 1, 3, 4, 5 and 4097 and one
n past a single pass of the capped grid, with and without `state`, both outputs and each alone; guard floats behind normal[n - 1]
stay untouched.  A captured draw gives a fresh, restated draw on each of 3 replays; `Draws.state_dict` resumes; the key differs from
`DropoutMasks`' stream.  The worst |x - x64| / (8 * 2^-24 * max(|x64|, 1)) goes to the file TDMPC2_DRAW_JSON names
(profiles/draw_edges.json).  Nothing here reads the reference tree."""
import json
import os

import numpy as np
import pytest
import torch

from tests import draw_common as dr
from tests import dropout_common as dc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = 64  # floats behind every normal buffer
SENTINEL = -777.25
KEY = dr.key_of(20261)


def _merge_json(key, value):
    path = os.environ.get("TDMPC2_DRAW_JSON")
    if not path:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.setdefault("gate", "|x - x64| <= 8 * 2^-24 * max(|x64|, 1) per element, x64 the fp64 Box-Muller step on the same fp32 uniforms; "
                           "values are the worst |x - x64| / (8 * 2^-24 * max(|x64|, 1)); the pair is compared for equality")
    doc[key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def _state(words):
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32, device=DEV)


def _counter(state):
    lo, hi = (int(v) & 0xFFFFFFFF for v in state.tolist())
    return (hi << 32) | lo


def _check(buf, pair, n, num_q, key, call, what):
    """The outputs of one call against the restatement at `call` -> the gate ratio of its normals."""
    ratio = 0.0
    if buf is not None:
        got = buf.cpu().numpy()
        ratio = dr.gate_ratio(got[:n], dr.normals64(n, key, call))
        print(what, "n", n, "worst |x - x64| / (8 * 2^-24 * max(|x64|, 1))", ratio)
        assert np.isfinite(got[:n]).all() and ratio <= 1.0, (what, n, ratio)
        assert (got[n:] == SENTINEL).all(), (what, n, "guard")
    if pair is not None:
        assert tuple(pair.tolist()) == dr.pair_of(num_q, key, call), (what, n, "pair")
    return ratio


@pytest.mark.parametrize("num_q", (2, 5, 8))
def test_normals_and_pair_against_the_restatement(num_q):
    from tdmpc2_amd import native

    calls0 = native.DRAW_CALLS
    start = 0xFFFFFFFE  # the device counter crosses the carry on its second call
    state = _state((start & 0xFFFFFFFF, start >> 32))
    k, worst = 0, 0.0
    for n in dr.GPU_SIZES + ((dr.PAST_ONE_PASS,) if num_q == 5 else ()):
        for want_normal, want_pair in ((True, True), (True, False), (False, True)):
            nn = n if want_normal else 0
            buf = torch.full((n + GUARD,), SENTINEL, device=DEV) if want_normal else None
            pair = torch.full((2,), -9, dtype=torch.int32, device=DEV) if want_pair else None
            # host counter (state NULL): the descriptor's call counter, both words in use
            call = 0x0000000300000000 + n
            native.draw_noise(native.draw_desc(nn, num_q, KEY, call), None, buf, pair)
            worst = max(worst, _check(buf, pair, nn, num_q, KEY, call, "host counter"))
            # device counter: read from state (the descriptor's is ignored), then advanced by one
            if buf is not None:
                buf.fill_(SENTINEL)
            if pair is not None:
                pair.fill_(-9)
            native.draw_noise(native.draw_desc(nn, num_q, KEY, 12345), state, buf, pair)
            worst = max(worst, _check(buf, pair, nn, num_q, KEY, start + k, "device counter"))
            k += 1
            assert _counter(state) == start + k  # after k calls the state reads start + k
    assert native.DRAW_CALLS - calls0 == 2 * k
    _merge_json(f"normals_num_q{num_q}", round(worst, 4))
    # a view at a 16-byte aligned offset is taken, one that is not is refused before anything is written
    buf = torch.full((64,), SENTINEL, device=DEV)
    native.draw_noise(native.draw_desc(5, num_q, KEY, 1), None, buf[4:])
    got = buf.cpu().numpy()
    assert dr.gate_ratio(got[4:9], dr.normals64(5, KEY, 1)) <= 1.0 and (got[9:] == SENTINEL).all() and (got[:4] == SENTINEL).all()
    with pytest.raises(native.NativeError, match="not 16-byte aligned"):
        native.draw_noise(native.draw_desc(5, num_q, KEY, 1), None, buf[2:])
    with pytest.raises(native.NativeError, match="num_q"):
        native.draw_noise(native.draw_desc(5, 9, KEY, 1), None, buf, torch.zeros(2, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == got).all()


def test_the_moments_of_a_large_draw():
    """The kernel's own 2^20 normals: the bounds tests/test_draw_route.py puts on the restatement, and the gate once more."""
    from tdmpc2_amd import native

    n, key = 1 << 20, dr.key_of(1)
    buf = torch.empty(n, device=DEV)
    native.draw_noise(native.draw_desc(n, 0, key, 0), None, buf)
    x = buf.cpu().numpy().astype(np.float64)
    ratio = dr.gate_ratio(x, dr.normals64(n, key, 0))
    print("n 2^20: worst gate ratio", ratio, "mean", x.mean(), "var", x.var())
    _merge_json("normals_2^20", round(ratio, 4))
    assert ratio <= 1.0
    assert abs(x.mean()) <= 6.0 / np.sqrt(n) and abs(x.var() - 1.0) <= 6.0 * np.sqrt(2.0 / n)


def test_draws_state_dict_and_resume():
    from tdmpc2_amd import autograd, native

    seed, num_q = 20261, 5
    dw = autograd.Draws(seed, DEV)
    assert dw.state_dict() == {"seed": seed, "counter": 0} and dw.key == dr.key_of(seed)
    shape = (4, 33, 6)
    n = int(np.prod(shape))
    (a, pa), (b, pb) = dw.draw(shape, num_q), dw.draw(shape, num_q)
    assert a.shape == shape and a.dtype == torch.float32 and a.is_contiguous() and a.data_ptr() != b.data_ptr()
    assert pa.dtype == torch.int32 and pa.shape == (2,) and pa.data_ptr() != pb.data_ptr()
    for call, (m, p) in enumerate(((a, pa), (b, pb))):
        assert dr.gate_ratio(m.cpu().numpy().reshape(-1), dr.normals64(n, dw.key, call)) <= 1.0
        assert tuple(p.tolist()) == dr.pair_of(num_q, dw.key, call)
    sd = dw.state_dict()
    assert sd == {"seed": seed, "counter": 2}
    c, pc = dw.draw((7, 3), num_q)
    other = autograd.Draws(999, DEV)
    other.load_state_dict(sd)
    c2, pc2 = other.draw((7, 3), num_q)
    assert torch.equal(c2, c) and torch.equal(pc2, pc) and other.state_dict()["counter"] == 3
    other.load_state_dict({"seed": 5, "counter": (1 << 32) - 1})  # the carry through a resumed counter
    d, pd = other.draw((9,), 3)
    assert dr.gate_ratio(d.cpu().numpy(), dr.normals64(9, dr.key_of(5), (1 << 32) - 1)) <= 1.0
    assert tuple(pd.tolist()) == dr.pair_of(3, dr.key_of(5), (1 << 32) - 1) and other.state_dict()["counter"] == 1 << 32
    none, pn = other.draw((0, 3), 3)  # no elements: the pair alone, and the counter still advances
    assert none.shape == (0, 3) and tuple(pn.tolist()) == dr.pair_of(3, dr.key_of(5), 1 << 32) and other.state_dict()["counter"] == (1 << 32) + 1
    with pytest.raises(native.NativeError, match="num_q"):
        dw.draw((4,), 1)


def test_a_captured_draw_draws_afresh_on_every_replay():
    from tdmpc2_amd import autograd

    seed, shape, num_q = 77, (3, 5, 67), 5
    n = int(np.prod(shape))
    autograd.Draws(seed, DEV).draw(shape, num_q)  # the kernels are loaded by another stream's first call, outside the capture
    dw = autograd.Draws(seed, DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eps, pair = dw.draw(shape, num_q)
    torch.cuda.synchronize()
    assert dw.state_dict()["counter"] == 0  # nothing ran during the capture
    seen = []
    for r in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got = eps.cpu().numpy().reshape(-1)
        assert dr.gate_ratio(got, dr.normals64(n, dw.key, r)) <= 1.0, r
        assert tuple(pair.tolist()) == dr.pair_of(num_q, dw.key, r), r
        assert all((got != s).any() for s in seen)
        seen.append(got)
    assert dw.state_dict()["counter"] == 3


def test_the_key_keeps_the_stream_apart_from_the_dropout_masks():
    from tdmpc2_amd import autograd

    seed = 20261
    dm, dw = autograd.DropoutMasks(seed, DEV), autograd.Draws(seed, DEV)
    mask = dm.draw((64,), 0.5).cpu().numpy()
    eps, _ = dw.draw((64,), 5)
    eps = eps.cpu().numpy()
    # each stream is the restatement under its own key ...
    assert mask.tobytes() == dc.mask_model(64, 0.5, seed, 0).tobytes()
    assert dr.gate_ratio(eps, dr.normals64(64, dr.key_of(seed), 0)) <= 1.0
    # ... the two keys give the first quad (same counter: quad 0, call 0) different words: a statement about the restatement alone,
    # which no library result enters (the device-side evidence is the line above and the last one) ...
    w_mask, w_draw = dc.philox(np.zeros(1, np.uint64), 0, seed)[0], dc.philox(np.zeros(1, np.uint64), 0, dr.key_of(seed))[0]
    assert (w_mask != w_draw).all()
    # ... and the drawn normals are not those of the masks' words: this is the check that the library keyed the draw apart
    assert dr.gate_ratio(eps[:4], dr.normals_of_words(w_mask[None])[0]) > 1e3
