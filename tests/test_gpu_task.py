"""GPU: the task unit alone (tdmpc2_task_forward / tdmpc2_task_backward / tdmpc2_task_renorm, include/tdmpc2_task.h) against the
numpy restatements of tests/task_common.py.  Every step runs on fresh tensors with guard floats around every output.

Renorm: named rows bit-equal to the fp32 restatement and within task_common.renorm_tol of the fp64 one, unnamed rows and guards
bit-untouched, a second forward inside the same bound.  Forward: `out` bit-equal at four shapes, one id and an id per batch column,
both id widths, spread and single-task ids, with and without renorm, on aligned and misaligned buffers.  Backward: dx and da exact
copies, dtable bit-equal to the fixed-order restatement and within the sequential-sum bound of fp64, zeros for unnamed tasks, at the
same shapes, at the chunk edges, on both sides of TASK_STAGE, each output alone and all three.  Ids outside the table: NaN columns,
everything else as restated.  `autograd.task_concat` against torch's F.embedding(max_norm=1) + cat in fp64.  One forward and one
backward captured in a graph and replayed three times.  The worst renorm ratio goes to the file TDMPC2_TASK_JSON names
(profiles/task_edges.json).  Nothing here reads the reference tree."""
import json
import os

import numpy as np
import pytest
import torch

from tests import task_common as tc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = 64  # floats on either side of every output
SENTINEL = -777.25
NT = tc.NUM_TASKS


def _merge_json(key, value):
    path = os.environ.get("TDMPC2_TASK_JSON")
    if not path:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.setdefault("gate", "renorm: |x - x64| <= 2 (depth(T) + 4) 2^-24 |x64|, depth(T) = 1 + ceil(T / 64) + 6; table gradient: "
                           "|s - s64| <= gamma(min(n, 64) + chunks(n)) sum |terms|; values are the worst error / bound (gate: 1)")
    doc[key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


class Guarded:
    """A device buffer of n floats between two guards; `off` extra floats in front misalign it."""

    def __init__(self, n, init=None, off=0):
        self.n, self.lo = n, GUARD + off
        self.buf = torch.full((n + 2 * GUARD + off,), SENTINEL, device=DEV)
        self.t = self.buf[self.lo:self.lo + n]
        if init is not None:
            self.t.copy_(torch.as_tensor(np.asarray(init, np.float32).reshape(-1)))

    def read(self):
        got = self.buf.cpu().numpy()
        assert (got[:self.lo] == SENTINEL).all() and (got[self.lo + self.n:] == SENTINEL).all(), "guard"
        return got[self.lo:self.lo + self.n]


def _ids(ids_len, id_bytes, one_task=False):
    ids = np.full(ids_len, 7) if one_task else np.arange(ids_len) % NT
    return np.ascontiguousarray(ids, np.int64 if id_bytes == 8 else np.int32)


def _table(T, rng):
    """[NT, T]: rows of norm 0.5, 0.999, 1.001 and 8, e_i (norm exactly 1), 2 e_i (exactly 2), a zero row; every other row's norm
    lies in [0.2, 0.9] or [1.1, 3].  Checked with the fp64 restatement: no norm but e_i's lies within 0.9e-3 of 1."""
    v = rng.standard_normal((NT, T))
    norms = np.where(rng.random(NT) < 0.5, rng.uniform(0.2, 0.9, NT), rng.uniform(1.1, 3.0, NT))
    norms[:4] = (0.5, 0.999, 1.001, 8.0)
    table = (v / np.sqrt((v * v).sum(1, keepdims=True)) * norms[:, None]).astype(np.float32)
    table[4:7] = 0.0
    table[4, 4 % T], table[5, 5 % T] = 1.0, 2.0
    n64 = np.sqrt((table.astype(np.float64) ** 2).sum(1))
    assert n64[4] == 1.0 and n64[5] == 2.0 and n64[6] == 0.0
    assert (np.abs(np.delete(n64, 4) - 1.0) >= 0.9e-3).all()
    return table


def _renorm_ratio(got, table, ids, T):
    """Named rows against fp64 -> the worst |x - x64| / (tol |x64|) (0 / 0 counts as 0)."""
    ref = tc.renorm64(table, ids, 1.0)
    err, bound = np.abs(got.astype(np.float64) - ref), tc.renorm_tol(T) * np.abs(ref)
    assert (err <= bound).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, err / bound, 0.0)
    return float(r.max())


def _desc(shape, ids, max_norm=1.0):
    from tdmpc2_amd import native

    steps, batch, D, T, A = shape
    return native.task_desc(steps, batch, ids.size, ids.itemsize, NT, D, T, A, max_norm)


def _forward(shape, ids, max_norm, table, rng, off=0):
    """One forward on fresh tensors -> (out [R, W], table after, x, a) as numpy, guards checked."""
    from tdmpc2_amd import native

    steps, batch, D, T, A = shape
    R = steps * batch
    x = rng.standard_normal((R, D)).astype(np.float32)
    a = rng.standard_normal((R, A)).astype(np.float32) if A else None
    tb, out = Guarded(NT * T, table, off), Guarded(R * (D + T + A), None, off)
    xg, ag = Guarded(R * D, x, off), (Guarded(R * A, a, off) if A else None)
    native.task_forward(_desc(shape, ids, max_norm), tb.t, torch.as_tensor(ids).to(DEV), xg.t, None if ag is None else ag.t, out.t)
    torch.cuda.synchronize()
    assert xg.read().tobytes() == x.tobytes()
    return out.read().reshape(R, -1), tb.read().reshape(NT, T), x, a


# ---------------------------------------------------------------- renorm
@pytest.mark.parametrize("T", (1, 5, 64, 96, 129))
def test_renorm_gates(T):
    from tdmpc2_amd import native

    rng = np.random.default_rng(100 + T)
    table = _table(T, rng)
    worst = 0.0
    for id_bytes in (4, 8):
        ids = np.ascontiguousarray(np.r_[np.arange(0, NT, 2), [1, 3, 5]], np.int64 if id_bytes == 8 else np.int32)  # 1, 3, 5 and the evens
        named = np.zeros(NT, bool)
        named[ids] = True
        want = tc.renorm32(table, ids, 1.0)
        assert (want[~named] == table[~named]).all() and want[4].tobytes() == table[4].tobytes()  # e_i stays as it is
        assert all(want[k].tobytes() != table[k].tobytes() for k in (2, 3, 5))  # norms 1.001, 8 and 2 are scaled
        d = native.task_desc(1, ids.size, ids.size, id_bytes, NT, 3, T, 0, 1.0)
        # the renorm alone
        tb = Guarded(NT * T, table)
        native.task_renorm(d, tb.t, torch.as_tensor(ids).to(DEV))
        torch.cuda.synchronize()
        got = tb.read().reshape(NT, T)
        assert got.tobytes() == want.tobytes()
        worst = max(worst, _renorm_ratio(got, table, ids, T))
        # the forward's renorm, and a second forward on the same table
        x, out = Guarded(ids.size * 3, rng.standard_normal(ids.size * 3)), Guarded(ids.size * (3 + T))
        tb = Guarded(NT * T, table)
        for call in range(2):
            native.task_forward(d, tb.t, torch.as_tensor(ids).to(DEV), x.t, None, out.t)
            torch.cuda.synchronize()
            got = tb.read().reshape(NT, T)
            if call == 0:
                assert got.tobytes() == want.tobytes()
            assert got[~named].tobytes() == table[~named].tobytes()
            worst = max(worst, _renorm_ratio(got, table, ids, T))
            assert out.read().reshape(ids.size, -1)[:, 3:].tobytes() == got[ids].tobytes()
        # max_norm <= 0: nothing is launched, nothing moves
        tb = Guarded(NT * T, table)
        native.task_renorm(native.task_desc(1, ids.size, ids.size, id_bytes, NT, 3, T, 0, 0.0), tb.t, torch.as_tensor(ids).to(DEV))
        torch.cuda.synchronize()
        assert tb.read().tobytes() == table.tobytes()
    print("T", T, "worst renorm error / bound", worst)
    _merge_json(f"renorm.T{T}", round(worst, 4))


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("shape", tc.SHAPES)
def test_forward_equals_the_restatement(shape):
    steps, batch, D, T, A = shape
    rng = np.random.default_rng(sum(shape))
    table = _table(T, rng)
    for per_row in (False, True):
        for id_bytes in (4, 8):
            for one_task in (False, True):
                for max_norm in (1.0, 0.0):
                    for off in ((0, 1) if (id_bytes == 8 and not one_task) else (0,)):  # 1: no pointer is 16-byte aligned
                        ids = _ids(batch if per_row else 1, id_bytes, one_task)
                        out, after, x, a = _forward(shape, ids, max_norm, table, rng, off)
                        want_table = tc.renorm32(table, ids, max_norm)
                        want = tc.gather(want_table, tc.row_ids(steps, batch, ids), x, a)
                        what = (per_row, id_bytes, one_task, max_norm, off)
                        assert after.tobytes() == want_table.tobytes(), what
                        assert out.tobytes() == want.tobytes(), what
                        if max_norm == 0.0:
                            assert after.tobytes() == table.tobytes(), what


# ---------------------------------------------------------------- backward
def _backward_case(shape, ids, rng, num_tasks=NT, offs=(0,)):
    from tdmpc2_amd import native

    steps, batch, D, T, A = shape
    R, W = steps * batch, D + T + A
    dout = (rng.standard_normal((R, W)) * 10.0 ** rng.integers(-3, 4, (R, 1))).astype(np.float32)
    rid = tc.row_ids(steps, batch, ids)
    g = dout[:, D:D + T]
    want = tc.dtable32(g, rid, num_tasks)
    err, bound = np.abs(want.astype(np.float64) - tc.dtable64(g, rid, num_tasks)), tc.dtable_bound(g, rid, num_tasks)
    assert (err <= bound).all()  # (the kernel's result is compared with `want` bit for bit below)
    named = np.zeros(num_tasks, bool)
    named[rid[tc.valid(rid, num_tasks)]] = True
    assert not want[~named].any()
    d = native.task_desc(steps, batch, ids.size, ids.itemsize, num_tasks, D, T, A, 1.0)
    idt = torch.as_tensor(ids).to(DEV)
    combos = [(1, 0, 0), (0, 0, 1), (1, 1, 1)] + ([(0, 1, 0)] if A else [])
    for off in offs:
        for want_dx, want_da, want_dt in combos:
            want_da = want_da and A > 0
            dg = Guarded(R * W, dout, off)
            dx = Guarded(R * D, None, off) if want_dx else None
            da = Guarded(R * A, None, off) if want_da else None
            dt = Guarded(num_tasks * T, None, off) if want_dt else None
            native.task_backward(d, idt, dg.t, *(None if b is None else b.t for b in (dx, da, dt)))
            torch.cuda.synchronize()
            what = (shape, ids.size, ids.itemsize, off, want_dx, want_da, want_dt)
            assert dg.read().tobytes() == dout.tobytes(), what
            if dx is not None:
                assert dx.read().tobytes() == np.ascontiguousarray(dout[:, :D]).tobytes(), what
            if da is not None:
                assert da.read().tobytes() == np.ascontiguousarray(dout[:, D + T:]).tobytes(), what
            if dt is not None:
                assert dt.read().tobytes() == want.tobytes(), what
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(bound > 0, err / bound, 0.0).max())


@pytest.mark.parametrize("shape", tc.SHAPES)
def test_backward_equals_the_restatement(shape):
    batch = shape[1]
    rng = np.random.default_rng(7 + sum(shape))
    worst = 0.0
    for per_row in (False, True):
        for id_bytes in (4, 8):
            for one_task in (False, True):
                ids = _ids(batch if per_row else 1, id_bytes, one_task)
                worst = max(worst, _backward_case(shape, ids, rng, offs=(0, 1) if id_bytes == 8 else (0,)))
    print(shape, "worst fixed-order error / bound", worst)
    _merge_json("dtable." + "x".join(str(v) for v in shape), round(worst, 4))


@pytest.mark.parametrize("R", tc.ONE_TASK_ROWS)
def test_backward_at_the_chunk_edges(R):
    rng = np.random.default_rng(R)
    for id_bytes in (4, 8):
        _backward_case((1, R, 3, 5, 2), _ids(R, id_bytes, one_task=True), rng)   # an id per row, all the same
        _backward_case((1, R, 3, 5, 2), _ids(1, id_bytes, one_task=True), rng)   # one id
    _backward_case((R, 1, 4, 8, 4), _ids(1, 8, one_task=True), rng)              # R steps of one batch column
    if R == tc.CHUNK + 1:
        _backward_case((5, 13, 3, 5, 0), _ids(13, 8, one_task=True), rng)        # a chunk that wraps from one step into the next


@pytest.mark.parametrize("batch", (tc.STAGE, tc.STAGE + 1))
def test_backward_on_both_sides_of_the_staged_list(batch):
    rng = np.random.default_rng(batch)
    for steps in (1, 2):
        _backward_case((steps, batch, 1, 3, 0), np.ascontiguousarray(np.arange(batch) % 5, np.int32), rng, num_tasks=6)
    _backward_case((1, batch, 1, 3, 0), _ids(batch, 8, one_task=True), rng, num_tasks=8)


# ---------------------------------------------------------------- ids outside the table
@pytest.mark.parametrize("id_bytes", (4, 8))
def test_ids_outside_the_table(id_bytes):
    shape = (3, 12, 8, 64, 4)
    steps, batch, D, T, A = shape
    rng = np.random.default_rng(id_bytes)
    table = _table(T, rng)
    ids = _ids(batch, id_bytes)
    ids[2], ids[5], ids[9] = -1, NT, 3  # two ids name no row; 3 is named twice
    for off in (0, 1):
        out, after, x, a = _forward(shape, ids, 1.0, table, rng, off)
        want_table = tc.renorm32(table, ids, 1.0)
        assert after.tobytes() == want_table.tobytes()
        want = tc.gather(want_table, tc.row_ids(steps, batch, ids), x, a)
        bad = ~tc.valid(tc.row_ids(steps, batch, ids), NT)
        assert bad.sum() == 2 * steps and np.isnan(out[bad][:, D:D + T]).all() and np.isnan(want[bad][:, D:D + T]).all()
        assert out[~bad].tobytes() == want[~bad].tobytes()
        assert out[bad][:, :D].tobytes() == want[bad][:, :D].tobytes() and out[bad][:, D + T:].tobytes() == want[bad][:, D + T:].tobytes()
    _backward_case(shape, ids, rng, offs=(0, 1))
    one = np.ascontiguousarray([NT + 4], ids.dtype)  # one id for every row, outside the table
    out, after, x, a = _forward(shape, one, 1.0, table, rng)
    assert after.tobytes() == table.tobytes() and np.isnan(out[:, D:D + T]).all()
    assert out[:, :D].tobytes() == x.tobytes() and out[:, D + T:].tobytes() == a.tobytes()
    _backward_case(shape, one, rng)


# ---------------------------------------------------------------- autograd
@pytest.mark.parametrize("shape", ((4, 12, 8, 64, 4), (3, 43, 24, 96, 6), (1, 43, 5, 64, 0)))
def test_task_concat_against_torch_in_fp64(shape):
    import torch.nn.functional as F

    from tdmpc2_amd import autograd, native

    steps, batch, D, T, A = shape
    rng = np.random.default_rng(11 + sum(shape))
    table = _table(T, rng)
    ids = torch.as_tensor(_ids(batch, 8)).to(DEV)
    x = rng.standard_normal((steps, batch, D)).astype(np.float32)
    a = rng.standard_normal((steps, batch, A)).astype(np.float32) if A else None
    gw = rng.standard_normal((steps, batch, D + T + A)).astype(np.float32)
    if steps == 1:  # the 2-D branch with an id per row
        x, gw, a = x[0], gw[0], (None if a is None else a[0])
    # torch, fp64, on a copy
    w64 = torch.tensor(table, dtype=torch.float64, device=DEV, requires_grad=True)
    x64 = torch.tensor(x, dtype=torch.float64, device=DEV, requires_grad=True)
    a64 = None if a is None else torch.tensor(a, dtype=torch.float64, device=DEV, requires_grad=True)
    emb = F.embedding(ids, w64, max_norm=1.0)
    if x64.dim() == 3:
        emb = emb.unsqueeze(0).repeat(steps, 1, 1)
    ref = torch.cat([x64, emb] + ([a64] if a64 is not None else []), dim=-1)
    (ref * torch.tensor(gw, dtype=torch.float64, device=DEV)).sum().backward()
    rid = tc.row_ids(steps, batch, ids.cpu().numpy())
    bound_t = tc.dtable_bound(gw.reshape(-1, D + T + A)[:, D:D + T], rid, NT)
    tol = tc.renorm_tol(T)
    for need in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
        if need[2] and a is None:
            continue
        w = torch.tensor(table, device=DEV, requires_grad=need[0])
        xt = torch.tensor(x, device=DEV, requires_grad=need[1])
        at = None if a is None else torch.tensor(a, device=DEV, requires_grad=need[2])
        before = native.TASK_CALLS
        out = autograd.task_concat(w, ids, xt, at, max_norm=1.0)
        assert native.TASK_CALLS == before + 1 and out.shape == ref.shape and out.requires_grad
        (out * torch.tensor(gw, device=DEV)).sum().backward()
        assert native.TASK_CALLS == before + 2
        torch.cuda.synchronize()
        r64, o = ref.detach().cpu().numpy(), out.detach().cpu().numpy().astype(np.float64)
        assert (np.abs(o - r64) <= tol * np.abs(r64)).all()
        assert o[..., :D].tobytes() == r64[..., :D].tobytes() and o[..., D + T:].tobytes() == r64[..., D + T:].tobytes()
        w_after = w64.detach().cpu().numpy()
        assert (np.abs(w.detach().cpu().numpy() - w_after) <= tol * np.abs(w_after)).all()
        assert (w.grad is not None) == need[0] and (xt.grad is not None) == need[1]
        if need[0]:
            assert (np.abs(w.grad.cpu().numpy() - w64.grad.cpu().numpy()) <= bound_t).all()
            assert not w.grad.cpu().numpy()[~np.isin(np.arange(NT), rid)].any()
        if need[1]:
            assert xt.grad.cpu().numpy().astype(np.float64).tobytes() == x64.grad.cpu().numpy().tobytes()
        if at is not None:
            assert (at.grad is not None) == need[2]
            if need[2]:
                assert at.grad.cpu().numpy().astype(np.float64).tobytes() == a64.grad.cpu().numpy().tobytes()
    # nothing needs a gradient: no node, no backward call
    before = native.TASK_CALLS
    out = autograd.task_concat(torch.tensor(table, device=DEV), ids, torch.tensor(x, device=DEV), None if a is None else torch.tensor(a, device=DEV))
    assert not out.requires_grad and native.TASK_CALLS == before + 1
    # one id for every row, given as an int
    out = autograd.task_concat(torch.tensor(table, device=DEV), 5, torch.tensor(x, device=DEV), None if a is None else torch.tensor(a, device=DEV))
    want = tc.gather(tc.renorm32(table, [5], 1.0), np.full(steps * batch, 5), x, a)
    assert out.cpu().numpy().reshape(want.shape).tobytes() == want.tobytes()


# ---------------------------------------------------------------- capture
def test_a_captured_forward_and_backward_replay():
    from tdmpc2_amd import native

    shape = (3, 43, 24, 96, 6)
    steps, batch, D, T, A = shape
    R, W = steps * batch, D + T + A
    ids_np = _ids(batch, 8)
    d = _desc(shape, ids_np)
    ids = torch.as_tensor(ids_np).to(DEV)
    new = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    table, x, a, out, dout = new(NT, T), new(R, D), new(R, A), new(R, W), new(R, W)
    dx, da, dtable = new(R, D), new(R, A), new(NT, T)

    def calls(tb, xx, aa, oo, dd, gx, ga, gt):
        native.task_forward(d, tb, ids, xx, aa, oo)
        native.task_backward(d, ids, dd, gx, ga, gt)

    calls(table.clone(), x, a, out, dout, dx, da, dtable)  # the kernels are loaded outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        calls(table, x, a, out, dout, dx, da, dtable)
    torch.cuda.synchronize()
    rng = np.random.default_rng(5)
    for r in range(3):
        tb_np = _table(T, rng)
        for dst, src in ((table, tb_np), (x, rng.standard_normal((R, D))), (a, rng.standard_normal((R, A))),
                         (dout, rng.standard_normal((R, W)))):
            dst.copy_(torch.as_tensor(np.asarray(src, np.float32)))
        eager_in = [t.clone() for t in (table, x, a, dout)]
        graph.replay()
        torch.cuda.synchronize()
        e_out, e_dx, e_da, e_dt = new(R, W), new(R, D), new(R, A), new(NT, T)
        calls(eager_in[0], eager_in[1], eager_in[2], e_out, eager_in[3], e_dx, e_da, e_dt)
        torch.cuda.synchronize()
        for got, want in ((table, eager_in[0]), (out, e_out), (dx, e_dx), (da, e_da), (dtable, e_dt)):
            assert torch.equal(got, want), r
        assert table.cpu().numpy().tobytes() == tc.renorm32(tb_np, ids_np, 1.0).tobytes()
        assert dtable.cpu().numpy().tobytes() == tc.dtable32(dout.cpu().numpy()[:, D:D + T], tc.row_ids(steps, batch, ids_np), NT).tobytes()
