"""CPU: tdmpc2_amd/csrc/task_route.h compiled with the host compiler (tests/task_common.py: SHIM).  The gather's walk writes every
element of `out` exactly once from the source its layout names, on the single-column path and on the 16-byte path; the backward's
grid writes every element of dx, da and dtable exactly once for each set of wanted outputs; the chunk walk lists each task's rows
in rising order, in chunks of TASK_CHUNK, and every row with a valid id exactly once; the chunk walk and the scan past TASK_STAGE
make the same additions, which are the numpy restatement's; the serial renorm is the numpy restatement bit for bit.  The same
walks run as a stand-alone program under AddressSanitizer and UBSan.  Every run here is deterministic."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import task_common as tc

FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    return tc.build_route(tmp_path_factory.mktemp("task_route"))


def _ids(batch, ids_len, id_bytes, one_task=False):
    ids = np.full(ids_len, 7) if one_task else np.arange(ids_len) % tc.NUM_TASKS
    return np.ascontiguousarray(ids, np.int64 if id_bytes == 8 else np.int32)


def test_constants_and_descriptor(route):
    from tdmpc2_amd import native

    out = (C.c_int32 * 8)()
    route.constants(out)
    assert list(out) == [tc.THREADS, tc.WAVE, tc.WAVES, tc.ROWS, tc.COLS, tc.CHUNK, tc.STAGE, 40]
    assert C.sizeof(native.TaskDesc) == C.sizeof(tc.Desc) == 40
    assert [f[0] for f in native.TaskDesc._fields_] == [f[0] for f in tc.Desc._fields_]
    assert tc.THREADS == tc.WAVE * tc.WAVES and tc.COLS == tc.WAVE


def test_refusals_in_the_header_s_order(route):
    fwd = tc.has("table", "ids", "x", "a", "out")

    def chk(op=tc.FORWARD, has=fwd, **kw):
        f = dict(steps=4, batch=12, ids_len=12, id_bytes=8, num_tasks=30, D=8, T=64, A=4)
        f.update(kw)
        return route.check(C.byref(tc.desc_of(**f)), op, has)

    assert chk() == 0 and chk(ids_len=1, id_bytes=4) == 0 and chk(A=0, has=fwd - tc.HAS["a"]) == 0
    assert [chk(steps=0), chk(batch=0), chk(D=0), chk(T=0), chk(A=-1), chk(num_tasks=0)] == [1, 2, 3, 4, 5, 6]
    assert chk(ids_len=2) == 7 and chk(ids_len=0) == 7 and chk(id_bytes=2) == 8 and chk(id_bytes=16) == 8
    for name in ("table", "ids", "x", "out"):
        assert chk(has=fwd - tc.HAS[name]) == 9, name
    assert chk(A=0) == 10 and chk(has=fwd - tc.HAS["a"]) == 11
    bwd = tc.has("ids", "dout", "dx", "da", "dtable")
    assert chk(tc.BACKWARD, bwd) == 0 and chk(tc.BACKWARD, tc.has("ids", "dout", "dtable")) == 0
    assert chk(tc.BACKWARD, tc.has("ids", "dout")) == 12 and chk(tc.BACKWARD, bwd - tc.HAS["dout"]) == 9
    assert chk(tc.BACKWARD, bwd - tc.HAS["ids"]) == 9 and chk(tc.BACKWARD, bwd, A=0) == 10
    assert chk(tc.RENORM, tc.has("table", "ids")) == 0 and chk(tc.RENORM, tc.has("ids")) == 9
    top = (1 << 31) - 1
    assert chk(steps=top, batch=top, ids_len=1) == 13                   # R W >= 2^62
    assert chk(steps=1 << 20, batch=1 << 16, ids_len=1, D=1, T=1, A=1) == 14  # 2^32 gather workgroups
    assert chk(tc.BACKWARD, bwd, steps=1 << 20, batch=1 << 16, ids_len=1) == 14
    assert chk(tc.BACKWARD, tc.has("ids", "dout", "dtable"), steps=1 << 20, batch=1 << 16, ids_len=1) == 0  # sum workgroups alone
    assert chk(steps=top, batch=top, ids_len=1, id_bytes=3) == 8        # INVALID comes before UNSUPPORTED


def test_paths(route):
    d = lambda D, T, A, batch=12: C.byref(tc.desc_of(1, batch, batch, 4, 30, D, T, A))  # noqa: E731
    assert route.vec(d(8, 64, 4), 1) == 1 and route.vec(d(8, 64, 4), 0) == 0 and route.vec(d(8, 64, 0), 1) == 1
    assert not any(route.vec(d(*s), 1) for s in ((5, 64, 4), (8, 63, 4), (8, 64, 6), (1, 1, 0)))
    assert route.staged(d(1, 1, 0, tc.STAGE)) == 1 and route.staged(d(1, 1, 0, tc.STAGE + 1)) == 0
    assert route.staged(C.byref(tc.desc_of(1, tc.STAGE + 1, 1, 4, 30, 1, 1))) == 1  # one id: no list
    assert route.renorm_grid(d(1, 1, 0)) == -(-30 // tc.WAVES)


@pytest.mark.parametrize("id_bytes", (4, 8))
def test_an_id_outside_the_table_reads_as_none(route, id_bytes):
    ids = np.ascontiguousarray([0, 29, 30, -1, 1 << 20, -(1 << 20)], np.int64 if id_bytes == 8 else np.int32)
    d = tc.desc_of(1, 6, 6, id_bytes, 30, 1, 1)
    assert [route.id_read(C.byref(d), ids.ctypes.data, s) for s in range(6)] == [0, 29, -1, -1, -1, -1]
    if id_bytes == 8:  # a value whose low word alone would name a row
        big = np.asarray([(1 << 32) + 3, -(1 << 32) + 3], np.int64)
        assert [route.id_read(C.byref(d), big.ctypes.data, s) for s in range(2)] == [-1, -1]


@pytest.mark.parametrize("shape", tc.SHAPES)
def test_the_walks_cover_every_output_element_exactly_once(route, shape):
    steps, batch, D, T, A = shape
    d = tc.desc_of(steps, batch, batch, 8, tc.NUM_TASKS, D, T, A)
    assert route.gather_grid(C.byref(d)) == -(-steps * batch // tc.ROWS)
    for vec in range(route.vec(C.byref(d), 1) + 1):
        assert route.gather_cover(C.byref(d), vec) == 0
        for dx, da, dt in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 0, 1)):
            if da and not A:
                continue
            assert route.backward_cover(C.byref(d), vec, dx, da, dt) == 0, (vec, dx, da, dt)
    assert route.backward_grid(C.byref(d), 1, 1) == -(-steps * batch // tc.ROWS) + tc.NUM_TASKS * -(-T // tc.COLS)
    assert route.backward_grid(C.byref(d), 0, 1) == tc.NUM_TASKS * -(-T // tc.COLS)
    if shape == (4, 12, 8, 64, 4):
        assert route.vec(C.byref(d), 1) == 1


def _walk(route, d, ids, k):
    R = d.steps * d.batch
    rows, chunk_of = np.zeros(R, np.uint64), np.zeros(R, np.uint64)
    u64p = C.POINTER(C.c_uint64)
    n = route.chunk_walk(C.byref(d), ids.ctypes.data, k, rows.ctypes.data_as(u64p), chunk_of.ctypes.data_as(u64p))
    return rows[:n].astype(np.int64), chunk_of[:n].astype(np.int64)


def _chunk_cases():
    cases = [(s, b, b, False) for s, b, *_ in tc.SHAPES] + [(s, b, 1, True) for s, b, *_ in tc.SHAPES]
    cases += [(1, R, R, True) for R in tc.ONE_TASK_ROWS] + [(1, R, 1, True) for R in tc.ONE_TASK_ROWS]
    return cases + [(3, 43, 43, True), (5, tc.CHUNK // 2 + 1, 1, True)]


@pytest.mark.parametrize("id_bytes", (4, 8))
@pytest.mark.parametrize("case", _chunk_cases())
def test_the_chunk_lists_partition_each_task_s_rows_in_rising_order(route, case, id_bytes):
    steps, batch, ids_len, one_task = case
    ids = _ids(batch, ids_len, id_bytes, one_task)
    d = tc.desc_of(steps, batch, ids_len, id_bytes, tc.NUM_TASKS, 3, 5, 0)
    rid = tc.row_ids(steps, batch, ids)
    for k in range(tc.NUM_TASKS):
        rows, chunk_of = _walk(route, d, ids, k)
        assert rows.tolist() == np.flatnonzero(rid == k).tolist(), k
        assert chunk_of.tolist() == (np.arange(rows.size) // tc.CHUNK).tolist(), k
    if one_task:
        assert _walk(route, d, ids, 7)[0].size == steps * batch


@pytest.mark.parametrize("case", _chunk_cases())
def test_both_sums_make_the_numpy_restatement_s_additions(route, case):
    steps, batch, ids_len, one_task = case
    D, T, A = 3, 5, 2
    ids = _ids(batch, ids_len, 8, one_task)
    d = tc.desc_of(steps, batch, ids_len, 8, tc.NUM_TASKS, D, T, A)
    rng = np.random.default_rng(steps * 1000 + batch)
    dout = (rng.standard_normal((steps * batch, D + T + A)) * 10.0 ** rng.integers(-3, 4, (steps * batch, 1))).astype(np.float32)
    want = tc.dtable32(dout[:, D:D + T], tc.row_ids(steps, batch, ids), tc.NUM_TASKS)
    for which in (0, 1):
        got = np.full((tc.NUM_TASKS, T), np.nan, np.float32)
        route.dtable(C.byref(d), ids.ctypes.data, dout.ctypes.data_as(FP), which, got.ctypes.data_as(FP))
        assert got.tobytes() == want.tobytes(), which
    err = np.abs(want.astype(np.float64) - tc.dtable64(dout[:, D:D + T], tc.row_ids(steps, batch, ids), tc.NUM_TASKS))
    assert (err <= tc.dtable_bound(dout[:, D:D + T], tc.row_ids(steps, batch, ids), tc.NUM_TASKS)).all()


@pytest.mark.parametrize("T", (1, 5, 63, 64, 65, 96, 129))
def test_the_serial_renorm_is_the_numpy_restatement(route, T):
    rng = np.random.default_rng(T)
    for scale in (0.05, 0.3, 4.0):
        row = (rng.standard_normal(T) * scale).astype(np.float32)
        assert np.float32(route.norm(row.ctypes.data_as(FP), T)).tobytes() == tc.norm32(row).tobytes()
        got = row.copy()
        route.renorm_row(got.ctypes.data_as(FP), T, 1.0)
        want = tc.renorm32(row[None], [0], 1.0)
        assert got.tobytes() == want.tobytes()
        ref = tc.renorm64(row[None], [0], 1.0)[0]
        assert (np.abs(got - ref) <= tc.renorm_tol(T) * np.abs(ref)).all()


def test_the_walks_as_a_program_under_the_sanitizers(tmp_path):
    exe = tc.build_walk(tmp_path, sanitize=True)
    res = subprocess.run([exe, tc.walk_input(str(tmp_path / "cases.bin"))], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "bad 0" in res.stdout and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
