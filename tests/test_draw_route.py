"""CPU: tdmpc2_amd/csrc/draw_route.h compiled with the host compiler (tests/draw_common.py: SHIM).  Its words, its uniforms, its fp64
normals and its pair equal the numpy restatement (words and pair bit for bit; normals to fp64 rounding) at n of 1, 2, 3, 4, 5 and
4097, at quads past 2^32 and across the counter's carry; the grid walks every quad exactly once at those n and at one n beyond a
single pass of the capped grid, and the same walk runs as a stand-alone program under AddressSanitizer and UBSan; the pair rule holds
at its edge words, and over 2^16 consecutive counters every ordered pair's count lies within 6 binomial sigma of its share; the
normals' mean and variance over 2^20 elements lie within 6 sigma of 0 and 1.  Every run here is deterministic."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import draw_common as dr

DP = C.POINTER(C.c_double)
KEY, CALL = 0x1234567887654321, 0x0000000500000007


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    return dr.build_route(tmp_path_factory.mktemp("draw_route"))


def _fill(route, d, call, first, count):
    out = np.empty(count, np.float64)
    route.fill(C.byref(d), call, first, count, out.ctypes.data_as(DP))
    return out


def test_constants_and_descriptor(route):
    from tdmpc2_amd import native

    out = (C.c_int32 * 4)()
    route.constants(out)
    assert list(out) == [dr.THREADS, dr.MAX_BLOCKS, dr.MAXQ, 32] and C.sizeof(native.DrawDesc) == C.sizeof(dr.Desc) == 32
    assert [f[0] for f in native.DrawDesc._fields_] == [f[0] for f in dr.Desc._fields_]
    assert dr.ONE_PASS == 4 * 256 * 2048 and route.grid(dr.ONE_PASS) == 2048 == route.grid(dr.ONE_PASS + 1)
    assert route.grid(0) == 1 == route.grid(1)  # the pair alone still takes a workgroup
    assert native.DRAW_KEY_HI == dr.KEY_HI == int.from_bytes(b"DRAW", "big")


def test_refusals_in_the_header_s_order(route):
    chk = lambda n=5, q=5, normal=True, pair=True, addr=256: route.check(C.byref(dr.desc_of(n, q)), normal, pair, addr)  # noqa: E731
    assert chk() == 0 and chk(pair=False, q=0) == 0 and chk(n=0, normal=False) == 0 and chk(n=(1 << 62) - 1) == 0
    assert chk(q=2) == 0 and chk(q=8) == 0
    assert chk(normal=False, pair=False) == 1
    assert chk(n=-1) == 2 and chk(n=-(1 << 62)) == 2
    assert chk(n=0) == 3
    assert chk(n=5, normal=False) == 4
    assert [chk(addr=256 + o) for o in (1, 4, 8, 12)] == [5] * 4
    assert chk(q=1) == 6 and chk(q=9) == 6 and chk(q=0) == 6 and chk(q=-3) == 6
    assert chk(n=1 << 62) == 7 and chk(n=(1 << 63) - 1) == 7
    assert chk(n=1 << 62, addr=260) == 5  # INVALID comes before UNSUPPORTED


def test_uniform_of_a_word(route):
    edge = np.asarray([0, 255, 256, 1 << 31, (1 << 31) + 256, 0xFFFFFE00, 0xFFFFFF00, 0xFFFFFFFF], np.uint32)
    rng = np.random.default_rng(3)
    xs = np.concatenate([edge, rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32)])
    got = np.asarray([route.u01(int(x)) for x in xs], np.float32)
    assert got.tobytes() == dr.u01(xs).tobytes()
    assert got.min() == np.float32(2.0 ** -25) and got.max() == 1.0 and (got > 0).all()  # never 0: the logarithm is finite


@pytest.mark.parametrize("n", dr.SIZES)
def test_words_and_normals_equal_the_numpy_restatement(route, n):
    d = dr.desc_of(n, 5, KEY)
    quads = (n + 3) // 4
    w = np.zeros((quads, 4), np.uint32)
    for q in range(quads):
        route.quad_words(C.byref(d), CALL, q, w[q].ctypes.data_as(C.POINTER(C.c_uint32)))
    assert w.tobytes() == dr.words(n, KEY, CALL).tobytes()
    got, want = _fill(route, d, CALL, 0, n), dr.normals64(n, KEY, CALL)
    # libm's and numpy's fp64 log / sin / cos agree to a few fp64 ulps: nine orders of magnitude below the fp32 gate
    assert np.abs(got - want).max() <= 1e-13 and np.isfinite(got).all()
    assert route.serial(C.byref(d), CALL, n - 1) == got[-1]


def test_quads_past_2_32_and_the_counter_carry(route):
    d = dr.desc_of(1 << 40, 5, 77)
    first = ((1 << 32) - 3) * 4 + 1  # straddles q_hi 0 -> 1
    got = _fill(route, d, 9, first, 40)
    assert np.abs(got - dr.normals64(40, 77, 9, first=first)).max() <= 1e-13
    assert route.quad_of(first) == (1 << 32) - 3 and route.quad_of(first + 39) == (1 << 32) + 7 and route.lane_of(first) == 1
    assert route.bump(0xFFFFFFFF) == 1 << 32 and route.bump((1 << 64) - 1) == 0 and route.bump(0) == 1
    a, b = _fill(route, d, 0xFFFFFFFF, 0, 9), _fill(route, d, 1 << 32, 0, 9)
    assert np.abs(a - dr.normals64(9, 77, 0xFFFFFFFF)).max() <= 1e-13 and np.abs(b - dr.normals64(9, 77, 1 << 32)).max() <= 1e-13
    assert (a != b).all() and (b != _fill(route, d, 0, 0, 9)).all()  # call_lo and call_hi enter the counter


@pytest.mark.parametrize("n", dr.SIZES + (dr.PAST_ONE_PASS,))
def test_the_grid_covers_every_element_exactly_once(route, n):
    quads = (n + 3) // 4
    assert route.grid(n) == min(-(-quads // dr.THREADS), dr.MAX_BLOCKS)
    assert route.cover(n) == 0
    assert route.quad_elems(quads - 1, n) == (n - 1) % 4 + 1 and (quads == 1 or route.quad_elems(quads - 2, n) == 4)
    if n == dr.PAST_ONE_PASS:  # a second pass: thread 0 of workgroup 0 takes quad grid * 256 next
        assert route.grid(n) == dr.MAX_BLOCKS and route.quad_stride(route.grid(n)) == dr.ONE_PASS // 4 < quads
    assert route.first_quad(3, 17) == 3 * 256 + 17


def test_the_walk_as_a_program_under_the_sanitizers(tmp_path):
    exe = dr.build_walk(tmp_path, sanitize=True)
    res = subprocess.run([exe, dr.walk_input(str(tmp_path / "sizes.bin"))], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "bad 0" in res.stdout and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr


# ---------------------------------------------------------------- the pair
@pytest.mark.parametrize("num_q", range(2, dr.MAXQ + 1))
def test_the_pair_rule_at_its_edge_words(route, num_q):
    out = (C.c_int32 * 2)()
    for w0, w1 in ((0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0, 0xFFFFFFFF), (0xFFFFFFFF, 0)):
        route.pair_rule(w0, w1, num_q, out)
        i, j = out
        assert (i, j) == dr.pair_rule(w0, w1, num_q) and i != j and 0 <= i < num_q and 0 <= j < num_q, (w0, w1)
    route.pair_rule(0, 0, num_q, out)
    assert tuple(out) == (0, 1)  # k = 0 >= i = 0: stepped over i
    route.pair_rule(0xFFFFFFFF, 0xFFFFFFFF, num_q, out)
    assert tuple(out) == (num_q - 1, num_q - 2)  # k = num_q - 2 < i: kept


@pytest.mark.parametrize("num_q", dr.NUM_QS)
def test_every_ordered_pair_gets_its_share(route, num_q):
    count, key = 1 << 16, dr.key_of(7)
    d = dr.desc_of(0, num_q, key)
    counts = np.zeros(num_q * num_q, np.uint64)
    route.pair_counts(C.byref(d), 0, count, counts.ctypes.data_as(C.POINTER(C.c_uint64)))
    counts = counts.reshape(num_q, num_q).astype(np.int64)
    assert counts.sum() == count and not np.diag(counts).any()
    p = 1.0 / (num_q * (num_q - 1))
    dev = np.abs(counts[~np.eye(num_q, dtype=bool)] - count * p) / np.sqrt(count * p * (1.0 - p))
    print(num_q, "worst deviation", float(dev.max()), "sigma")
    assert dev.max() <= 6.0
    # the first counters against the numpy restatement, the pair's counter being the one no quad reaches
    out = (C.c_int32 * 2)()
    for call in (0, 1, 2, 0xFFFFFFFF, 1 << 32):
        route.pair(C.byref(d), call, out)
        assert tuple(out) == dr.pair_of(num_q, key, call), call


# ---------------------------------------------------------------- the normals' moments
def test_mean_and_variance_of_the_restated_normals():
    n = 1 << 20
    x = dr.normals64(n, dr.key_of(1), 0)
    mean, var = float(x.mean()), float(x.var())
    print("mean", mean, "bound", 6 / np.sqrt(n), "var - 1", var - 1, "bound", 6 * np.sqrt(2 / n))
    assert abs(mean) <= 6.0 / np.sqrt(n)
    assert abs(var - 1.0) <= 6.0 * np.sqrt(2.0 / n)
    assert np.isfinite(x).all() and np.abs(x).max() < 6.0  # sqrt(-2 ln 2^-25) = 5.89
