"""CPU: tdmpc2_amd/csrc/dropout_route.h compiled with the host compiler (tests/dropout_common.py: SHIM): `drop_serial` equals the numpy
Philox restatement bit for bit at n of 1, 3, 4, 5, 1023 and 1025, at quads past 2^32 and across the counter's carry; the threshold and
the kept value are torch's for the five p values; the grid walks every quad exactly once at those n and at one n beyond a single pass of
the capped grid.  The same walk runs as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import dropout_common as dc

FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    return dc.build_route(tmp_path_factory.mktemp("dropout_route"))


def _fill(route, d, call, first, count):
    out = np.empty(count, np.float32)
    route.fill(C.byref(d), call, first, count, out.ctypes.data_as(FP))
    return out


def test_constants_and_descriptor(route):
    from tdmpc2_amd import native

    out = (C.c_int32 * 3)()
    route.constants(out)
    assert list(out) == [dc.THREADS, dc.MAX_BLOCKS, 32] and C.sizeof(native.DropoutDesc) == C.sizeof(dc.Desc) == 32
    assert [f[0] for f in native.DropoutDesc._fields_] == [f[0] for f in dc.Desc._fields_]
    assert dc.ONE_PASS == 4 * 256 * 2048 and route.grid(dc.ONE_PASS) == 2048 == route.grid(dc.ONE_PASS + 1)


def test_descriptor_refusals(route):
    ok = lambda **kw: route.check(C.byref(dc.desc_of(**{**dict(n=5, p=0.25), **kw})))  # noqa: E731
    assert ok() == 0 and ok(p=0.0) == 0 and ok(n=1) == 0 and ok(n=(1 << 62) - 1) == 0
    assert ok(n=0) == 1 and ok(n=-3) == 1
    assert ok(p=-0.1) == 2 and ok(p=1.0) == 2 and ok(p=1.5) == 2 and ok(p=float("nan")) == 2
    assert ok(n=1 << 62) == 3 and ok(n=(1 << 63) - 1) == 3


@pytest.mark.parametrize("p", dc.PS)
def test_threshold_and_kept_value_are_torch_s(route, p):
    import torch
    import torch.nn.functional as F

    thr, keep = route.thr(p), np.float32(route.keep(p))
    assert thr == dc.thr_of(p) == int(np.floor(float(np.float32(p)) * 2.0 ** 32)) and 0 < thr < 2 ** 32
    assert abs(thr / 2.0 ** 32 - p) <= 2.0 ** -32 + p * 2.0 ** -24  # P(drop) is p to the rounding of p to fp32 and one count
    # torch is handed the p the descriptor carries: the fp32 value, widened (0.9 is 0.89999997615...)
    pf = float(np.float32(p))
    torch.manual_seed(5)
    m = F.dropout(torch.ones(1 << 20), pf, True).numpy()
    kept = np.unique(m[m != 0])
    assert kept.size == 1 and kept[0].tobytes() == keep.tobytes() == dc.keep_of(p).tobytes(), (kept, keep)
    # the expression chosen: fp32 one over fp32 (1 - p), what torch's fp32 division of the mask by the scalar gives; the other
    # candidate, fp64 1 / (1 - p) rounded once, is the same number at these five p and so cannot be told apart here
    assert keep.tobytes() == (np.float32(1.0) / np.float32(1.0 - pf)).tobytes() == np.float32(1.0 / (1.0 - pf)).tobytes()
    # handed the double p instead, torch gives the same multiplier exactly when rounding p to fp32 does not move fp32(1 - p): at
    # 0.01, 0.1, 0.25 and 0.5 it does not; at 0.9 it does (10.0 against 9.999998 for the descriptor's 0.89999998)
    kd = np.unique(F.dropout(torch.ones(1 << 12), p, True).numpy())[-1]
    assert (kd.tobytes() == keep.tobytes()) == (np.float32(1.0 - p) == np.float32(1.0 - pf)) == (p != 0.9), (p, kd, keep)
    # torch's own drop frequency agrees with thr / 2^32 to sampling accuracy
    q, n = thr / 2.0 ** 32, m.size
    assert abs(float((m == 0).sum()) - n * q) <= 5.0 * np.sqrt(n * q * (1.0 - q))


def test_p_zero_keeps_everything_at_exactly_one(route):
    assert route.thr(0.0) == 0 and route.keep(0.0) == 1.0
    got = _fill(route, dc.desc_of(1025, 0.0, seed=9), 4, 0, 1025)
    assert (got == 1.0).all() and got.tobytes() == dc.mask_model(1025, 0.0, 9, 4).tobytes()


@pytest.mark.parametrize("n", dc.SIZES)
@pytest.mark.parametrize("p", (0.01, 0.25, 0.9))
def test_serial_equals_the_numpy_restatement(route, n, p):
    seed, call = 0x1234567887654321, 0x0000000500000007
    got = _fill(route, dc.desc_of(n, p, seed=seed), call, 0, n)
    want = dc.mask_model(n, p, seed, call)
    assert got.tobytes() == want.tobytes()
    assert set(np.unique(got).tolist()) <= {0.0, float(dc.keep_of(p))} and not np.signbit(got).any()
    assert np.float32(route.serial(C.byref(dc.desc_of(n, p, seed=seed)), call, n - 1)).tobytes() == want[-1:].tobytes()


def test_quads_past_2_32_and_the_counter_carry(route):
    d, seed = dc.desc_of(1 << 40, 0.5, seed=77), 77
    first = ((1 << 32) - 3) * 4 + 1  # straddles q_hi 0 -> 1
    got = _fill(route, d, 9, first, 40)
    assert got.tobytes() == dc.mask_model(40, 0.5, seed, 9, first=first).tobytes()
    assert route.quad_of(first) == (1 << 32) - 3 and route.quad_of(first + 39) == (1 << 32) + 7 and route.lane_of(first) == 1
    # q_hi enters the counter: the same q_lo under q_hi 0 and 1 gives different words
    lo = dc.philox(np.asarray([5, (1 << 32) + 5], np.uint64), 9, seed)
    assert (lo[0] != lo[1]).any()
    # the carry: 0xFFFFFFFF + 1 -> (0, 1), and the masks on either side are the restatement's at those counters
    assert route.bump(0xFFFFFFFF) == 1 << 32 and route.bump((1 << 64) - 1) == 0 and route.bump(0) == 1
    a, b = _fill(route, d, 0xFFFFFFFF, 0, 1025), _fill(route, d, 1 << 32, 0, 1025)
    assert a.tobytes() == dc.mask_model(1025, 0.5, seed, 0xFFFFFFFF).tobytes()
    assert b.tobytes() == dc.mask_model(1025, 0.5, seed, 1 << 32).tobytes() and a.tobytes() != b.tobytes()
    assert b.tobytes() != _fill(route, d, 0, 0, 1025).tobytes()  # call_hi enters the counter


@pytest.mark.parametrize("n", dc.SIZES + (dc.PAST_ONE_PASS,))
def test_the_grid_covers_every_quad_exactly_once(route, n):
    quads = (n + 3) // 4
    assert route.grid(n) == min(-(-quads // dc.THREADS), dc.MAX_BLOCKS)
    assert route.cover(n) == 0
    assert route.quad_elems(quads - 1, n) == (n - 1) % 4 + 1 and (quads == 1 or route.quad_elems(quads - 2, n) == 4)
    if n == dc.PAST_ONE_PASS:  # a second pass: thread 0 of workgroup 0 takes quad grid * 256 next
        assert route.grid(n) == dc.MAX_BLOCKS and route.quad_stride(route.grid(n)) == dc.ONE_PASS // 4 < quads
    assert route.first_quad(3, 17) == 3 * 256 + 17


def test_the_walk_stays_exact_at_the_largest_n(route):
    n = (1 << 62) - 1
    assert route.grid(n) == dc.MAX_BLOCKS and route.quad_elems((n + 3) // 4 - 1, n) == 3
    assert route.first_quad(dc.MAX_BLOCKS - 1, 255) == dc.ONE_PASS // 4 - 1 and route.quad_of(n - 1) == (1 << 60) - 1


def test_the_walk_as_a_program_under_the_sanitizers(tmp_path):
    exe = dc.build_walk(tmp_path, sanitize=True)
    res = subprocess.run([exe, dc.walk_input(str(tmp_path / "sizes.bin"))], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "bad 0" in res.stdout and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
