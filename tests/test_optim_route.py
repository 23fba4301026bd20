"""CPU: tdmpc2_amd/csrc/optim_route.h, built with the host compiler (tests/optim_common.build_route), against the Python model of
tests/optim_common.py: offsets padded to 4 floats; the chunks cover every arena quad exactly once at the case table and at totals
past 2^32 elements; every quad finds its segment through chunk_seg and the search; the norm's order is the published one, with
its longest addition chain D = 8 + 6 + 3 + ceil(chunks / 256) + 6 + 3; the device block; the refusals.  The same walk runs once as
a stand-alone program (oc.build_walk: the program that is also built with AddressSanitizer and UBSan, outside the suite)."""
import ctypes
import subprocess

import numpy as np
import pytest

from tests import optim_common as oc


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    return oc.build_route(tmp_path_factory.mktemp("optroute"))


def _i64(v):
    return (ctypes.c_int64 * len(v))(*v)


def test_constants_match_the_python_model(route):
    out = (ctypes.c_int32 * 8)()
    route.constants(out)
    c = dict(zip(oc.CONSTANT_KEYS, [int(v) for v in out]))
    assert (c["THREADS"], c["QUADS_PER_THREAD"], c["CHUNK"]) == (oc.THREADS, oc.QUADS_PER_THREAD, oc.CHUNK)
    assert c["WAVES"] * 64 == c["THREADS"] and c["QUAD"] == 4 and c["CHUNK_QUADS"] * 4 == c["CHUNK"] and c["SEG_BYTES"] == 32


@pytest.mark.parametrize("case", oc.cases(), ids=lambda c: c["name"])
def test_offsets_are_padded_to_four_floats(route, case):
    counts = case["counts"]
    offs = (ctypes.c_int64 * len(counts))()
    total = route.layout(len(counts), _i64(counts), offs)
    assert (list(offs), total) == oc.layout(counts)
    assert all(o % 4 == 0 for o in offs) and total % 4 == 0
    assert all(b - a == -(-c // 4) * 4 for a, b, c in zip(offs, list(offs)[1:] + [total], counts))


def _cover(route, arena_floats, chunk_ids):
    quads = arena_floats // 4
    for c in chunk_ids:
        marks = np.zeros(oc.CHUNK // 4, np.uint8)
        assert route.cover_chunk(c, quads, marks.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))) == 0
        live = np.arange(c * (oc.CHUNK // 4), (c + 1) * (oc.CHUNK // 4)) < quads
        assert (marks == live).all(), c


@pytest.mark.parametrize("case", oc.cases(), ids=lambda c: c["name"])
def test_chunks_cover_every_quad_once_and_find_its_segment(route, case):
    counts = case["counts"]
    offs, total = oc.layout(counts)
    n = route.chunks(total)
    assert n == -(-total // oc.CHUNK)
    _cover(route, total, range(n))  # contiguous ranges of one chunk each: together every quad once
    ref = np.repeat(np.arange(len(counts), dtype=np.int32), [-(-c // 4) for c in counts])
    assert ref.size == total // 4
    assert route.seg_walk(len(counts), _i64(offs), total, ref.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0


def test_chunks_past_2_32_elements(route):
    for total in ((1 << 32) + 8, (1 << 32) + 3 * oc.CHUNK + 8, (1 << 40) + 4):
        n = route.chunks(total)
        assert n == -(-total // oc.CHUNK) and n * oc.CHUNK >= total > (n - 1) * oc.CHUNK
        _cover(route, total, [0, 1, (1 << 32) // oc.CHUNK - 1, (1 << 32) // oc.CHUNK, n - 2, n - 1])
    offs = (ctypes.c_int64 * 3)()
    assert route.layout(3, _i64([(1 << 33) + 1, 5, 7]), offs) == (1 << 33) + 4 + 8 + 8 and list(offs) == [0, (1 << 33) + 4, (1 << 33) + 12]


def test_norm_order_is_the_published_one(route):
    """The Python model of the order (oc.norm_model) holds the order the header publishes: its depth is the header's D, and on
    data where the order shows -- one huge square among small ones -- it differs from other orders yet keeps the derived bound."""
    for case in oc.cases():
        _, total = oc.layout(case["counts"])
        assert route.depth(total) == oc.norm_depth(total), case["name"]
    assert oc.norm_depth(2048) == 8 + 6 + 3 + 1 + 6 + 3 and oc.norm_depth((1 << 20) + 4) == 8 + 6 + 3 + 3 + 6 + 3
    rng = np.random.default_rng(5)
    for case in oc.cases():
        arena = oc.to_arena(oc.make_values(case["counts"], rng.integers(1 << 30)), case["counts"])
        norm, partial = oc.norm_model(arena)
        assert partial.size == route.chunks(arena.size)
        n64 = float(np.sqrt(np.sum(arena.astype(np.float64) ** 2)))
        assert abs(float(norm) - n64) <= (oc.norm_depth(arena.size) + 2) * oc.U * n64
    # quads of one thread are 256 quads apart: thread 0 of chunk 0 sums elements 0..3 and 1024..1027, in that order
    arena = np.zeros(2048, np.float32)
    arena[[0, 1, 1024]] = (2.0 ** 12, 1.0, 1.0)
    assert float(oc.norm_model(arena)[0]) ** 2 == 2.0 ** 24  # (2^24 + 1) + 1 rounds twice to even; 2^24 + (1 + 1) would not


def test_device_block_and_refusals(route):
    out = (ctypes.c_uint64 * 7)()
    route.block(300, 3, 513, out)
    b = dict(zip(oc.BLOCK_KEYS, [int(v) for v in out]))
    up = lambda x: -(-x // 256) * 256  # noqa: E731
    assert b["segs_off"] == 0 and b["chunk_seg_off"] == up(300 * 32) and b["lr_off"] == b["chunk_seg_off"] + up(514 * 4)
    assert b["state_off"] == b["lr_off"] + 256 and b["ss_off"] == b["state_off"] + 40
    assert b["partial_off"] == b["state_off"] + 256 and b["bytes"] == b["partial_off"] + up(513 * 4)
    nan = float("nan")
    assert route.check_hyper(0.9, 0.999, 1e-8, 1.0) == 0 and route.check_hyper(0.0, 0.0, 1e-30, 1e-30) == 0
    for bad in ((1.0, 0.9, 1e-8, 1.0), (-0.1, 0.9, 1e-8, 1.0), (0.9, 1.0, 1e-8, 1.0), (0.9, -1.0, 1e-8, 1.0), (0.9, 0.9, 0.0, 1.0),
                (0.9, 0.9, -1.0, 1.0), (0.9, 0.9, 1e-8, 0.0), (0.9, 0.9, 1e-8, -2.0), (nan, 0.9, 1e-8, 1.0), (0.9, nan, 1e-8, 1.0),
                (0.9, 0.9, nan, 1.0), (0.9, 0.9, 1e-8, nan)):
        assert route.check_hyper(*bad) != 0, bad
    assert route.check_seg(1, 0, 1, 1) == 0 and route.check_seg(0, 0, 1, 1) != 0 and route.check_seg(-3, 0, 1, 1) != 0
    assert route.check_seg(1, 1, 1, 1) != 0 and route.check_seg(1, -1, 1, 1) != 0 and route.check_seg(1, 0, 1, 0) != 0


def test_route_walk_as_a_stand_alone_program(tmp_path):
    """Its own main: layout, coverage and the segment search over the case table and past 2^32 elements."""
    exe = oc.build_walk(tmp_path)
    run = subprocess.run([exe, oc.walk_input(str(tmp_path / "cases.bin"))], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "bad 0" in run.stdout
