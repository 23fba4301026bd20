"""CPU: the replay buffer's arithmetic (tdmpc2_amd/csrc/buffer_route.h, compiled with the host compiler) against the plain-Python
restatement of tests/buffer_common.py: table evolution, the two draws, access widths and grids, 64-bit offsets, and that the
decoded workgroups cover every byte of every output row exactly once.  Plus the sampler's distribution, on the restatement (the
GPU is compared with it bit for bit in tests/test_gpu_buffer.py, so it needs no statistical test of its own)."""
import ctypes
import math

import numpy as np
import pytest

from tests import buffer_common as bc


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return bc.build_route(tmp_path_factory.mktemp("buffer_route"))


def _ref(cap, S):
    return bc.RefBuffer(cap, S, [(1, 0, S)])


def _rows(T):
    return [np.zeros((T, 1), np.uint8)]


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("cap_of", [lambda S: S, lambda S: S + 1, lambda S: 10, lambda S: 64])
def test_table_evolution_over_random_adds(lib, S, cap_of):
    cap = cap_of(S)
    rng = np.random.default_rng(1000 * S + cap)
    for trial in range(20):
        ring, ref = bc.RouteRing(lib, cap, S), _ref(cap, S)
        assert ring.tcap == cap // S + 1 == lib.table_cap(cap, S)
        for step in range(60):
            T = int(rng.integers(1, cap + 1)) if rng.random() < 0.7 else int(rng.integers(1, min(cap, S + 1) + 1))
            before = ring.state()["count"]
            u = ring.write(1, T)
            ref.add(_rows(T))
            st = ring.state()
            want = ref.eligible()
            assert ring.mirror_entries() == want, (cap, S, trial, step, T)
            assert ring.device_entries() == want, (cap, S, trial, step, T)  # what the update kernel's by-value numbers produce
            assert (st["cursor"], st["floor"], st["num_eps"], st["count"]) == (ref.cursor, ref.floor, ref.num_eps, len(want))
            assert st["count"] <= cap // S < st["tcap"] and st["head"] < st["tcap"]
            # O(entries touched): the popped ones, the survivor looked at, the pushed one -- never the whole table
            assert u["touched"] <= (before - (st["count"] - u["n_push"])) + 1 + u["n_push"]
            # the copy: at most two pieces, in bounds, covering the episode in order
            assert u["pieces"] in (1, 2) and u["skip"] == 0 and u["copy"] == T
            assert u["src0"] == 0 and u["dst0"] == (ref.cursor - T) % cap and u["dst0"] + u["n0"] <= cap
            if u["pieces"] == 2:
                assert (u["src1"], u["dst1"], u["n0"] + u["n1"]) == (u["n0"], 0, T) and u["dst0"] + u["n0"] == cap


def test_an_episode_that_loses_its_front_stays_a_shorter_trajectory(lib):
    ring = bc.RouteRing(lib, 10, 4)
    ring.write(1, 6)
    u = ring.write(1, 6)  # wraps physically; the first episode keeps steps 2..5: exactly one start
    assert ring.device_entries() == [(2, 4), (6, 6)] and u["shrink"] == 1 and u["pieces"] == 2
    ring.write(1, 1)      # one more step: the first episode has 3 < S live steps and is popped
    assert ring.device_entries() == [(6, 6)]
    ring.write(1, 3)      # shorter than S: occupies storage, counts, is never entered
    assert ring.device_entries() == [(6, 6)] and ring.state()["num_eps"] == 4
    ring.write(1, 10)     # T == capacity evicts everything else
    assert ring.device_entries() == [(16, 10)]


@pytest.mark.parametrize("cap,S", [(4, 4), (5, 4), (10, 4), (64, 4), (64, 2), (7, 3)])
def test_bulk_load_equals_single_adds(lib, cap, S):
    rng = np.random.default_rng(cap * 31 + S)
    for trial in range(40):
        a, b = bc.RouteRing(lib, cap, S), bc.RouteRing(lib, cap, S)
        for _ in range(int(rng.integers(0, 4))):  # some history first
            T = int(rng.integers(1, cap + 1))
            a.write(1, T)
            b.write(1, T)
        N, T = int(rng.integers(1, 40)), int(rng.integers(1, cap + 1))
        cursor = a.state()["cursor"]
        u = a.write(N, T)
        for _ in range(N):
            b.write(1, T)
        assert a.state() == b.state(), (cap, S, trial, N, T)  # head position included
        assert a.device_entries() == b.device_entries() == a.mirror_entries()
        # only steps that stay live are copied: the last min(N T, capacity), to where single adds would have left them
        assert u["skip"] == max(0, N * T - cap) and u["copy"] == N * T - u["skip"]
        assert u["dst0"] == (cursor + u["skip"]) % cap and u["n0"] + u["n1"] == u["copy"]


def test_draw_mappings_never_return_n(lib):
    for n in (1, 2, 37, 2 ** 31):
        for r in (0, 1, 2 ** 32 - 1):
            want = (r * n) >> 32
            assert lib.draw_episode(r, n) == want == int(bc.draw(r, n)) and want < n
            S = 4
            if n + S - 1 < 2 ** 32:
                assert lib.draw_start(r, n + S - 1, S) == want  # len - S + 1 == n starts
        assert lib.draw_episode(2 ** 32 - 1, n) == n - 1 and lib.draw_episode(0, n) == 0
    rng = np.random.default_rng(5)
    for r, n in zip(rng.integers(0, 2 ** 32, 2000), rng.integers(1, 2 ** 32, 2000)):
        assert lib.draw_episode(int(r), int(n)) == (int(r) * int(n)) >> 32 < int(n)


ROW_BYTES = (1, 4, 12, 16, 20, 96, 892, 36864)


def test_access_width_and_grid(lib):
    c = (ctypes.c_uint32 * 5)()
    lib.constants(c)
    threads, chunk_units, pack_below = c[0], c[1], c[2]
    for rb in ROW_BYTES:
        for bits, align in ((0x7f00, 16), (0x7f08, 8), (0x7f04, 4), (0x7f02, 2), (0x7f01, 1)):
            want = 16 if (rb % 16 == 0 and align >= 16) else 4 if (rb % 4 == 0 and align >= 4) else 1
            assert lib.access_width(rb, bits) == want, (rb, bits)
            for rows in (1, 8, 257, 4 * 257):
                g = (ctypes.c_uint32 * 5)()
                lib.field_grid(rb, bits, rows, g)
                width, units, rpw, chunks, blocks = g
                assert width == want and units * width == rb
                if rb < pack_below:  # several rows to a workgroup: a 4-byte reward row does not cost a workgroup
                    assert rpw == max(1, threads // units) and blocks == -(-rows // rpw)
                    if rb == 4 and want == 4:
                        assert rpw == threads
                else:                # a pixel row is split over several workgroups
                    assert rpw == 0 and chunks == -(-units // chunk_units) and blocks == rows * chunks
                    if rb == 36864 and want == 16:
                        assert chunks == 3


def test_decoded_workgroups_cover_every_row_exactly_once(lib):
    for rb in ROW_BYTES:
        for bits in (0x1000, 0x1004, 0x1001):
            for rows in (1, 8, 257):
                g = (ctypes.c_uint32 * 5)()
                lib.field_grid(rb, bits, rows, g)
                width, units, blocks = g[0], g[1], g[4]
                cover = np.zeros((rows, units), np.int32)
                for blk in range(blocks):
                    w = (ctypes.c_uint64 * 4)()
                    lib.decode(rb, bits, rows, blk, w)
                    row0, nrows, unit0, nunits = (int(v) for v in w)
                    assert nrows >= 1 and nunits >= 1 and row0 + nrows <= rows and unit0 + nunits <= units
                    cover[row0:row0 + nrows, unit0:unit0 + nunits] += 1
                assert (cover == 1).all(), (rb, bits, rows)


def test_offsets_are_64_bit(lib):
    cap, rbs = 550_450_000, (156, 24, 4, 8)
    base = (ctypes.c_uint64 * 4)()
    total = lib.field_bases(cap, 4, (ctypes.c_uint32 * 4)(*rbs), base)
    off, want = 0, []
    for rb in rbs:
        want.append(off)
        off = -(-(off + cap * rb) // 256) * 256
    assert list(base) == want and total == off and base[1] > 2 ** 32
    assert lib.offset(base[0], cap - 1, 156) == (cap - 1) * 156 > 2 ** 32
    assert lib.offset(base[3], cap - 1, 8) == want[3] + (cap - 1) * 8 > 2 ** 36
    for f in range(3):  # the regions do not overlap
        assert lib.offset(base[f], cap - 1, rbs[f]) + rbs[f] <= base[f + 1]


def test_philox_restatement_matches_the_published_vectors():
    """Random123's known-answer tests for philox4x32-10."""
    z = bc.philox4x32_10((0, 0, 0, 0), (0, 0))
    assert [int(v) for v in z] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = bc.philox4x32_10((M := 0xffffffff, M, M, M), (M, M))
    assert [int(v) for v in f] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    p = bc.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))
    assert [int(v) for v in p] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_sampling_distribution():
    """Episodes of S, 2 S and 40 steps, S = 4, 16 384 draws under a fixed seed: the episode counts against 1/3 each and the starts
    inside the 40-step episode against uniform over 37, each chi-square below its 1 - 1e-6 quantile."""
    S, n = 4, 16384
    ref = bc.RefBuffer(64, S, [(1, 0, S)])
    for T in (S, 2 * S, 40):
        ref.add(_rows(T))
    assert ref.eligible() == [(0, 4), (4, 8), (12, 40)]
    start, e = ref.starts(n, seed=20240607, call=0)
    counts = np.bincount(e, minlength=3)
    chi_e = float(((counts - n / 3) ** 2 / (n / 3)).sum())
    bound_e = -2.0 * math.log(1e-6)  # chi-square with 2 degrees of freedom: the survival function is exp(-x / 2)
    assert abs(bc.chi2_sf_even(bound_e, 2) - 1e-6) < 1e-12
    assert chi_e < bound_e, (counts, chi_e)
    s40 = start[e == 2] - 12
    assert s40.min() >= 0 and s40.max() <= 36
    c40 = np.bincount(s40, minlength=37)
    exp = len(s40) / 37
    chi_s = float(((c40 - exp) ** 2 / exp).sum())
    bound_s = bc.chi2_quantile_even(1e-6, 36)
    assert 85.0 < bound_s < 95.0 and abs(bc.chi2_sf_even(bound_s, 36) - 1e-6) < 1e-9  # (about 90: 36 + 5.4 standard deviations)
    assert chi_s < bound_s, (c40, chi_s)
    # the other episodes' starts stay inside them
    assert set(start[e == 0]) == {0} and set(start[e == 1]) <= set(range(4, 9)) and len(set(start[e == 1])) == 5
