"""CPU: tdmpc2_amd/csrc/pixel_grad_route.h compiled with g++ (tests/pixel_grad_route_model.py).  For n in {1, 2, 3, 17}, C in
{8, 24, 32, 40, 64}, cin in {1, 9, 16}: the decoded tiles cover every dW, db and da element exactly once; the tap and source maps are
the transposes of pixb_src, with the stride-2 validity of transposed taps; chunks are consecutive and whole but for the last; the
operand offsets of a chunk's rows name the forward's elements; the workspace regions follow each other.  Separately: the second
stage's order, size_t offsets past 2^32 at n = 2^20, the launch count, the refusals, and the same walk as a stand-alone program under
AddressSanitizer and UBSan."""
import ctypes as C
import subprocess

import pytest

from tests import pixel_grad_route_model as prm

NS, CS, CINS = (1, 2, 3, 17), (8, 24, 32, 40, 64), (1, 9, 16)
HW, KERNEL = (841, 169, 36, 16), (7, 5, 3, 3)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return prm.build(tmp_path_factory.mktemp("pixel_grad_route"))


@pytest.mark.parametrize("n", NS)
def test_walk(lib, n):
    for Cc in CS:
        for cin in CINS:
            assert lib.pg_walk(n, Cc, cin) == 0, (n, Cc, cin, "line", lib.pg_walk(n, Cc, cin))


def test_constants_and_launch_count(lib):
    out = (C.c_int * 5)()
    assert lib.pg_consts(out) == 5 and list(out) == [256, 32, 32, 128, 1 << 20]
    assert lib.pg_launches() == 12 and lib.pg_fwd_launches() == 5   # constants: n does not enter


def test_chunks_and_the_second_stage_order(lib):
    for n in NS + (256,):
        for l in range(4):
            rows = n * HW[l]
            chunks = lib.pg_chunks_c(l, n)
            assert chunks == -(-rows // 256)
            assert [lib.pg_chunk_rows_c(l, n, c) for c in (0, chunks - 1)] == [min(rows, 256), rows - 256 * (chunks - 1)]
            groups = lib.pg_fold_groups_c(chunks)
            assert groups == -(-chunks // 32)
            # groups are runs of 32 consecutive chunks in rising order
            assert [lib.pg_fold_group_c(c) for c in range(min(chunks, 70))] == [c // 32 for c in range(min(chunks, 70))]
    assert lib.pg_chunks_c(0, 256) == 841 and lib.pg_fold_groups_c(841) == 27
    for Cc in CS:
        for l in (1, 2, 3):
            K = Cc * KERNEL[l] ** 2
            assert lib.pg_da_steps_c(l, Cc) == -(-K // 2) and lib.pg_da_segs_c(l, Cc) == -(-K // 256)


def test_offsets_past_4g_at_a_million_images(lib):
    n, Cc, cin = 1 << 20, 64, 16
    off = 0
    for l in range(4):
        assert lib.pg_dy_off_c(l, n, Cc) == off
        off += n * Cc * HW[l]
    assert off > 1 << 32 and lib.pg_part_base_c(n, Cc) == off
    parts = max(-(-n * HW[l] // 256) * ((cin if l == 0 else Cc) * KERNEL[l] ** 2 + 1) * Cc for l in range(4))
    assert lib.pg_bwd_ws_floats_c(n, cin, Cc) == off + parts
    assert lib.pg_z_off_c(n, Cc) == n * Cc * (841 + 169 + 36) > 1 << 32
    assert lib.pg_acts_floats_c(n, Cc) == n * Cc * (841 + 169 + 36 + 16)
    M = cin * 49 + 1
    last = -(-n * 841 // 256) - 1
    assert lib.pg_part_off_c(M, Cc, last, M - 1, Cc - 1) == (last * M + M - 1) * Cc + Cc - 1 > 1 << 32
    assert lib.pg_dy_elem_c(0, Cc, n - 1, Cc - 1, 840) == n * Cc * 841 - 1 > 1 << 32
    w = 0
    for l in range(4):
        assert lib.pg_wp_off_c(l, cin, Cc) == w
        w += (cin if l == 0 else Cc) * KERNEL[l] ** 2 * Cc
    assert lib.pg_fwd_ws_floats_c(cin, Cc) == w


def test_refusals(lib):
    ok = dict(n=3, cin=9, Cc=32, dt=0, seed=0)
    call = lambda **kw: lib.pg_check_c(*{**ok, **kw}.values())  # noqa: E731
    assert call() == 0
    assert call(n=0) == 1 and call(n=-1) == 1 and call(n=(1 << 20) + 1) == 6 and call(n=1 << 20) == 0
    assert call(cin=0) == 2 and call(cin=17) == 2 and call(cin=16) == 0 and call(cin=1) == 0
    assert call(Cc=4) == 3 and call(Cc=68) == 3 and call(Cc=30) == 3 and call(Cc=8) == 0 and call(Cc=64) == 0
    assert call(dt=2) == 4 and call(dt=-1) == 4 and call(dt=1) == 0
    assert call(seed=2) == 5 and call(seed=1) == 0


def test_walk_under_the_sanitizers(tmp_path):
    exe = prm.build_walk(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])
