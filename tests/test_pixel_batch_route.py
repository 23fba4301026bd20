"""CPU: the pixel encoder's batch route as tdmpc2_amd/csrc/pixel_batch_route.h decides it (compiled with g++:
tests/pixel_batch_route_model.py).  Every output element is stored by exactly one accumulator register and padding rows / columns
never are; a numpy GEMM driven only by the header's k-map and source-element map is torch's conv2d exactly (integer data); the
kernel's address split and layer 0's staging agree with that map; the passes partition a call; the LDS fits; and the two new symbols
are declared, bound, documented and refuse bad arguments before the device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pixel_batch_route_model as pbm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = (8, 16, 24, 32, 40, 48, 56, 64)
KERNEL, STRIDE = (7, 5, 3, 3), (2, 2, 2, 1)
NEW = ("tdmpc2_plan_pix_batch_reserve", "tdmpc2_plan_encode_pix_batch")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return pbm.build(tmp_path_factory.mktemp("pixel_batch_route"))


def test_geometry_and_accumulator_layout(lib):
    c = pbm.consts(lib)
    assert c["TILE"] == 32 and c["KSTEP"] == 2 and c["ACC"] == 16 and c["THREADS"] == 64 * c["WAVES"] and c["WG_ROWS"] == 32 * c["WAVES"]
    assert c["WG_ROWS"] < lib.hw(0)  # a workgroup of layer 0 touches at most two images (the staging's assumption)
    assert [lib.hw(l) for l in range(4)] == [841, 169, 36, 16]
    # the 32 x 32 C/D layout: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5); every tile element once
    seen = set()
    for lane in range(64):
        for i in range(16):
            o = (ctypes.c_int * 2)()
            lib.acc_elem(lane, i, o)
            assert tuple(o) == ((i & 3) + 8 * (i >> 2) + 4 * (lane >> 5), lane & 31)
            seen.add(tuple(o))
    assert len(seen) == 32 * 32
    # layer 3: a SimNorm group (8 consecutive pixels of one channel = rows 8 g .. 8 g + 7 of a column) is registers 4 g .. 4 g + 3 of
    # lanes c and c + 32
    for g in range(4):
        rows = set()
        for lane in (5, 37):
            for i in range(4 * g, 4 * g + 4):
                o = (ctypes.c_int * 2)()
                lib.acc_elem(lane, i, o)
                assert o[1] == 5
                rows.add(o[0])
        assert rows == set(range(8 * g, 8 * g + 8))


@pytest.mark.parametrize("C", CHANNELS)
def test_every_element_is_stored_exactly_once(lib, C):
    for l in range(4):
        for n in (1, 2, 3, 5):
            counts, outside = pbm.coverage(lib, l, n, C, 9)
            assert outside == 0, (l, n, C)                       # padding rows and columns are never stored
            assert counts.min() == 1 and counts.max() == 1, (l, n, C)  # every (image, pixel, channel) by exactly one item
            g = pbm.grid(lib, l, n, C, 9)
            assert g["x"] == -(-n * lib.hw(l) // pbm.consts(lib)["WG_ROWS"]) and g["y"] == g["z"] == 1 and g["threads"] == pbm.consts(lib)["THREADS"]
            assert lib.col_tiles(C) == -(-C // 32)


@pytest.mark.parametrize("cin", [1, 9, 16])
@pytest.mark.parametrize("l", [0, 1, 2, 3])
def test_k_map_reproduces_conv2d_exactly(lib, l, cin):
    n = 3  # tiles straddle images on every layer
    Cs = (8, 40) if l == 0 else (8, 24)
    for C in Cs:
        cin_l = cin if l == 0 else C
        g = torch.Generator().manual_seed(100 * l + cin + C)
        s = lib.side(l)
        x = torch.randint(-3, 4, (n, cin_l, s, s), generator=g).float()
        W = torch.randint(-3, 4, (C, cin_l, KERNEL[l], KERNEL[l]), generator=g).float()
        want = F.conv2d(x, W, stride=STRIDE[l])  # [n, C, o, o]
        wp = W.permute(1, 2, 3, 0).contiguous().reshape(-1).numpy()  # k_pix_pack's [cin][ky][kx][C]
        idx, woff = pbm.gather(lib, l, n, cin_l, C)
        K, kp = lib.k_true(l, cin_l), lib.k_pad(l, cin_l)
        assert K == cin_l * KERNEL[l] ** 2 and kp >= K and kp % (2 * pbm.consts(lib)["KGROUP"]) == 0 and kp - K < 2 * pbm.consts(lib)["KGROUP"]
        assert (idx[:, K:] == -1).all() and (woff[K:] == -1).all() and (idx[:, :K] >= 0).all() and (woff[:K] >= 0).all()
        assert sorted(woff[:K].tolist()) == [r * C for r in range(K)]  # every row of the bound weights once
        A = np.where(idx >= 0, x.reshape(-1).numpy()[np.maximum(idx, 0)], np.float32(0))          # padding k: a zero input
        Bm = np.where(woff[:, None] >= 0, wp[np.maximum(woff, 0)[:, None] + np.arange(C)[None, :]], np.float32(0))  # times a zero weight
        D = (A.astype(np.float32) @ Bm.astype(np.float32)).reshape(n, lib.hw(l), C)  # row r = image r / hw, pixel r % hw
        assert np.array_equal(D.transpose(0, 2, 1), want.reshape(n, C, -1).numpy()), (l, cin, C)
        assert lib.address_errors(l, n, cin_l) == 0


def test_k_order_follows_the_scalar_routes(lib):
    # layer 0: (ky, kx) outside, input channel inside; layers 1..3: input channel outside, (ky, kx) inside (k_pix_spread's loops)
    assert [pbm.k_decode(lib, 0, 9, k) for k in (0, 1, 8, 9, 9 * 7, 440)] == [(0, 0, 0), (1, 0, 0), (8, 0, 0), (0, 0, 1), (0, 1, 0), (8, 6, 6)]
    assert [pbm.k_decode(lib, 1, 32, k) for k in (0, 1, 5, 25, 799)] == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (31, 4, 4)]
    assert [pbm.k_decode(lib, 3, 8, k) for k in (0, 2, 3, 9, 71)] == [(0, 0, 0), (0, 0, 2), (0, 1, 0), (1, 0, 0), (7, 2, 2)]


def test_layer0_staging_for_every_workgroup(lib):
    for n in (1, 2, 3, 5):
        for cin in (1, 16):
            assert lib.address_errors(0, n, cin) == 0, (n, cin)


def test_layer0_staging_fits_its_slots_at_every_offset(lib):
    # a workgroup's first row is 256 b, so its offset inside an image is 256 b mod 841: any of [0, 841).  The rows it stages are
    # derived here from the geometry alone (output row oy reads input rows 2 oy .. 2 oy + 6) and must be what the header stages,
    # within PIXB_L0_SLOTS and within the frame.
    c = pbm.consts(lib)
    worst = 0
    for r0 in range(lib.hw(0)):
        r1 = r0 + c["WG_ROWS"] - 1
        oy0, oy1 = r0 // 29, r1 // 29  # output rows, counted through the second image
        nA, nB, yA0, yA1, yB1 = pbm.stage(lib, r0)
        if oy1 < 29:
            assert (yA0, yA1, nB) == (2 * oy0, 2 * oy1 + 6, 0), r0
        else:
            assert (yA0, yA1, yB1) == (2 * oy0, 2 * 28 + 6, 2 * (oy1 - 29) + 6), r0
        assert nA == yA1 - yA0 + 1 and yA1 <= 63 and yB1 <= 63 and nA >= 7 and nB >= 0, r0
        worst = max(worst, nA + nB)
    assert worst <= c["L0_SLOTS"] == 30, worst
    assert worst == c["L0_SLOTS"]  # the bound is reached: no slot is wasted


@pytest.mark.parametrize("n,chunk", [(1, 1), (4, 4), (5, 4), (9, 4), (3, 256)])
def test_passes_partition_the_call(lib, n, chunk):
    k = lib.chunks(n, chunk)
    assert k == -(-n // chunk)
    at = 0
    for i in range(k):
        assert lib.chunk_begin(i, chunk) == at
        cnt = lib.chunk_count(n, chunk, i)
        assert 1 <= cnt <= chunk
        at += cnt
    assert at == n
    assert lib.ws_bytes(chunk, 32) == chunk * 32 * (841 + 169 + 36) * 4


def test_lds_fits_for_every_accepted_shape(lib):
    c = pbm.consts(lib)
    worst = 0
    for C in CHANNELS:
        for cin in range(1, 17):
            for l in range(4):
                b = lib.lds(l, C, cin)
                kp = lib.k_pad(l, cin if l == 0 else C)
                assert b == kp * 8 + (cin * c["L0_SLOTS"] * 64 * 4 if l == 0 else 0)
                assert b <= c["LDS_MAX"] == 160 * 1024, (l, C, cin, b)
                assert pbm.grid(lib, l, 2, C, cin)["lds"] == b
                worst = max(worst, b)
    assert worst == lib.lds(0, 64, 16)


def test_symbols_declared_bound_and_documented():
    from tdmpc2_amd import native

    hdr = open(os.path.join(ROOT, "include", "tdmpc2_plan.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"#define TDMPC2_PLAN_ABI_VERSION 14\b", hdr) and native.ABI_VERSION == 14  # additions to ABI 14
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, hdr) and sym in native.ABI_SYMBOLS and f"`{sym}" in doc, sym
    assert "reserve_pix_batch" in doc and "encode_pix_batch" in doc
    assert callable(native.NativePlanner.reserve_pix_batch) and callable(native.NativePlanner.encode_pix_batch)


def test_refusals_before_the_device():
    from tdmpc2_amd import native

    so = ctypes.CDLL(native.lib_path())
    so.tdmpc2_last_error.restype = ctypes.c_char_p
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    so.tdmpc2_plan_pix_batch_reserve.argtypes = [vp, i32, vp]
    so.tdmpc2_plan_encode_pix_batch.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp]
    INVALID = 1
    fake = vp(1)  # never dereferenced: the arguments below are refused first
    assert so.tdmpc2_plan_pix_batch_reserve(None, 4, None) == INVALID and b"null" in so.tdmpc2_last_error()
    assert so.tdmpc2_plan_pix_batch_reserve(fake, 0, None) == INVALID and b"chunk_images" in so.tdmpc2_last_error()
    assert so.tdmpc2_plan_pix_batch_reserve(fake, -3, None) == INVALID
    assert so.tdmpc2_plan_encode_pix_batch(None, 1, fake, 0, 9, fake, fake, None) == INVALID and b"null" in so.tdmpc2_last_error()
    for args in ((fake, 1, None, 0, 9, fake, fake), (fake, 1, fake, 0, 9, None, fake), (fake, 1, fake, 0, 9, fake, None)):
        assert so.tdmpc2_plan_encode_pix_batch(*args, None) == INVALID and b"null" in so.tdmpc2_last_error()
    assert so.tdmpc2_plan_encode_pix_batch(fake, 0, fake, 0, 9, fake, fake, None) == INVALID and b"n_images" in so.tdmpc2_last_error()
    assert so.tdmpc2_plan_encode_pix_batch(fake, 2, fake, 2, 9, fake, fake, None) == INVALID and b"obs_dtype" in so.tdmpc2_last_error()
    assert so.tdmpc2_plan_encode_pix_batch(fake, 2, fake, 0, 17, fake, fake, None) == INVALID and b"input channels" in so.tdmpc2_last_error()
