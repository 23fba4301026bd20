"""CPU test of the pixel encoder's geometry (tdmpc2_amd/csrc/pixel_route.h, compiled with g++: tests/pixel_route_model.py):
ShiftAug's resampling table against the PyTorch module, the coverage of every route's grid, its LDS and workspace, and the
argument checks of the pixel entry points (no GPU needed)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import pixel_route_model as prm

CUS = 256
GATE = 3e-5  # raw pixel levels


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return prm.build(tmp_path_factory.mktemp("pixel_route"))


def _shift_aug(x, shifts, monkeypatch):
    """tdmpc2_amd.layers.ShiftAug on the CPU with its randint draw replaced by the given (dx, dy) per image."""
    from tdmpc2_amd import layers

    s = torch.tensor(shifts, dtype=torch.float32).view(len(shifts), 1, 1, 2)
    with monkeypatch.context() as m:
        m.setattr(torch, "randint", lambda *a, **k: s.clone())
        return layers.ShiftAug()(x).numpy()


def test_shift_table_reproduces_shift_aug(lib, monkeypatch):
    tab = prm.shift_table(lib)
    shifts = [(dx, dy) for dx in range(7) for dy in range(7)]
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 256, (len(shifts), 9, 64, 64), generator=g).float()
    ref = _shift_aug(x, shifts, monkeypatch)
    worst = max(np.abs(prm.resample(tab, x[i].numpy(), dx, dy) - ref[i]).max() for i, (dx, dy) in enumerate(shifts))
    assert worst <= GATE, worst
    # negative control: the exact integer crop of the padded image is NOT what ShiftAug computes
    pad = np.pad(x.numpy(), ((0, 0), (0, 0), (3, 3), (3, 3)), mode="edge")
    crop = max(np.abs(pad[i, :, dy:dy + 64, dx:dx + 64] - ref[i]).max() for i, (dx, dy) in enumerate(shifts))
    assert crop > GATE, crop


def test_shift_table_neighbours(lib):
    lo, hi, w0, w1 = prm.shift_table(lib)
    assert lo.min() >= 0 and hi.max() <= 63
    # away from the border the source of index j under shift s is pixel j + s - 3 of the unpadded frame, give or take round-off
    for s in range(7):
        for j in range(64):
            src = j + s - 3
            if 0 <= src < 64:
                assert (lo[s, j] == src and w0[s, j] > 0.99) or (hi[s, j] == src and w1[s, j] > 0.99), (s, j)


@pytest.mark.parametrize("C", [8, 16, 32, 40, 48, 64])
def test_every_output_is_computed_once(lib, C):
    seen_routes = {}
    for E in range(1, 1025):
        r = prm.route(lib, E, C, CUS)
        g = r["grids"]
        if r["kind"] == prm.PIX_PER_IMAGE:
            assert r["launches"] == 1 and g[0]["x"] == E and g[0]["y"] == g[0]["z"] == 1
            assert g[0]["lds"] <= 160 * 1024
            key = ("image", g[0]["threads"])
        else:
            assert r["launches"] == 4 and all(gg["z"] == E and gg["lds"] == 0 for gg in g)
            key = ("spread",) + tuple((gg["x"], gg["y"], gg["threads"]) for gg in g)
        seen_routes.setdefault(key, r)
    for key, r in seen_routes.items():
        for layer in range(4):
            hw = lib.hw(layer)
            count = np.zeros((C, hw), dtype=np.int64)
            lanes = []  # (c0, p, valid) in lane order, for the SimNorm groups
            if r["kind"] == prm.PIX_SPREAD:
                gg = r["grids"][layer]
                for by in range(gg["y"]):
                    for bx in range(gg["x"]):
                        for t in range(gg["threads"]):
                            e, c0, p, valid = prm.item(lib, prm.PIX_SPREAD, layer, bx, by, 0, t)
                            assert e == 0
                            lanes.append((c0, p, valid))
                            if valid:
                                count[c0:c0 + 4, p] += 1
            else:
                wg = r["grids"][0]["threads"]
                n = lib.image_items(layer, C)
                assert n % 64 == 0 and wg % 64 == 0
                for i in range(n):
                    e, c0, p, valid = prm.item(lib, prm.PIX_PER_IMAGE, layer, C, 5, i)
                    assert e == 5
                    lanes.append((c0, p, valid))
                    if valid:
                        count[c0:c0 + 4, p] += 1
            assert (count == 1).all(), (key, layer)
            if layer == 3:  # SimNorm over 8 consecutive features = 8 aligned lanes of one channel group, all valid or none
                for k in range(0, len(lanes), 8):
                    grp = lanes[k:k + 8]
                    assert len({c for c, _, _ in grp}) == 1 and len({v for _, _, v in grp}) == 1
                    if grp[0][2]:
                        assert [p for _, p, _ in grp] == list(range(grp[0][1], grp[0][1] + 8)) and grp[0][1] % 8 == 0


@pytest.mark.parametrize("C", [8, 16, 32, 40, 48, 64])
def test_lds_and_workspace_bounds(lib, C):
    # spread route: layer outputs of one image lie inside its workspace slice, which bind sizes for max_envs images
    offs = [lib.ws_off(l, C) for l in range(3)]
    for l in range(3):
        assert offs[l] + C * lib.hw(l) <= (offs[l + 1] if l < 2 else lib.ws_floats(C))
    for max_envs in (1, 7, 256, 1024):
        assert lib.ws_bytes(max_envs, C) == max_envs * lib.ws_floats(C) * 4
    # per-image route: layer 1 writes beside what it reads (layer 0's region), layer 2 writes over layer 0's region while reading
    # layer 1's: no overlap; everything inside the LDS the launch asks for
    r = prm.route(lib, 1024, C, CUS)
    if r["kind"] == prm.PIX_PER_IMAGE:
        lds_f = r["grids"][0]["lds"] // 4
        reg = [(lib.image_lds_off(l, C), lib.image_lds_off(l, C) + C * lib.hw(l)) for l in range(3)]
        assert all(hi <= lds_f for _, hi in reg) and r["grids"][0]["lds"] <= 160 * 1024
        assert reg[0][1] <= reg[1][0] and reg[2][1] <= reg[1][0]
    else:
        assert C * (lib.hw(0) + lib.hw(1)) * 4 > 160 * 1024  # only when the LDS would not hold it


def test_route_threshold(lib):
    """Few images spread over the chip, many take one workgroup each: both sides are exercised by the GPU tests
    (tests/test_gpu_pixel_encoder.py: E = 1, 2, 7, 64 and 256 on 256 compute units)."""
    kinds = {E: prm.route(lib, E, 32, CUS)["kind"] for E in (1, 2, 7, 64, 256)}
    assert kinds[1] == kinds[2] == kinds[7] == kinds[64] == prm.PIX_SPREAD
    assert kinds[256] == prm.PIX_PER_IMAGE
    assert prm.route(lib, 1024, 64, CUS)["kind"] == prm.PIX_SPREAD  # 64 channels: layer outputs too large for LDS


def test_pixel_entry_points_reject_null_arguments():
    from tdmpc2_amd import native

    lib = ctypes.CDLL(native.lib_path())
    lib.tdmpc2_last_error.restype = ctypes.c_char_p
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    calls = {
        "tdmpc2_plan_bind_pixel_encoder": ([vp, i32, vp, vp, i32, i32, i32, vp], [None, 0, None, None, 32, 9, 7, None]),
        "tdmpc2_plan_encode_pix": ([vp, i32, vp, i32, i32, vp, vp, vp], [None, 1, None, 0, 9, None, None, None]),
        "tdmpc2_plan_run_pix": ([vp, i32, vp, i32, i32, vp, vp, vp, vp, i32, vp, ctypes.c_uint64, vp, vp],
                                [None, 1, None, 0, 9, None, None, None, None, 0, None, 0, None, None]),
    }
    for name, (argtypes, args) in calls.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, i32
        assert fn(*args) == 1, name  # TDMPC2_ERR_INVALID
        assert b"null" in lib.tdmpc2_last_error(), name
