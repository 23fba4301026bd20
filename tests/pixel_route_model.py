"""The pixel encoder's routes and ShiftAug table from tdmpc2_amd/csrc/pixel_route.h itself, compiled with g++ behind the C shim
below (as tests/layer_route_model.py does for layer_route.h).  Used by tests/test_pixel_route.py."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include "pixel_route.h"
extern "C" void shift_table(int *lo, int *hi, float *w0, float *w1) {
    static PixTap t[PIX_SHIFTS * PIX_IN];
    pix_shift_table(t);
    for (int i = 0; i < PIX_SHIFTS * PIX_IN; ++i) { lo[i] = t[i].lo; hi[i] = t[i].hi; w0[i] = t[i].w0; w1[i] = t[i].w1; }
}
// kind, launches, then per launch x, y, z, threads, lds
extern "C" void route(int E, int C, int cus, long *out) {
    const PixRoute r = pix_route(E, C, cus);
    out[0] = r.kind; out[1] = r.launches;
    for (int l = 0; l < PIX_LAYERS; ++l) {
        long *o = out + 2 + 5 * l;
        o[0] = r.g[l].x; o[1] = r.g[l].y; o[2] = r.g[l].z; o[3] = r.g[l].threads; o[4] = (long)r.g[l].lds;
    }
}
extern "C" void spread_item(int l, int bx, int by, int bz, int t, int *out) {
    const PixItem it = pix_spread_item(l, bx, by, bz, t);
    out[0] = it.e; out[1] = it.c0; out[2] = it.p; out[3] = it.valid;
}
extern "C" int image_items(int l, int C) { return pix_image_items(l, C); }
extern "C" void image_item(int l, int C, int e, int i, int *out) {
    const PixItem it = pix_image_item(l, C, e, i);
    out[0] = it.e; out[1] = it.c0; out[2] = it.p; out[3] = it.valid;
}
extern "C" int hw(int l) { return pix_hw(l); }
extern "C" int out_side(int l) { return pix_out(l); }
extern "C" long ws_bytes(int max_envs, int C) { return (long)pix_ws_bytes(max_envs, C); }
extern "C" long ws_off(int l, int C) { return (long)pix_ws_off(l, C); }
extern "C" long ws_floats(int C) { return (long)pix_ws_floats(C); }
extern "C" int image_lds_off(int l, int C) { return pix_image_lds_off(l, C); }
extern "C" int consts(int i) {
    const int v[] = {PIX_CO, PIX_SPREAD_WG, PIX_IMAGE_WG, (int)PIX_LDS_MAX, PIX_LAYERS, PIX_SHIFTS};
    return v[i];
}
"""
PIX_SPREAD, PIX_PER_IMAGE = 0, 1


def build(tmpdir):
    src = os.path.join(str(tmpdir), "pixel_route_shim.cpp")
    with open(src, "w") as f:
        f.write(SHIM)
    so = os.path.join(str(tmpdir), "libpixel_route_shim.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tdmpc2_amd", "csrc"), src, "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    ci, pl, pi = ctypes.c_int, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_int)
    lib.route.argtypes = [ci, ci, ci, pl]
    lib.spread_item.argtypes = [ci, ci, ci, ci, ci, pi]
    lib.image_item.argtypes = [ci, ci, ci, ci, pi]
    lib.ws_bytes.restype = lib.ws_off.restype = lib.ws_floats.restype = ctypes.c_long
    return lib


def shift_table(lib):
    """(lo, hi, w0, w1), each [7, 64]: source indices of the unpadded image and bilinear weights per (shift, output index)."""
    n = 7 * 64
    lo, hi = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    w0, w1 = (ctypes.c_float * n)(), (ctypes.c_float * n)()
    lib.shift_table(lo, hi, w0, w1)
    return tuple(np.ctypeslib.as_array(a).reshape(7, 64).copy() for a in (lo, hi, w0, w1))


def resample(tab, img, dx, dy):
    """ShiftAug of one image [C, 64, 64] (raw levels) through the table, in numpy fp32 with grid_sample's product order."""
    lo, hi, w0, w1 = tab
    img = img.astype(np.float32)
    ry0, ry1, wy0, wy1 = lo[dy], hi[dy], w0[dy], w1[dy]
    cx0, cx1, wx0, wx1 = lo[dx], hi[dx], w0[dx], w1[dx]
    out = np.zeros_like(img)
    for (rr, wy), (cc, wx) in [((ry0, wy0), (cx0, wx0)), ((ry0, wy0), (cx1, wx1)), ((ry1, wy1), (cx0, wx0)), ((ry1, wy1), (cx1, wx1))]:
        out = out + img[:, rr][:, :, cc] * (wy[:, None] * wx[None, :]).astype(np.float32)
    return out


def route(lib, E, C, cus):
    out = (ctypes.c_long * 22)()
    lib.route(E, C, cus, out)
    g = [dict(zip(("x", "y", "z", "threads", "lds"), out[2 + 5 * i:7 + 5 * i])) for i in range(4)]
    return {"kind": out[0], "launches": out[1], "grids": g[:out[1]]}


def item(lib, kind, *args):
    o = (ctypes.c_int * 4)()
    (lib.spread_item if kind == PIX_SPREAD else lib.image_item)(*args, o)
    return tuple(o)
