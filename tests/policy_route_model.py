"""The policy prior's routes from tdmpc2_amd/csrc/policy_route.h itself, compiled with g++ behind the C shim below (as
tests/pixel_route_model.py does for pixel_route.h).  The coverage counts run in C++ over the header's own work-item functions.
Used by tests/test_policy_route.py."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include "policy_route.h"
// kind, launches, then per launch x, y, threads, lds, R, in, out
extern "C" void route(int n, int in0, int mlp, int A, int maxw, int mode, long *out) {
    const PolRoute r = pol_route(n, in0, mlp, A, maxw, mode);
    out[0] = r.kind; out[1] = r.launches;
    for (int l = 0; l < POL_SPREAD_LAUNCHES; ++l) {
        long *o = out + 2 + 7 * l;
        o[0] = r.g[l].x; o[1] = r.g[l].y; o[2] = r.g[l].threads; o[3] = (long)r.g[l].lds; o[4] = r.g[l].R; o[5] = r.g[l].in;
        o[6] = r.g[l].out;
    }
}
// how often each (row, feature) of an [n, out] output is written by a launch of grid g (kind 0 GEMV, 1 row / norm, 2 head)
extern "C" void cover(int kind, int gx, int gy, int threads, int R, int n, int out, int *count) {
    for (int by = 0; by < gy; ++by)
        for (int bx = 0; bx < gx; ++bx)
            for (int t = 0; t < threads; ++t) {
                if (kind == 0) {
                    const PolItem it = pol_gemv_item(bx, by, R, t, n, out);
                    if (it.valid) count[(long)it.row * out + it.f] += 1;
                } else if (kind == 1) {
                    for (int u = 0; u < POL_MAX_PER_THREAD; ++u) {
                        const PolItem it = pol_row_item(bx, t, u, out);
                        if (it.valid) count[(long)it.row * out + it.f] += 1;
                    }
                } else {
                    const PolItem it = pol_head_item(bx, t, out);
                    if (it.valid) count[(long)it.row * out + it.f] += 1;
                }
            }
}
extern "C" long gemv_lds(int R, int in) { return (long)pol_gemv_lds(R, in); }
extern "C" long row_lds(int maxw) { return (long)pol_row_lds(maxw); }
extern "C" long ws_x(int max_envs, int mlp) { return (long)pol_ws_x_floats(max_envs, mlp); }
extern "C" long ws_y(int max_envs, int mlp, int A) { return (long)pol_ws_y_floats(max_envs, mlp, A); }
extern "C" int consts(int i) {
    const int v[] = {POL_THREADS, POL_MAX_PER_THREAD, POL_GEMV_THREADS, (int)POL_LDS_MAX, POL_HEAD_THREADS, POL_MAX_R, POL_SPREAD_LAUNCHES};
    return v[i];
}
"""
POL_ROW, POL_SPREAD = 0, 1
AUTO, FORCE_ROW, FORCE_SPREAD = 0, 1, 2


def build(tmpdir):
    src = os.path.join(str(tmpdir), "policy_route_shim.cpp")
    with open(src, "w") as f:
        f.write(SHIM)
    so = os.path.join(str(tmpdir), "libpolicy_route_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tdmpc2_amd", "csrc"), src, "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    ci = ctypes.c_int
    lib.route.argtypes = [ci, ci, ci, ci, ci, ci, ctypes.POINTER(ctypes.c_long)]
    lib.cover.argtypes = [ci, ci, ci, ci, ci, ci, ci, ctypes.POINTER(ctypes.c_int)]
    for f in (lib.gemv_lds, lib.row_lds, lib.ws_x, lib.ws_y):
        f.restype = ctypes.c_long
    return lib


def route(lib, n, in0, mlp, A, maxw, mode):
    out = (ctypes.c_long * (2 + 7 * 6))()
    lib.route(n, in0, mlp, A, maxw, mode, out)
    keys = ("x", "y", "threads", "lds", "R", "in", "out")
    g = [dict(zip(keys, out[2 + 7 * i:9 + 7 * i])) for i in range(6)]
    return {"kind": out[0], "launches": out[1], "grids": g[:out[1]]}


def cover(lib, kind, g, n, out):
    """count [n, out] of the writes of one launch"""
    count = np.zeros(n * out, dtype=np.int32)
    lib.cover(kind, g["x"], g["y"], g["threads"], g["R"], n, out, count.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    return count.reshape(n, out)
