"""The pixel encoder's batch route from tdmpc2_amd/csrc/pixel_batch_route.h itself, compiled with g++ behind the C shim below (as
tests/pixel_route_model.py does for pixel_route.h).  Used by tests/test_pixel_batch_route.py."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include "pixel_batch_route.h"
extern "C" int consts(int i) {
    const int v[] = {PIXB_TILE, PIXB_KSTEP, PIXB_KGROUP, PIXB_WAVES, PIXB_THREADS, PIXB_WG_ROWS, PIXB_ACC, PIXB_L0_SLOTS, (int)PIX_LDS_MAX};
    return v[i];
}
extern "C" int hw(int l) { return pix_hw(l); }
extern "C" int side(int l) { return pix_side(l); }
extern "C" int k_true(int l, int cin_l) { return pixb_k(l, cin_l); }
extern "C" int k_pad(int l, int cin_l) { return pixb_k_pad(l, cin_l); }
extern "C" int col_tiles(int C) { return pixb_col_tiles(C); }
extern "C" long lds(int l, int C, int cin) { return (long)pixb_lds(l, C, cin); }
extern "C" void grid(int l, int n, int C, int cin, long *o) {
    const PixGrid g = pixb_grid(l, n, C, cin);
    o[0] = g.x; o[1] = g.y; o[2] = g.z; o[3] = g.threads; o[4] = (long)g.lds;
}
extern "C" int chunks(int n, int chunk) { return pixb_chunks(n, chunk); }
extern "C" int chunk_begin(int i, int chunk) { return pixb_chunk_begin(i, chunk); }
extern "C" int chunk_count(int n, int chunk, int i) { return pixb_chunk_count(n, chunk, i); }
extern "C" long ws_bytes(int chunk, int C) { return (long)pixb_ws_bytes(chunk, C); }

// every store the launch of layer l makes, as the kernel predicates it: counts [n][hw][C] += 1 per stored element; returns the
// number of stores that would land outside [n][hw][C] (padding rows / columns)
extern "C" long coverage(int l, int n, int C, int cin, int *counts) {
    const PixGrid g = pixb_grid(l, n, C, cin);
    long outside = 0;
    for (int b = 0; b < g.x; ++b)
        for (int w = 0; w < g.threads / 64; ++w) {
            const PixbItem it = pixb_item(l, n, b, w);
            for (int ct = 0; ct < pixb_col_tiles(C); ++ct)
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = 0; i < PIXB_ACC; ++i) {
                        const int tr = pixb_acc_row(lane, i), col = ct * PIXB_TILE + pixb_acc_col(lane);
                        if (!(col < C && tr < it.rows)) continue;
                        const long r = it.row0 + tr;
                        const int e = pixb_row_image(l, r), p = pixb_row_pixel(l, r);
                        if (e >= n || p >= pix_hw(l) || col >= C || r >= pixb_rows(l, n)) { ++outside; continue; }
                        ++counts[((long)e * pix_hw(l) + p) * C + col];
                    }
        }
    return outside;
}
// the accumulator layout: tile (row, col) of (lane, register)
extern "C" void acc_elem(int lane, int i, int *o) { o[0] = pixb_acc_row(lane, i); o[1] = pixb_acc_col(lane); }

// A's gather: idx [rows][k_pad] = linear index of the input element ((image * cin_l + ci) * side + y) * side + x that the k-map and
// the source-element map name, -1 on padding k; woff [k_pad] = float offset of B's row in the bound weights, -1 on padding k
extern "C" void gather(int l, int n, int cin_l, int C, long *idx, int *woff) {
    const int kp = pixb_k_pad(l, cin_l), K = pixb_k(l, cin_l), s = pix_side(l);
    for (int k = 0; k < kp; ++k) woff[k] = k < K ? pixb_w_off(l, cin_l, C, k) : -1;
    for (long r = 0; r < pixb_rows(l, n); ++r)
        for (int k = 0; k < kp; ++k) {
            if (k >= K) { idx[r * kp + k] = -1; continue; }
            const PixbSrc e = pixb_src(l, cin_l, r, k);
            idx[r * kp + k] = (((long)e.image * cin_l + e.ci) * s + e.y) * s + e.x;
        }
}
// layer 0's staging for a full workgroup that starts at row r0 (every residue of 256 b mod 841 is some r0 in [0, 841)): o =
// (nA, nB, first staged row of the first image, last staged row of the first image, last staged row of the second image or -1)
extern "C" void stage(long r0, int *o) {
    const PixbStage s = pixb_l0_stage(r0, r0 + PIXB_WG_ROWS - 1);
    o[0] = s.nA; o[1] = s.nB; o[2] = s.yA0; o[3] = s.yA0 + s.nA - 1; o[4] = s.nB - 1;
}
extern "C" void k_decode(int l, int cin_l, int k, int *o) {
    const PixbTap t = pixb_k_decode(l, cin_l, k);
    o[0] = t.ci; o[1] = t.ky; o[2] = t.kx;
}
// the kernel's address split base(row) + a_off(k) against the source-element map; layer 0 through the workgroup's staging
// (slot in range, one slot per staged (image, input row)).  Returns the number of disagreements.
extern "C" long address_errors(int l, int n, int cin_l) {
    long bad = 0;
    const int K = pixb_k(l, cin_l), s = pix_side(l);
    for (long r = 0; r < pixb_rows(l, n); ++r) {
        const int px = pixb_row_pixel(l, r);
        if (l > 0) {
            for (int k = 0; k < K; ++k) {
                const PixbSrc e = pixb_src(l, r, pixb_k_decode(l, cin_l, k));
                if (pixb_a_base(l, px) + pixb_a_off(l, cin_l, k) != (e.ci * s + e.y) * s + e.x) ++bad;
            }
            continue;
        }
        const long wg0 = r / PIXB_WG_ROWS * PIXB_WG_ROWS, nr = pixb_rows(l, n);
        const long wg1 = (wg0 + PIXB_WG_ROWS < nr ? wg0 + PIXB_WG_ROWS : nr) - 1;
        const PixbStage sg = pixb_l0_stage(wg0, wg1);
        if (sg.nA + sg.nB > PIXB_L0_SLOTS || sg.nA < 1 || sg.nB < 0) ++bad;
        const int oy = px / pix_out(0), ox = px % pix_out(0);
        const int base = pixb_l0_patch_off(0, pixb_l0_slot(sg, pixb_row_image(l, r), 2 * oy), 2 * ox);
        for (int k = 0; k < K; ++k) {
            const PixbSrc e = pixb_src(l, r, pixb_k_decode(l, cin_l, k));
            const int slot = pixb_l0_slot(sg, e.image, e.y);
            if (slot < 0 || slot >= sg.nA + sg.nB) ++bad;
            // what the staging loop puts into that slot
            const int se = slot < sg.nA ? sg.eA : sg.eA + 1, sy = slot < sg.nA ? sg.yA0 + slot : slot - sg.nA;
            if (se != e.image || sy != e.y || sy > PIX_IN - 1) ++bad;
            if (base + pixb_a_off(l, cin_l, k) != pixb_l0_patch_off(e.ci, slot, e.x)) ++bad;
        }
    }
    return bad;
}
"""


def build(tmpdir):
    src = os.path.join(str(tmpdir), "pixel_batch_route_shim.cpp")
    with open(src, "w") as f:
        f.write(SHIM)
    so = os.path.join(str(tmpdir), "libpixel_batch_route_shim.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tdmpc2_amd", "csrc"), src, "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    ci, pl, pi = ctypes.c_int, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_int)
    lib.lds.restype = lib.ws_bytes.restype = lib.coverage.restype = lib.address_errors.restype = ctypes.c_long
    lib.grid.argtypes = [ci, ci, ci, ci, pl]
    lib.coverage.argtypes = [ci, ci, ci, ci, pi]
    lib.gather.argtypes = [ci, ci, ci, ci, pl, pi]
    lib.k_decode.argtypes = [ci, ci, ci, pi]
    lib.stage.argtypes = [ctypes.c_long, pi]
    lib.acc_elem.argtypes = [ci, ci, pi]
    return lib


CONSTS = ("TILE", "KSTEP", "KGROUP", "WAVES", "THREADS", "WG_ROWS", "ACC", "L0_SLOTS", "LDS_MAX")


def consts(lib):
    return {k: lib.consts(i) for i, k in enumerate(CONSTS)}


def grid(lib, l, n, C, cin):
    o = (ctypes.c_long * 5)()
    lib.grid(l, n, C, cin, o)
    return dict(zip(("x", "y", "z", "threads", "lds"), o))


def coverage(lib, l, n, C, cin):
    """(counts [n, hw, C] of the stores of layer l's launch, stores outside that range)."""
    counts = np.zeros((n, lib.hw(l), C), dtype=np.int32)
    outside = lib.coverage(l, n, C, cin, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    return counts, int(outside)


def gather(lib, l, n, cin_l, C):
    """(idx [rows, k_pad] into the flattened input [n, cin_l, side, side], woff [k_pad] into the bound weights); -1 = padding."""
    kp, rows = lib.k_pad(l, cin_l), n * lib.hw(l)
    idx, woff = np.zeros((rows, kp), dtype=np.int64), np.zeros(kp, dtype=np.int32)
    lib.gather(l, n, cin_l, C, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_long)), woff.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    return idx, woff


def k_decode(lib, l, cin_l, k):
    o = (ctypes.c_int * 3)()
    lib.k_decode(l, cin_l, k, o)
    return tuple(o)


def stage(lib, r0):
    """(nA, nB, yA first, yA last, yB last) of layer 0's staging for the full workgroup whose first row is r0."""
    o = (ctypes.c_int * 5)()
    lib.stage(r0, o)
    return tuple(o)
