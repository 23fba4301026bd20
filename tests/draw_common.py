"""The draw unit (tdmpc2_draw_noise, include/tdmpc2_draw.h) restated for the tests:
  - `words` / `normals64` / `pair_of`: the header's rules in numpy on tests/dropout_common.py's Philox: element e belongs to quad
    e >> 2, lane e & 3; the quad's words are philox((q_lo, q_hi, call_lo, call_hi), (seed_lo, seed_hi)); u(x) is the fp32 value of
    (fp32(x >> 8) + 0.5) 2^-24; lanes 0 / 1 are r cos(2 pi u(w1)) / r sin(2 pi u(w1)), r = sqrt(-2 ln u(w0)), in fp64; lanes 2 / 3
    the same from (w2, w3).  The pair comes from the words of counter (2^64 - 1, call): i = (w0 num_q) >> 32, k = (w1 (num_q - 1))
    >> 32, j = k + (k >= i).
  - draw_route.h behind a C shim, and the same walk as a stand-alone program;
  - the gate of the normals: |x - x64| <= 8 * 2^-24 * max(|x64|, 1) (logf, sqrtf and the product at most 1 ulp each, sincospif about
    2, doubled).
Nothing here comes from a HIP result, and nothing here reads the reference tree."""
import ctypes

import numpy as np

from tests import route_shim
from tests.dropout_common import MASK64, philox

SYMBOLS = ("tdmpc2_draw_noise",)
KEY_HI = 0x44524157                        # "DRAW": autograd.Draws keys Philox with (cfg.seed, KEY_HI)
SIZES = (1, 2, 3, 4, 5, 4097)              # n: a partial quad of each length, one quad, a quad and a tail, past 1024 quads
GPU_SIZES = (1, 3, 4, 5, 4097)
THREADS, MAX_BLOCKS, MAXQ = 256, 2048, 8   # draw_route.h
ONE_PASS = 4 * THREADS * MAX_BLOCKS        # elements of a single pass of the capped grid
PAST_ONE_PASS = ONE_PASS + 4 * THREADS * 3 + 5  # three more workgroups' quads and a partial quad
PAIR_QUAD = MASK64                         # the quad index of the pair's counter
TOL = 8.0 * 2.0 ** -24
NUM_QS = (2, 3, 5, 8)


def key_of(seed):
    """The 64-bit key of autograd.Draws(seed)."""
    return (KEY_HI << 32) | (int(seed) & 0xFFFFFFFF)


# ---------------------------------------------------------------- numpy restatement
def u01(x):
    """uint32 words -> the fp32 uniforms, formed as the header says (fp32 throughout: above 2^23 the half rounds to even)."""
    return (np.asarray(x >> np.uint32(8), np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def words(n, key, call, first=0):
    """uint32 [quads, 4] of the quads that hold elements first .. first + n - 1."""
    q0, q1 = first >> 2, (first + n + 3) >> 2
    return philox(np.arange(q0, q1, dtype=np.uint64), call, key)


def normals_of_words(w):
    """uint32 [m, 4] -> fp64 [m, 4]."""
    u = u01(w).astype(np.float64)
    out = np.empty(w.shape, np.float64)
    for a in (0, 2):
        r, ang = np.sqrt(-2.0 * np.log(u[:, a])), 2.0 * np.pi * u[:, a + 1]
        out[:, a], out[:, a + 1] = r * np.cos(ang), r * np.sin(ang)
    return out


def normals64(n, key, call, first=0):
    """Elements first .. first + n - 1 of the normals at counter `call` -> fp64 [n]."""
    off = first - 4 * (first >> 2)
    return normals_of_words(words(n, key, call, first)).reshape(-1)[off:off + n]


def pair_rule(w0, w1, num_q):
    i = (int(w0) * num_q) >> 32
    k = (int(w1) * (num_q - 1)) >> 32
    return i, k + (k >= i)


def pair_of(num_q, key, call):
    w = philox(np.asarray([PAIR_QUAD], np.uint64), call, key)[0]
    return pair_rule(w[0], w[1], num_q)


def gate_ratio(got, ref64):
    """max |x - x64| / (TOL max(|x64|, 1)): at most 1 inside the gate."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    return float((np.abs(got - ref64) / (TOL * np.maximum(np.abs(ref64), 1.0))).max()) if got.size else 0.0


# ---------------------------------------------------------------- tdmpc2_amd/csrc/draw_route.h behind a C shim
SHIM = r"""
#include <string.h>
#include <vector>
#include "draw_route.h"
extern "C" void constants(int32_t *out) {
    const int32_t c[4] = {DRAW_THREADS, DRAW_MAX_BLOCKS, DRAW_MAXQ, (int32_t)sizeof(DrawDesc)};
    memcpy(out, c, sizeof c);
}
extern "C" int check(const DrawDesc *d, int has_normal, int has_pair, uint64_t addr) { return draw_check(*d, has_normal, has_pair, addr); }
extern "C" uint64_t grid(uint64_t n) { return draw_grid(n); }
extern "C" uint64_t first_quad(uint64_t block, int thread) { return draw_first_quad(block, thread); }
extern "C" uint64_t quad_stride(uint64_t g) { return draw_quad_stride(g); }
extern "C" uint64_t quad_of(uint64_t e) { return draw_quad_of(e); }
extern "C" int lane_of(uint64_t e) { return draw_lane_of(e); }
extern "C" int quad_elems(uint64_t q, uint64_t n) { return draw_quad_elems(q, n); }
extern "C" uint64_t bump(uint64_t call) {
    uint32_t lo = (uint32_t)call, hi = (uint32_t)(call >> 32);
    draw_bump(lo, hi);
    return ((uint64_t)hi << 32) | lo;
}
extern "C" float u01(uint32_t x) { return draw_u01(x); }
extern "C" void quad_words(const DrawDesc *d, uint64_t call, uint64_t q, uint32_t *w) { draw_quad_words(*d, call, q, w); }
extern "C" void pair_rule(uint32_t w0, uint32_t w1, int32_t num_q, int32_t *out) { draw_pair(w0, w1, num_q, out[0], out[1]); }
extern "C" void pair(const DrawDesc *d, uint64_t call, int32_t *out) { draw_pair_serial(*d, call, out[0], out[1]); }
extern "C" double serial(const DrawDesc *d, uint64_t call, uint64_t e) { return draw_serial64(*d, call, e); }
extern "C" void fill(const DrawDesc *d, uint64_t call, uint64_t first, uint64_t count, double *out) {
    for (uint64_t i = 0; i < count; ++i) out[i] = draw_serial64(*d, call, first + i);
}
// counts[i * num_q + j] += 1 for the pair of each of `count` consecutive call counters from `call`
extern "C" void pair_counts(const DrawDesc *d, uint64_t call, uint64_t count, uint64_t *counts) {
    for (uint64_t c = 0; c < count; ++c) {
        int32_t i, j;
        draw_pair_serial(*d, call + c, i, j);
        ++counts[i * d->num_q + j];
    }
}
// Every workgroup of the draw launch walked as the kernel walks it: each element a thread stores adds one to its mark, a full
// quad's four at once.  Returns the number of marks that are not exactly one plus the stores that would land outside [0, n).
extern "C" uint64_t cover(uint64_t n) {
    std::vector<uint8_t> mark(n, 0);
    uint64_t bad = 0;
    const uint64_t g = draw_grid(n), quads = draw_quads(n);
    bad += g < 1 || g > (uint64_t)DRAW_MAX_BLOCKS;
    for (uint64_t b = 0; b < g; ++b)
        for (int t = 0; t < DRAW_THREADS; ++t)
            for (uint64_t q = draw_first_quad(b, t); q < quads; q += draw_quad_stride(g)) {
                const int live = draw_quad_elems(q, n);
                if (live < 1 || live > 4) { ++bad; continue; }
                for (int j = 0; j < live; ++j) {
                    const uint64_t e = (q << 2) + (uint64_t)j;
                    if (e >= n) { ++bad; continue; }
                    ++mark[e];
                    bad += draw_quad_of(e) != q || draw_lane_of(e) != j;
                }
            }
    for (uint8_t m : mark) bad += m != 1;
    return bad;
}
"""
# the same walk as a program of its own (build_walk; with sanitize=True under AddressSanitizer and UBSan): argv[1] names a file of
# uint64 words: the number of sizes, then the sizes
MAIN = r"""
#include <stdio.h>
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t count = 0;
    if (fread(&count, 8, 1, f) != 1) return 2;
    uint64_t bad = 0;
    for (uint64_t k = 0; k < count; ++k) {
        uint64_t n = 0;
        if (fread(&n, 8, 1, f) != 1) return 2;
        DrawDesc d{(int64_t)n, 5, 5u, 7u, 0u, 0u, 0u};
        if (draw_check(d, true, true, 64) != DRAW_OK) return 2;
        bad += cover(n);
        std::vector<double> m(n < 4096 ? n : 4096);
        fill(&d, 0xFFFFFFFFull, n - m.size(), m.size(), m.data());
        double top = 0.0;
        for (double v : m) { bad += !(v == v) || !(fabs(v) < 6.0); top = fabs(v) > top ? fabs(v) : top; }
        int32_t p[2];
        pair(&d, 0xFFFFFFFFull + k, p);
        bad += p[0] == p[1] || p[0] < 0 || p[0] >= d.num_q || p[1] < 0 || p[1] >= d.num_q;
        printf("n %llu: %llu workgroups, largest of the last %zu %.3f, pair (%d, %d)\n", (unsigned long long)n,
               (unsigned long long)draw_grid(n), m.size(), top, p[0], p[1]);
    }
    fclose(f);
    // the pair alone, quads past 2^32, the edge words of the pair rule and the counter's carry
    DrawDesc none{0, 8, 1u, 2u, 0u, 0u, 0u};
    bad += draw_check(none, false, true, 0) != DRAW_OK || draw_grid(0) != 1 || cover(0) != 0;
    DrawDesc big{(int64_t)1 << 40, 2, 1u, 2u, 0u, 0u, 0u};
    const uint64_t e = (((uint64_t)1 << 32) + 5) * 4 + 3;
    bad += draw_quad_of(e) != ((uint64_t)1 << 32) + 5 || draw_lane_of(e) != 3;
    const double v = draw_serial64(big, 0xFFFFFFFFull, e);
    bad += !(fabs(v) < 6.0);
    for (int nq = 2; nq <= DRAW_MAXQ; ++nq) {
        const uint32_t edge[3][2] = {{0u, 0u}, {0xFFFFFFFFu, 0xFFFFFFFFu}, {0u, 0xFFFFFFFFu}};
        for (auto &w : edge) {
            int32_t p[2];
            pair_rule(w[0], w[1], nq, p);
            bad += p[0] == p[1] || p[0] < 0 || p[0] >= nq || p[1] < 0 || p[1] >= nq;
        }
    }
    bad += draw_u01(0xFFFFFFFFu) != 1.0f || !(draw_u01(0u) > 0.0f);
    bad += bump(0xFFFFFFFFull) != 0x100000000ull || bump(0xFFFFFFFFFFFFFFFFull) != 0 || bump(41) != 42;
    bad += draw_grid((uint64_t)1 << 61) != (uint64_t)DRAW_MAX_BLOCKS;
    printf("bad %llu\n", (unsigned long long)bad);
    return bad ? 1 : 0;
}
"""


class Desc(ctypes.Structure):  # DrawDesc = tdmpc2_draw_desc
    _fields_ = [("n", ctypes.c_int64), ("num_q", ctypes.c_int32), ("seed_lo", ctypes.c_uint32), ("seed_hi", ctypes.c_uint32),
                ("call_lo", ctypes.c_uint32), ("call_hi", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def desc_of(n, num_q=0, key=0, call=0):
    return Desc(n=n, num_q=num_q, seed_lo=key & 0xFFFFFFFF, seed_hi=(key >> 32) & 0xFFFFFFFF, call_lo=call & 0xFFFFFFFF,
                call_hi=(call >> 32) & 0xFFFFFFFF, reserved=0)


def build_route(tmpdir):
    dp, u64, u32, i32 = ctypes.POINTER(Desc), ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32
    return route_shim.build_shim(tmpdir, "draw_route", SHIM, dict(
        constants=[ctypes.POINTER(i32)], check=[dp, i32, i32, u64], first_quad=([u64, i32], u64), lane_of=[u64], quad_elems=[u64, u64],
        u01=([u32], ctypes.c_float), quad_words=[dp, u64, u64, ctypes.POINTER(u32)], pair_rule=[u32, u32, i32, ctypes.POINTER(i32)],
        pair=[dp, u64, ctypes.POINTER(i32)], serial=([dp, u64, u64], ctypes.c_double),
        fill=[dp, u64, u64, u64, ctypes.POINTER(ctypes.c_double)], pair_counts=[dp, u64, u64, ctypes.POINTER(u64)],
        **{name: ([u64], u64) for name in ("grid", "quad_stride", "quad_of", "bump", "cover")}))


def build_walk(tmpdir, sanitize=False):
    return route_shim.build_walk(tmpdir, "draw_route", SHIM + MAIN, sanitize)


def walk_input(path):
    sizes = SIZES + (PAST_ONE_PASS,)
    with open(path, "wb") as f:
        f.write(np.asarray([len(sizes), *sizes], np.uint64).tobytes())
    return path
