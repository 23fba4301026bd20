"""The dropout-mask unit (tdmpc2_dropout_mask, include/tdmpc2_dropout.h) restated for the tests:
  - `philox` / `mask_model`: Philox4x32-10 and the drop rule in numpy, bit for bit what the header publishes: element e belongs to
    quad e >> 2, lane e & 3; the quad's words are philox((q_lo, q_hi, call_lo, call_hi), (seed_lo, seed_hi)); dropped iff
    word < thr = floor(fp32(p) 2^32); +0.0 or keep = fp32(1) / fp32(1 - fp32(p)).
  - dropout_route.h behind a C shim, and the same walk as a stand-alone program;
  - the shape and the inputs of tests/golden/q_dropout.npz (tools/make_q_dropout_golden.py), and the seeds of the frequency check.
Nothing here comes from a HIP result, and nothing here reads the reference tree."""
import ctypes
import math
import os

import numpy as np

from tests import route_shim
from tests.optim_common import FLOOR, MARGIN, rel_err  # noqa: F401  (the measured gate of DESIGN 3.4h)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "q_dropout.npz")
SYMBOLS = ("tdmpc2_dropout_mask",)
PS = (0.01, 0.1, 0.25, 0.5, 0.9)           # the p values thr and keep are pinned at
SIZES = (1, 3, 4, 5, 1023, 1025)           # n: one element, a partial quad, one quad, a quad and a tail, around 256 quads
THREADS, MAX_BLOCKS = 256, 2048            # dropout_route.h
ONE_PASS = 4 * THREADS * MAX_BLOCKS        # elements of a single pass of the capped grid
PAST_ONE_PASS = ONE_PASS + 4 * THREADS * 3 + 5  # three more workgroups' quads and a partial quad
FREQ_N, FREQ_G, FREQ_P = 5 * 96 * 512, 5, 0.01  # the frequency check: [5, 96, 512] at the default cfg.dropout
FREQ_SEEDS = (1, 20261)                    # chosen in tests/test_q_dropout_math.py so that the restatement passes there
MASK64 = (1 << 64) - 1


# ---------------------------------------------------------------- numpy restatement
def thr_of(p):
    return int(math.floor(float(np.float32(p)) * 4294967296.0))


def keep_of(p):
    return np.float32(1.0) / np.float32(1.0 - float(np.float32(p)))


def philox(q, call, seed):
    """q: uint64 quad indices [m] -> uint32 [m, 4]: Philox4x32-10 of counter (q_lo, q_hi, call_lo, call_hi) under key `seed`."""
    q = np.asarray(q, np.uint64)
    call, seed = int(call) & MASK64, int(seed) & MASK64
    lo32 = np.uint64(0xFFFFFFFF)
    c0, c1 = q & lo32, q >> np.uint64(32)
    c2 = np.full_like(q, call & 0xFFFFFFFF)
    c3 = np.full_like(q, call >> 32)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        m0, m1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (m1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), m1 & lo32, (m0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), m0 & lo32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def mask_model(n, p, seed, call, first=0):
    """Elements first .. first + n - 1 of the mask at counter `call` -> fp32 [n]."""
    q0, q1 = first >> 2, (first + n + 3) >> 2
    words = philox(np.arange(q0, q1, dtype=np.uint64), call, seed).reshape(-1)
    words = words[first - 4 * q0: first - 4 * q0 + n]
    return np.where(words < np.uint32(thr_of(p)), np.float32(0.0), keep_of(p)).astype(np.float32)


# ---------------------------------------------------------------- the fixture's shape and inputs (tools/make_q_dropout_golden.py)
FIX = dict(G=3, T=2, B=5, K=11, hidden=16, out=7, p=0.25, seed=77, call=3)
DROPPED_ROW, KEPT_ROW = (0, 1, 2), (2, 0, 4)  # (member, t, b): a row with every element dropped, one with every element kept
PARAMS = ("w0", "b0", "g0", "be0", "w1", "b1", "g1", "be1", "w2", "b2")


def fixture_masks():
    """[G, T, B, hidden] fp32: the restatement's mask at FIX's seed and counter with the two edge rows overwritten."""
    f = FIX
    m = mask_model(f["G"] * f["T"] * f["B"] * f["hidden"], f["p"], f["seed"], f["call"]).reshape(f["G"], f["T"], f["B"], f["hidden"]).copy()
    m[DROPPED_ROW] = 0.0
    m[KEPT_ROW] = keep_of(f["p"])
    return m


def fixture_inputs():
    """fp32: x [T, B, K], the cotangent [G, T, B, out] and the stacked parameters of the G members (LayerNorm affine away from 1 / 0,
    so that a mask on the wrong side of it would show)."""
    f = FIX
    rng = np.random.default_rng(9100)
    G, K, M, O = f["G"], f["K"], f["hidden"], f["out"]
    x = dict(x=rng.standard_normal((f["T"], f["B"], K)), cot=rng.standard_normal((G, f["T"], f["B"], O)),
             w0=rng.standard_normal((G, M, K)) / np.sqrt(K), b0=0.3 * rng.standard_normal((G, M)),
             g0=1.0 + 0.3 * rng.standard_normal((G, M)), be0=0.2 * rng.standard_normal((G, M)),
             w1=rng.standard_normal((G, M, M)) / np.sqrt(M), b1=0.3 * rng.standard_normal((G, M)),
             g1=1.0 + 0.3 * rng.standard_normal((G, M)), be1=0.2 * rng.standard_normal((G, M)),
             w2=rng.standard_normal((G, O, M)) / np.sqrt(M), b2=0.3 * rng.standard_normal((G, O)))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in x.items()}


def stacked_params(x, dtype, device="cpu", requires_grad=True):
    """The fixture's parameters as the object QEnsemble.apply_params / autograd.ensemble_apply walk (n, layer(i)); -> (params, leaves)."""
    from types import SimpleNamespace

    import torch

    t = {k: torch.tensor(x[k], dtype=dtype, device=device, requires_grad=requires_grad) for k in PARAMS}
    ls = [SimpleNamespace(weight=t["w0"], bias=t["b0"], ln=SimpleNamespace(weight=t["g0"], bias=t["be0"])),
          SimpleNamespace(weight=t["w1"], bias=t["b1"], ln=SimpleNamespace(weight=t["g1"], bias=t["be1"])),
          SimpleNamespace(weight=t["w2"], bias=t["b2"], ln=None)]
    return SimpleNamespace(n=FIX["G"], layer=lambda i: ls[i]), t


def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


# ---------------------------------------------------------------- tdmpc2_amd/csrc/dropout_route.h behind a C shim
SHIM = r"""
#include <string.h>
#include <vector>
#include "dropout_route.h"
extern "C" void constants(int32_t *out) {
    const int32_t c[3] = {DROP_THREADS, DROP_MAX_BLOCKS, (int32_t)sizeof(DropDesc)};
    memcpy(out, c, sizeof c);
}
extern "C" int check(const DropDesc *d) { return drop_check(*d); }
extern "C" uint32_t thr(float p) { return drop_thr(p); }
extern "C" float keep(float p) { return drop_keep(p); }
extern "C" uint64_t grid(uint64_t n) { return drop_grid(n); }
extern "C" uint64_t first_quad(uint64_t block, int thread) { return drop_first_quad(block, thread); }
extern "C" uint64_t quad_stride(uint64_t g) { return drop_quad_stride(g); }
extern "C" uint64_t quad_of(uint64_t e) { return drop_quad_of(e); }
extern "C" int lane_of(uint64_t e) { return drop_lane_of(e); }
extern "C" int quad_elems(uint64_t q, uint64_t n) { return drop_quad_elems(q, n); }
extern "C" uint64_t bump(uint64_t call) {
    uint32_t lo = (uint32_t)call, hi = (uint32_t)(call >> 32);
    drop_bump(lo, hi);
    return ((uint64_t)hi << 32) | lo;
}
extern "C" float serial(const DropDesc *d, uint64_t call, uint64_t e) { return drop_serial(*d, call, e); }
extern "C" void fill(const DropDesc *d, uint64_t call, uint64_t first, uint64_t count, float *out) {
    for (uint64_t i = 0; i < count; ++i) out[i] = drop_serial(*d, call, first + i);
}
// Every workgroup of the mask launch walked as the kernel walks it: each element a thread stores adds one to its mark, a full
// quad's four at once.  Returns the number of marks that are not exactly one plus the stores that would land outside [0, n).
extern "C" uint64_t cover(uint64_t n) {
    std::vector<uint8_t> mark(n, 0);
    uint64_t bad = 0;
    const uint64_t g = drop_grid(n), quads = drop_quads(n);
    bad += g < 1 || g > (uint64_t)DROP_MAX_BLOCKS;
    for (uint64_t b = 0; b < g; ++b)
        for (int t = 0; t < DROP_THREADS; ++t)
            for (uint64_t q = drop_first_quad(b, t); q < quads; q += drop_quad_stride(g)) {
                const int live = drop_quad_elems(q, n);
                if (live < 1 || live > 4) { ++bad; continue; }
                for (int j = 0; j < live; ++j) {
                    const uint64_t e = (q << 2) + (uint64_t)j;
                    if (e >= n) { ++bad; continue; }
                    ++mark[e];
                    bad += drop_quad_of(e) != q || drop_lane_of(e) != j;
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
        DropDesc d{(int64_t)n, 0.25f, 5u, 7u, 0u, 0u, 0u};
        if (drop_check(d) != DROP_OK) return 2;
        bad += cover(n);
        uint64_t dropped = 0;
        std::vector<float> m(n < 4096 ? n : 4096);
        fill(&d, 0xFFFFFFFFull, n - m.size(), m.size(), m.data());
        for (float v : m) { bad += !(v == 0.0f || v == drop_keep(d.p)); dropped += v == 0.0f; }
        printf("n %llu: %llu workgroups, %llu of the last %zu dropped\n", (unsigned long long)n, (unsigned long long)drop_grid(n),
               (unsigned long long)dropped, m.size());
    }
    fclose(f);
    // quads past 2^32 and the counter's carry
    DropDesc big{(int64_t)1 << 40, 0.5f, 1u, 2u, 0u, 0u, 0u};
    const uint64_t e = (((uint64_t)1 << 32) + 5) * 4 + 3;
    bad += drop_quad_of(e) != ((uint64_t)1 << 32) + 5 || drop_lane_of(e) != 3;
    const float v = drop_serial(big, 0xFFFFFFFFull, e);
    bad += !(v == 0.0f || v == 2.0f);
    bad += bump(0xFFFFFFFFull) != 0x100000000ull || bump(0xFFFFFFFFFFFFFFFFull) != 0 || bump(41) != 42;
    bad += drop_grid((uint64_t)1 << 61) != (uint64_t)DROP_MAX_BLOCKS;
    printf("bad %llu\n", (unsigned long long)bad);
    return bad ? 1 : 0;
}
"""


class Desc(ctypes.Structure):  # DropDesc = tdmpc2_dropout_desc
    _fields_ = [("n", ctypes.c_int64), ("p", ctypes.c_float), ("seed_lo", ctypes.c_uint32), ("seed_hi", ctypes.c_uint32),
                ("call_lo", ctypes.c_uint32), ("call_hi", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def desc_of(n, p, seed=0, call=0):
    return Desc(n=n, p=p, seed_lo=seed & 0xFFFFFFFF, seed_hi=(seed >> 32) & 0xFFFFFFFF, call_lo=call & 0xFFFFFFFF,
                call_hi=(call >> 32) & 0xFFFFFFFF, reserved=0)


def build_route(tmpdir):
    dp, u64, i32 = ctypes.POINTER(Desc), ctypes.c_uint64, ctypes.c_int32
    return route_shim.build_shim(tmpdir, "dropout_route", SHIM, dict(
        constants=[ctypes.POINTER(i32)], check=[dp], thr=([ctypes.c_float], ctypes.c_uint32), keep=([ctypes.c_float], ctypes.c_float),
        first_quad=([u64, i32], u64), lane_of=[u64], quad_elems=[u64, u64], serial=([dp, u64, u64], ctypes.c_float),
        fill=[dp, u64, u64, u64, ctypes.POINTER(ctypes.c_float)],
        **{name: ([u64], u64) for name in ("grid", "quad_stride", "quad_of", "bump", "cover")}))


def build_walk(tmpdir, sanitize=False):
    return route_shim.build_walk(tmpdir, "dropout_route", SHIM + MAIN, sanitize)


def walk_input(path):
    sizes = SIZES + (PAST_ONE_PASS,)
    with open(path, "wb") as f:
        f.write(np.asarray([len(sizes), *sizes], np.uint64).tobytes())
    return path
