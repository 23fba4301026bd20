"""The optimiser step (tdmpc2_optim_*, include/tdmpc2_plan.h) restated for the tests:
  - `emulate_step`: one step in numpy, generic in the dtype.  With float32 every operation is a separately rounded fp32 operation
    in the header's order and the scalars are the fp64 running products rounded once: an emulation of the library's arithmetic,
    bit for bit (numpy's fp32 multiply, add, divide and sqrt are IEEE correctly rounded).  With float64 it is the reference.
  - `norm_model`: the gradient norm in the published order of tdmpc2_amd/csrc/optim_route.h (chunk -> partial -> total).
  - the case table shared by the CPU and the GPU tests, and the header behind a C shim.

Hyperparameters are fp32 in the C ABI.  `widen` gives the doubles the library computes with (fp32(0.999) = 0.99900001287...): the
fp64 references of the measured gates get those, so the gates measure arithmetic and not the representation of 0.999 in fp32."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24  # unit roundoff of fp32
from tests import route_shim
from tests.route_shim import FLOOR, MARGIN, rel_err  # noqa: F401  (the measured gate of DESIGN 3.4h)
THREADS, QUADS_PER_THREAD, CHUNK = 256, 2, 2048  # OPT_* of optim_route.h (test_optim_route.py checks them against the header)


def widen(x):
    """The double a fp32 hyperparameter of the C ABI stands for."""
    return float(np.float32(x))


# ---------------------------------------------------------------- cases
EDGE_COUNTS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 70001)
LRS = (3e-4, 1e-3, 9e-5)  # group 1 stays empty


def _case(name, counts, misaligned=False):
    counts = [int(c) for c in counts]
    return dict(name=name, counts=counts, groups=[0 if i % 3 else 2 for i in range(len(counts))], lrs=LRS, misaligned=misaligned)


def cases():
    rng = np.random.default_rng(300)
    return [_case("edges", EDGE_COUNTS),
            _case("many", rng.integers(1, 8, 300)),
            _case("long", [(1 << 20) + 3]),  # crosses every chunk boundary of 513 chunks; 3 partials per thread of the total pass
            _case("misaligned", (1, 3, 4, 5, 64, 257, 1025, 4097), misaligned=True)]


CASES = {c["name"]: c for c in cases()}
HYPER = dict(beta1=0.9, beta2=0.999, eps=1e-8)
REGIMES = {"noclip": 1e7, "clip": 1.0}  # max_norm above / below every norm make_grads can produce at these sizes


def layout(counts):
    """offsets and arena floats: every segment padded to 4 floats."""
    offs, at = [], 0
    for c in counts:
        offs.append(at)
        at += (c + 3) // 4 * 4
    return offs, at


def make_values(counts, seed, lo=1e-6, hi=1e3):
    """Per segment: fp32 values with |x| log-uniform in [lo, hi] and a random sign."""
    rng = np.random.default_rng(seed)
    return [(np.exp(rng.uniform(np.log(lo), np.log(hi), c)) * rng.choice((-1.0, 1.0), c)).astype(np.float32) for c in counts]


def to_arena(segs, counts):
    offs, n = layout(counts)
    a = np.zeros(n, np.float32)
    for s, o, c in zip(segs, offs, counts):
        a[o:o + c] = s
    return a


def from_arena(a, counts):
    offs, _ = layout(counts)
    return [a[o:o + c].copy() for o, c in zip(offs, counts)]


def padding_mask(counts):
    offs, n = layout(counts)
    m = np.ones(n, bool)
    for o, c in zip(offs, counts):
        m[o:o + c] = False
    return m


# ---------------------------------------------------------------- the step
def new_state(counts, dtype):
    return dict(step=0, b1p=1.0, b2p=1.0, m=[np.zeros(c, dtype) for c in counts], v=[np.zeros(c, dtype) for c in counts])


def set_step(st, k, beta1, beta2):
    st["step"], st["b1p"], st["b2p"] = k, 1.0, 1.0
    for _ in range(k):
        st["b1p"] *= beta1
        st["b2p"] *= beta2


def emulate_step(st, params, grads, groups, lrs, beta1, beta2, eps, max_norm, dtype, norm=None, zero_grad=True):
    """In place on st, params, grads (lists of arrays of `dtype`).  beta1, beta2, lrs, eps, max_norm: python doubles (for float32
    pass the widened fp32 values).  norm: the norm to clip with (the fp32 gate feeds the library's own), default: the norm of
    `grads` with the squares summed in fp64.  Returns the norm used."""
    f = dtype
    if norm is None:
        norm = f(np.sqrt(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in grads)))
    norm = f(norm)
    with np.errstate(all="ignore"):
        r = f(max_norm) / (norm + f(1e-6))
        c = f(1) if r > f(1) else r  # keeps a NaN
        st["step"] += 1
        st["b1p"] *= beta1
        st["b2p"] *= beta2
        bc = f(np.sqrt(np.float64(1.0 - st["b2p"])))
        a1, a2, b2, e = f(1.0 - beta1), f(1.0 - beta2), f(beta2), f(eps)
        for i, (p, g) in enumerate(zip(params, grads)):
            ss = f(np.float64(lrs[groups[i]]) / np.float64(1.0 - st["b1p"]))
            m, v = st["m"][i], st["v"][i]
            g[:] = g * c
            m[:] = m + (g - m) * a1
            v[:] = v * b2 + (g * a2) * g
            d = np.sqrt(v) / bc + e
            p[:] = p - ss * (m / d)
            if zero_grad:
                g[:] = 0
            assert p.dtype == f and m.dtype == f and v.dtype == f and d.dtype == f
    return norm


def torch_steps(params0, grads_per_step, groups, lrs, beta1, beta2, eps, max_norm, dtype):
    """clip_grad_norm_ + torch.optim.Adam on the CPU in `dtype` -> (params, exp_avg, exp_avg_sq as lists of numpy arrays, norms)."""
    import torch

    ps = [torch.nn.Parameter(torch.tensor(p, dtype=dtype)) for p in params0]
    by_group = [dict(params=[p for p, g in zip(ps, groups) if g == gi], lr=lr) for gi, lr in enumerate(lrs)]
    opt = torch.optim.Adam([g for g in by_group if g["params"]], lr=lrs[0], betas=(beta1, beta2), eps=eps)
    norms = []
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = torch.tensor(g, dtype=dtype)
        norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
        opt.step()
    out = lambda k: [opt.state[p][k].numpy().copy() for p in ps]  # noqa: E731
    return [p.detach().numpy().copy() for p in ps], out("exp_avg"), out("exp_avg_sq"), norms


# ---------------------------------------------------------------- the norm's published order
def _butterfly_and_waves(acc):
    """acc [..., 256] per-thread sums -> [...] the workgroup's sum: xor butterfly per wave of 64, then ((w0 + w1) + w2) + w3."""
    a = acc.reshape(acc.shape[:-1] + (4, 64)).astype(np.float32)
    lane = np.arange(64)
    for w in (32, 16, 8, 4, 2, 1):
        a = a + a[..., lane ^ w]
    t = a[..., 0, 0]
    for w in (1, 2, 3):
        t = t + a[..., w, 0]
    return t


def norm_model(arena):
    """fp32 arena (padded layout) -> (norm, partials) in the order of optim_route.h."""
    chunks = -(-arena.size // CHUNK)
    g = np.zeros(chunks * CHUNK, np.float32)
    g[:arena.size] = arena
    with np.errstate(all="ignore"):
        g = g.reshape(chunks, QUADS_PER_THREAD, THREADS, 4)  # quad = chunk * 512 + j * 256 + thread
        acc = np.zeros((chunks, THREADS), np.float32)
        for j in range(QUADS_PER_THREAD):
            for i in range(4):
                acc = acc + g[:, j, :, i] * g[:, j, :, i]
        partial = _butterfly_and_waves(acc)
        rounds = -(-chunks // THREADS)
        p = np.zeros(rounds * THREADS, np.float32)
        p[:chunks] = partial
        acc = np.zeros(THREADS, np.float32)
        for k in range(rounds):
            acc = acc + p[k * THREADS:(k + 1) * THREADS]
        return np.sqrt(_butterfly_and_waves(acc)), partial


def norm_depth(arena_floats):
    """D: the longest chain of additions a square passes through (opt_norm_depth)."""
    chunks = -(-arena_floats // CHUNK)
    return QUADS_PER_THREAD * 4 + 6 + 3 + -(-chunks // THREADS) + 6 + 3


# ---------------------------------------------------------------- tdmpc2_amd/csrc/optim_route.h behind a C shim
SHIM = r"""
#include <string.h>
#include "optim_route.h"
extern "C" void constants(int32_t *out) {
    const int32_t c[8] = {OPT_THREADS, OPT_WAVES, OPT_QUAD, OPT_QUADS_PER_THREAD, OPT_CHUNK_QUADS, OPT_CHUNK, OPT_ALIGN, (int32_t)sizeof(OptSeg)};
    memcpy(out, c, sizeof c);
}
extern "C" uint64_t layout(int64_t n, const int64_t *counts, int64_t *offsets) { return opt_layout(n, counts, sizeof(int64_t), offsets); }
extern "C" uint64_t chunks(uint64_t arena_floats) { return opt_chunks(arena_floats); }
extern "C" uint64_t depth(uint64_t arena_floats) { return opt_norm_depth(arena_floats); }
// every (thread, j) of chunk `chunk` that passes the kernels' bounds test adds one to its quad, relative to the chunk's first;
// returns the number of quads that fell outside the chunk's own range
extern "C" uint64_t cover_chunk(uint64_t chunk, uint64_t arena_quads, uint8_t *marks) {
    uint64_t bad = 0;
    for (int t = 0; t < OPT_THREADS; ++t)
        for (int j = 0; j < OPT_QUADS_PER_THREAD; ++j) {
            const uint64_t q = opt_quad(chunk, t, j);
            if (q >= arena_quads) continue;
            if (q < chunk * OPT_CHUNK_QUADS || q >= (chunk + 1) * OPT_CHUNK_QUADS) ++bad; else ++marks[q - chunk * OPT_CHUNK_QUADS];
        }
    return bad;
}
// the segment of every quad as the update kernel finds it (chunk_seg bounds, then the search); returns mismatches against seg_ref
extern "C" uint64_t seg_walk(int32_t n, const int64_t *offsets, uint64_t arena_floats, const int32_t *seg_ref) {
    OptSeg *segs = new OptSeg[n];
    for (int32_t i = 0; i < n; ++i) segs[i] = OptSeg{nullptr, (uint64_t)offsets[i] / OPT_QUAD, 0, 0, 0};
    const uint64_t nch = opt_chunks(arena_floats), quads = arena_floats / OPT_QUAD;
    int32_t *chunk_seg = new int32_t[nch + 1];
    int32_t s = 0;
    for (uint64_t c = 0; c < nch; ++c) chunk_seg[c] = s = opt_seg_of_quad(&segs[0].quad0, sizeof(OptSeg), s, n - 1, c * OPT_CHUNK_QUADS);
    chunk_seg[nch] = n - 1;
    uint64_t bad = 0;
    for (uint64_t c = 0; c < nch; ++c)
        for (int t = 0; t < OPT_THREADS; ++t)
            for (int j = 0; j < OPT_QUADS_PER_THREAD; ++j) {
                const uint64_t q = opt_quad(c, t, j);
                if (q >= quads) continue;
                if (opt_seg_of_quad(&segs[0].quad0, sizeof(OptSeg), chunk_seg[c], chunk_seg[c + 1], q) != seg_ref[q]) ++bad;
            }
    delete[] segs;
    delete[] chunk_seg;
    return bad;
}
extern "C" void block(uint64_t n_segs, uint64_t n_groups, uint64_t nch, uint64_t *out) {
    const OptBlock b = opt_block(n_segs, n_groups, nch);
    const uint64_t o[7] = {b.segs_off, b.chunk_seg_off, b.lr_off, b.state_off, b.ss_off, b.partial_off, b.bytes};
    memcpy(out, o, sizeof o);
}
extern "C" int check_hyper(float b1, float b2, float eps, float mn) { return opt_check_hyper(b1, b2, eps, mn); }
extern "C" int check_seg(int64_t count, int32_t group, int32_t n_groups, int has_param) { return opt_check_seg(count, group, n_groups, has_param ? "" : nullptr); }
"""
# the same walk as a program of its own (build_walk; with sanitize=True under AddressSanitizer and UBSan): argv[1] names a file of
# int64 words: cases, then per case n and its counts
MAIN = r"""
#include <stdio.h>
#include <vector>
extern "C" uint64_t layout(int64_t, const int64_t *, int64_t *);
extern "C" uint64_t chunks(uint64_t);
extern "C" uint64_t cover_chunk(uint64_t, uint64_t, uint8_t *);
extern "C" uint64_t seg_walk(int32_t, const int64_t *, uint64_t, const int32_t *);
extern "C" uint64_t depth(uint64_t);
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t ncases = 0;
    if (fread(&ncases, 8, 1, f) != 1) return 2;
    uint64_t bad = 0;
    for (int64_t k = 0; k < ncases; ++k) {
        int64_t n = 0;
        if (fread(&n, 8, 1, f) != 1) return 2;
        std::vector<int64_t> counts(n), offs(n);
        if (fread(counts.data(), 8, n, f) != (size_t)n) return 2;
        const uint64_t arena = layout(n, counts.data(), offs.data()), quads = arena / 4, nch = chunks(arena);
        std::vector<int32_t> ref(quads);
        for (int64_t i = 0; i < n; ++i)
            for (uint64_t q = offs[i] / 4; q < (i + 1 < n ? (uint64_t)offs[i + 1] / 4 : quads); ++q) ref[q] = (int32_t)i;
        bad += seg_walk((int32_t)n, offs.data(), arena, ref.data());
        for (uint64_t c = 0; c < nch; ++c) {
            std::vector<uint8_t> marks(512, 0);
            bad += cover_chunk(c, quads, marks.data());
            for (uint64_t q = 0; q < 512; ++q) bad += marks[q] != (c * 512 + q < quads ? 1 : 0);
        }
        printf("case %lld: arena %llu chunks %llu depth %llu\n", (long long)k, (unsigned long long)arena, (unsigned long long)nch,
               (unsigned long long)depth(arena));
    }
    // totals past 2^32 elements: the last chunks of a long arena
    const uint64_t big = (1ull << 32) + 3 * 2048 + 8, quads = big / 4, nch = chunks(big);
    for (uint64_t c = nch - 3; c < nch; ++c) {
        std::vector<uint8_t> marks(512, 0);
        bad += cover_chunk(c, quads, marks.data());
        for (uint64_t q = 0; q < 512; ++q) bad += marks[q] != (c * 512 + q < quads ? 1 : 0);
    }
    fclose(f);
    printf("bad %llu\n", (unsigned long long)bad);
    return bad ? 1 : 0;
}
"""
CONSTANT_KEYS = ("THREADS", "WAVES", "QUAD", "QUADS_PER_THREAD", "CHUNK_QUADS", "CHUNK", "ALIGN", "SEG_BYTES")
BLOCK_KEYS = ("segs_off", "chunk_seg_off", "lr_off", "state_off", "ss_off", "partial_off", "bytes")


def build_route(tmpdir):
    i64p, u64, i32 = ctypes.POINTER(ctypes.c_int64), ctypes.c_uint64, ctypes.c_int32
    return route_shim.build_shim(tmpdir, "optim_route", SHIM, dict(
        constants=[ctypes.POINTER(i32)], layout=([ctypes.c_int64, i64p, i64p], u64), chunks=([u64], u64), depth=([u64], u64),
        cover_chunk=([u64, u64, ctypes.POINTER(ctypes.c_uint8)], u64), seg_walk=([i32, i64p, u64, ctypes.POINTER(i32)], u64),
        block=[u64, u64, u64, ctypes.POINTER(u64)], check_hyper=[ctypes.c_float] * 4, check_seg=[ctypes.c_int64, i32, i32, ctypes.c_int]))


def build_walk(tmpdir, sanitize=False):
    return route_shim.build_walk(tmpdir, "optim_route", SHIM + MAIN, sanitize)


def walk_input(path):
    words = [len(cases())]
    for case in cases():
        words += [len(case["counts"])] + case["counts"]
    with open(path, "wb") as f:
        f.write(np.asarray(words, np.int64).tobytes())
    return path
