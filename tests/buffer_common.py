"""The replay buffer restated in plain Python / numpy (tdmpc2_buffer_*, tdmpc2_amd/csrc/buffer_route.h): Philox4x32-10, the ring
with its episodes as a deque, the two integer draws and the gather as numpy indexing.  Written independently of the header's
incremental table (eligibility is derived from the list of ALL live episodes at every call), so that the two can be compared.
Also: the header itself behind a C shim for the host compiler (build_route), as tests/refresh_route_model.py does for its header."""
import collections
import ctypes
import math
import os

import numpy as np

from tests import route_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SITE_BUFFER = 8
M32 = 0xFFFFFFFF


def philox4x32_10(c, k):
    """c: four uint32 arrays (or ints), k: two uint32 -> four uint64 arrays holding 32-bit words (common.cuh: philox4x32_10)."""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in c]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k[0]) & M32, int(k[1]) & M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(M32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(M32)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c


def slice_draws(batch, seed, call):
    """r.x, r.y of slice b: counter (b, site, 0, call), key = seed (common.cuh: rng_raw with iter = env = 0)."""
    r = philox4x32_10((np.arange(batch), SITE_BUFFER, 0, int(call) & M32), (seed & M32, (seed >> 32) & M32))
    return r[0], r[1]


def draw(r, n):
    """floor(r n / 2^32): uniform over [0, n), never n."""
    return (np.asarray(r, dtype=np.uint64) * np.uint64(n)) >> np.uint64(32)


class RefBuffer:
    """fields: (row_bytes, step_first, step_count) per field; rows are uint8 arrays [T, row_bytes]."""

    def __init__(self, capacity, slice_len, fields):
        self.cap, self.S, self.fields = int(capacity), int(slice_len), [tuple(f) for f in fields]
        self.storage = [np.zeros((self.cap, rb), np.uint8) for rb, _, _ in self.fields]
        self.episodes = collections.deque()  # (first_logical, end_logical) of every episode with a live step
        self.cursor = 0
        self.num_eps = 0
        self.call = 0

    @property
    def floor(self):
        return max(0, self.cursor - self.cap)

    def add(self, rows):
        T = rows[0].shape[0]
        assert T <= self.cap
        for st, r in zip(self.storage, rows):
            st[(self.cursor + np.arange(T)) % self.cap] = r.reshape(T, -1)
        self.episodes.append((self.cursor, self.cursor + T))
        self.cursor += T
        self.num_eps += 1
        while self.episodes and self.episodes[0][1] <= self.floor:
            self.episodes.popleft()

    def load(self, rows):
        for i in range(rows[0].shape[0]):
            self.add([r[i] for r in rows])

    def eligible(self):
        """[(first live logical step, live steps)] of the episodes with at least S live steps, oldest first."""
        out = []
        for first, end in self.episodes:
            first = max(first, self.floor)
            if end - first >= self.S:
                out.append((first, end - first))
        return out

    def stats(self):
        return {"num_eps": self.num_eps, "live_steps": self.cursor - self.floor, "cursor": self.cursor,
                "eligible": len(self.eligible()), "next_call": self.call}

    def starts(self, batch, seed, call=None):
        el = self.eligible()
        assert el
        rx, ry = slice_draws(batch, seed, self.call if call is None else call)
        e = draw(rx, len(el)).astype(np.int64)
        first = np.array([f for f, _ in el], np.int64)[e]
        ln = np.array([n for _, n in el], np.int64)[e]
        s = ((ry * (ln - self.S + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        return first + s, e

    def sample(self, batch, seed):
        """-> ([step_count, batch, row_bytes] uint8 per field, int64 [batch] logical index of step 0); advances the counter."""
        start, _ = self.starts(batch, seed)
        self.call = (self.call + 1) & M32
        return self.gather(start), start

    def gather(self, start):
        outs = []
        for st, (rb, s0, sc) in zip(self.storage, self.fields):
            logical = start[None, :] + s0 + np.arange(sc)[:, None]
            outs.append(st[logical % self.cap])
        return outs


def chi2_sf_even(x, df):
    """P(chi2_df > x) for even df: exp(-x/2) sum_{j < df/2} (x/2)^j / j!"""
    assert df % 2 == 0
    h, term, tot = x / 2.0, 1.0, 0.0
    for j in range(df // 2):
        tot += term
        term *= h / (j + 1)
    return math.exp(-h) * tot


def chi2_quantile_even(p_upper, df):
    """x with P(chi2_df > x) = p_upper (bisection on the closed form)."""
    lo, hi = 0.0, 1000.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if chi2_sf_even(mid, df) > p_upper else (lo, mid)
    return hi


# ---------------------------------------------------------------- tdmpc2_amd/csrc/buffer_route.h behind a C shim
SHIM = r"""
#include <vector>
#include "buffer_route.h"
struct Ring { BufRing r; std::vector<BufEntry> t; };
extern "C" void *ring_new(uint64_t cap, uint32_t S) {
    Ring *g = new Ring{buf_ring_init(cap, S), {}};
    g->t.assign(g->r.tcap, BufEntry{});
    return g;
}
extern "C" void ring_free(void *p) { delete (Ring *)p; }
// out: cursor, floor, head, count, shrink, shrink_first, shrink_len, n_push, push_slot, push_base, T, touched, skip, copy,
//      pieces, src0, dst0, n0, src1, dst1, n1
extern "C" void ring_write(void *p, uint64_t n_eps, uint32_t T, uint64_t *out) {
    Ring *g = (Ring *)p;
    const uint64_t before = g->r.cursor;
    const BufUpdate u = buf_write(g->r, g->t.data(), n_eps, T);
    uint64_t src[2] = {0, 0}, dst[2] = {0, 0}, n[2] = {0, 0};
    const int pieces = buf_copy_pieces(g->r.cap, before, u, src, dst, n);
    const uint64_t v[21] = {u.cursor, u.floor, u.head, u.count, u.shrink, u.shrink_first, u.shrink_len, u.n_push, u.push_slot,
                            u.push_base, u.T, u.touched, u.skip_steps, u.copy_steps, (uint64_t)pieces, src[0], dst[0], n[0],
                            src[1], dst[1], n[1]};
    for (int i = 0; i < 21; ++i) out[i] = v[i];
}
// out: cap, cursor, floor, num_eps, S, tcap, head, count
extern "C" void ring_state(void *p, uint64_t *out) {
    const BufRing &r = ((Ring *)p)->r;
    const uint64_t v[8] = {r.cap, r.cursor, r.floor, r.num_eps, r.S, r.tcap, r.head, r.count};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
}
extern "C" void ring_entry(void *p, uint32_t slot, uint64_t *out) {
    const BufEntry &e = ((Ring *)p)->t[slot];
    out[0] = e.first; out[1] = e.len;
}
extern "C" void pushed_entry(uint64_t base, uint32_t T, uint64_t floor, uint32_t j, uint64_t *out) {
    BufUpdate u{}; u.push_base = base; u.T = T; u.floor = floor;
    const BufEntry e = buf_pushed_entry(u, j);
    out[0] = e.first; out[1] = e.len;
}
extern "C" uint32_t table_cap(uint64_t cap, uint32_t S) { return buf_table_cap(cap, S); }
extern "C" uint32_t draw_episode(uint32_t r, uint32_t n) { return buf_draw_episode(r, n); }
extern "C" uint32_t draw_start(uint32_t r, uint32_t len, uint32_t S) { return buf_draw_start(r, len, S); }
extern "C" uint32_t access_width(uint32_t rb, uint64_t bits) { return buf_access_width(rb, bits); }
// out: width, units, rows_per_wg, chunks, blocks
extern "C" void field_grid(uint32_t rb, uint64_t bits, uint64_t rows, uint32_t *out) {
    const BufFieldGrid g = buf_field_grid(rb, bits, rows);
    out[0] = g.width; out[1] = g.units; out[2] = g.rows_per_wg; out[3] = g.chunks; out[4] = g.blocks;
}
// out: row0, nrows, unit0, nunits
extern "C" void decode(uint32_t rb, uint64_t bits, uint64_t rows, uint32_t blk, uint64_t *out) {
    const BufWork w = buf_decode(buf_field_grid(rb, bits, rows), rows, blk);
    out[0] = w.row0; out[1] = w.nrows; out[2] = w.unit0; out[3] = w.nunits;
}
extern "C" uint64_t field_bases(uint64_t cap, int n, const uint32_t *rb, uint64_t *base) { return buf_field_bases(cap, n, rb, base); }
extern "C" uint64_t offset(uint64_t base, uint64_t phys, uint32_t rb) { return buf_offset(base, phys, rb); }
extern "C" void constants(uint32_t *out) { out[0] = BUF_THREADS; out[1] = BUF_CHUNK_UNITS; out[2] = BUF_PACK_BELOW; out[3] = BUF_FIELD_ALIGN; out[4] = BUF_MAX_FIELDS; }
"""
UPDATE_KEYS = ("cursor", "floor", "head", "count", "shrink", "shrink_first", "shrink_len", "n_push", "push_slot", "push_base", "T",
               "touched", "skip", "copy", "pieces", "src0", "dst0", "n0", "src1", "dst1", "n1")


def build_route(tmpdir):
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    return route_shim.build_shim(tmpdir, "buffer_route", SHIM, dict(
        ring_new=([u64, u32], vp), ring_free=[vp], ring_write=[vp, u64, u32, ctypes.POINTER(u64)], ring_state=[vp, ctypes.POINTER(u64)],
        ring_entry=[vp, u32, ctypes.POINTER(u64)], pushed_entry=[u64, u32, u64, u32, ctypes.POINTER(u64)], table_cap=([u64, u32], u32),
        draw_episode=([u32, u32], u32), draw_start=([u32, u32, u32], u32), access_width=([u32, u64], u32),
        field_grid=[u32, u64, u64, ctypes.POINTER(u32)], decode=[u32, u64, u64, u32, ctypes.POINTER(u64)],
        field_bases=([u64, ctypes.c_int, ctypes.POINTER(u32), ctypes.POINTER(u64)], u64), offset=([u64, u64, u32], u64),
        constants=[ctypes.POINTER(u32)]), ("-O2",))


class RouteRing:
    """The header's ring and table (the host mirror), plus a second table that is only ever changed the way k_buf_update changes
    the device's: from the by-value numbers of a BufUpdate."""

    def __init__(self, lib, cap, S):
        self.lib, self.h = lib, lib.ring_new(cap, S)
        self.tcap = self.state()["tcap"]
        self.dev_table = [(0, 0)] * self.tcap
        self.dev_head = self.dev_count = 0

    def __del__(self):
        self.lib.ring_free(self.h)

    def state(self):
        out = (ctypes.c_uint64 * 8)()
        self.lib.ring_state(self.h, out)
        return dict(zip(("cap", "cursor", "floor", "num_eps", "S", "tcap", "head", "count"), [int(v) for v in out]))

    def write(self, n_eps, T):
        out = (ctypes.c_uint64 * 21)()
        self.lib.ring_write(self.h, n_eps, T, out)
        u = dict(zip(UPDATE_KEYS, [int(v) for v in out]))
        for j in range(u["n_push"]):  # k_buf_update, thread j
            e = (ctypes.c_uint64 * 2)()
            self.lib.pushed_entry(u["push_base"], u["T"], u["floor"], j, e)
            self.dev_table[(u["push_slot"] + j) % self.tcap] = (int(e[0]), int(e[1]))
        if u["shrink"]:
            self.dev_table[u["head"]] = (u["shrink_first"], u["shrink_len"])
        self.dev_head, self.dev_count = u["head"], u["count"]
        return u

    def mirror_entries(self):
        st = self.state()
        out = []
        for i in range(st["count"]):
            e = (ctypes.c_uint64 * 2)()
            self.lib.ring_entry(self.h, (st["head"] + i) % st["tcap"], e)
            out.append((int(e[0]), int(e[1])))
        return out

    def device_entries(self):
        return [self.dev_table[(self.dev_head + i) % self.tcap] for i in range(self.dev_count)]
