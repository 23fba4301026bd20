// The arithmetic of the replay buffer (tdmpc2_buffer_*): ring and eligibility table, the two integer draws of a slice, and the
// grouped gather's launch geometry, as pure functions.  Compilable on the host, no HIP types: tests/test_buffer_route.py builds
// it with the host compiler and checks it against a Python restatement.  The host side (k_buffer.hip) walks what these return;
// the kernels (buffer_kernels.cuh) use the same functions to decode a workgroup index.
//
// Ring: steps carry a 64-bit LOGICAL index (count of steps ever written); the physical row is logical % capacity.  Writing
// evicts the oldest logical steps: floor = max(0, cursor - capacity) is the oldest live one.
// Table: the episodes with at least S = slice_len live steps, as {first_logical, len}, in a ring of capacity / S + 1 entries:
// appended at the tail, shrunk or popped at the head only (eviction always strikes the oldest steps).
#pragma once
#include "seed_route.h"  // <math.h>, <stdint.h> and the __host__ / __device__ shim for the host compiler of the test

enum { BUF_MAX_FIELDS = 8, BUF_THREADS = 256 };
enum { BUF_CHUNK_UNITS = 768 };   // accesses per workgroup of a split row: 3 per thread, all loads in flight before the stores
enum { BUF_PACK_BELOW = 1024 };   // rows under this many bytes are packed several to a workgroup
enum { BUF_FIELD_ALIGN = 256 };   // every field's storage starts on this boundary

struct BufEntry {
    uint64_t first;  // logical index of the episode's oldest live step
    uint32_t len;    // live steps (>= S while the entry is in the table)
    uint32_t pad;
};
struct BufRing {
    uint64_t cap, cursor, floor, num_eps;  // cursor: steps ever written; floor: oldest live logical step
    uint32_t S, tcap, head, count;         // table ring: tcap slots, `count` entries from `head`
};
__host__ __device__ inline uint32_t buf_table_cap(uint64_t cap, uint32_t S) { return (uint32_t)(cap / S) + 1u; }
inline BufRing buf_ring_init(uint64_t cap, uint32_t S) {
    BufRing r{};
    r.cap = cap;
    r.S = S;
    r.tcap = buf_table_cap(cap, S);
    return r;
}

// What writing n_eps episodes of T steps each (add: n_eps = 1) does to the ring and the table.  The host applies it to its
// mirror (buf_write does) and hands the same numbers to the update kernel by value.
struct BufUpdate {
    uint64_t cursor, floor;          // after the write
    uint32_t head, count;            // after the write
    uint32_t shrink;                 // 1: the surviving head entry lost its front -> table[head] = {shrink_first, shrink_len}
    uint32_t shrink_len;
    uint64_t shrink_first;
    uint32_t n_push, push_slot;      // new entries j < n_push go to slot (push_slot + j) % tcap ...
    uint64_t push_base;              // ... and are {max(push_base + j T, floor), push_base + (j + 1) T - that}
    uint32_t T;
    uint32_t touched;                // table entries read or written (add is O(touched), never O(num_eps))
    uint64_t skip_steps;             // leading source steps that would be evicted by the same write: not copied
    uint64_t copy_steps;             // steps copied, starting at logical cursor_before + skip_steps
};
__host__ __device__ inline BufEntry buf_pushed_entry(const BufUpdate &u, uint32_t j) {
    const uint64_t beg = u.push_base + (uint64_t)j * u.T, end = beg + u.T;
    const uint64_t first = beg > u.floor ? beg : u.floor;
    return BufEntry{first, (uint32_t)(end - first), 0u};
}
// table: the host mirror, tcap entries.  T >= 1, n_eps >= 1, T <= cap (the caller refuses the rest).
inline BufUpdate buf_write(BufRing &r, BufEntry *table, uint64_t n_eps, uint32_t T) {
    BufUpdate u{};
    const uint64_t total = n_eps * (uint64_t)T;
    u.cursor = r.cursor + total;
    u.floor = u.cursor > r.cap ? u.cursor - r.cap : 0;
    u.skip_steps = total > r.cap ? total - r.cap : 0;
    u.copy_steps = total - u.skip_steps;
    u.T = T;
    // old entries: pop while fewer than S steps stay live; the first survivor may lose its front
    uint32_t head = r.head, count = r.count;
    while (count) {
        BufEntry &e = table[head];
        ++u.touched;
        if (e.first >= u.floor) break;
        const uint64_t lost = u.floor - e.first;
        if (lost < e.len && e.len - lost >= r.S) {
            e.first = u.floor;
            e.len = (uint32_t)(e.len - lost);
            u.shrink = 1;
            u.shrink_first = e.first;
            u.shrink_len = e.len;
            break;
        }
        head = (head + 1) % r.tcap;
        --count;
    }
    // new episodes: episode i covers [cursor + i T, cursor + (i + 1) T); the ones this same write evicts below S live steps
    // were pushed and popped again by n_eps single adds: the head moves past their slots, nothing is written
    if (T >= r.S) {
        uint64_t i0 = 0;  // first episode that keeps >= S live steps: (i + 1) T - S >= floor - cursor_before
        if (u.floor > r.cursor) {
            const uint64_t need = u.floor - r.cursor + r.S;  // cursor + (i + 1) T >= floor + S
            i0 = (need + T - 1) / T - 1;
        }
        const uint32_t tail = (uint32_t)((head + count) % r.tcap);
        if (i0 > 0 && count == 0) head = (uint32_t)((head + i0) % r.tcap);  // (count == 0 whenever i0 > 0: the floor passed every old step)
        u.push_slot = i0 > 0 ? head : tail;
        u.push_base = r.cursor + i0 * T;
        u.n_push = (uint32_t)(n_eps - i0);
        for (uint32_t j = 0; j < u.n_push; ++j) table[(u.push_slot + j) % r.tcap] = buf_pushed_entry(u, j);
        u.touched += u.n_push;
        count += u.n_push;
    }
    u.head = head;
    u.count = count;
    r.cursor = u.cursor;
    r.floor = u.floor;
    r.head = head;
    r.count = count;
    r.num_eps += n_eps;
    return u;
}
// the copy of a write: at most two physical pieces around the wrap.  Returns the number of pieces; piece k moves n[k] steps from
// source step src[k] to physical row dst[k].
inline int buf_copy_pieces(uint64_t cap, uint64_t cursor_before, const BufUpdate &u, uint64_t src[2], uint64_t dst[2], uint64_t n[2]) {
    if (!u.copy_steps) return 0;
    const uint64_t phys = (cursor_before + u.skip_steps) % cap;
    const uint64_t n0 = u.copy_steps < cap - phys ? u.copy_steps : cap - phys;
    src[0] = u.skip_steps; dst[0] = phys; n[0] = n0;
    if (n0 == u.copy_steps) return 1;
    src[1] = u.skip_steps + n0; dst[1] = 0; n[1] = u.copy_steps - n0;
    return 2;
}

// ---- the two draws of a slice (Philox words r.x, r.y): floor(r n / 2^32) is uniform over [0, n) and can never return n
__host__ __device__ inline uint32_t buf_draw(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * n) >> 32); }
__host__ __device__ inline uint32_t buf_draw_episode(uint32_t rx, uint32_t count) { return buf_draw(rx, count); }
__host__ __device__ inline uint32_t buf_draw_start(uint32_t ry, uint32_t len, uint32_t S) { return buf_draw(ry, len - S + 1u); }

// ---- storage: one region per field, field after field, each on a BUF_FIELD_ALIGN boundary.  All byte offsets are 64-bit.
__host__ __device__ inline uint64_t buf_align_up(uint64_t x) { return (x + (BUF_FIELD_ALIGN - 1)) & ~(uint64_t)(BUF_FIELD_ALIGN - 1); }
inline uint64_t buf_field_bases(uint64_t cap, int n_fields, const uint32_t *row_bytes, uint64_t *base) {  // returns the total
    uint64_t off = 0;
    for (int f = 0; f < n_fields; ++f) {
        base[f] = off;
        off = buf_align_up(off + cap * (uint64_t)row_bytes[f]);
    }
    return off;
}
__host__ __device__ inline uint64_t buf_offset(uint64_t field_base, uint64_t phys_row, uint32_t row_bytes) {
    return field_base + phys_row * (uint64_t)row_bytes;
}

// ---- the grouped gather: per field the access width, and how its B x step_count output rows map to workgroups
// align_bits: the OR of both base addresses (its low 4 bits decide)
__host__ __device__ inline uint32_t buf_access_width(uint32_t row_bytes, uint64_t align_bits) {
    if (row_bytes % 16 == 0 && (align_bits & 15) == 0) return 16;
    if (row_bytes % 4 == 0 && (align_bits & 3) == 0) return 4;
    return 1;
}
struct BufFieldGrid {
    uint32_t width;         // bytes per access: 16, 4 or 1
    uint32_t units;         // accesses per row
    uint32_t rows_per_wg;   // > 0: packed, this many whole rows per workgroup; 0: split, `chunks` workgroups per row
    uint32_t chunks;
    uint32_t blocks;        // workgroups of the field
};
__host__ __device__ inline BufFieldGrid buf_field_grid(uint32_t row_bytes, uint64_t align_bits, uint64_t rows) {
    BufFieldGrid g{};
    g.width = buf_access_width(row_bytes, align_bits);
    g.units = row_bytes / g.width;
    if (row_bytes < BUF_PACK_BELOW) {
        g.rows_per_wg = g.units >= BUF_THREADS ? 1u : BUF_THREADS / g.units;
        g.chunks = 1;
        g.blocks = (uint32_t)((rows + g.rows_per_wg - 1) / g.rows_per_wg);
    } else {
        g.rows_per_wg = 0;
        g.chunks = (g.units + BUF_CHUNK_UNITS - 1) / BUF_CHUNK_UNITS;
        g.blocks = (uint32_t)(rows * g.chunks);
    }
    return g;
}
// Workgroup `blk` of a field -> its output rows [row0, row0 + nrows) and units [unit0, unit0 + nunits) of each
struct BufWork {
    uint64_t row0;
    uint32_t nrows, unit0, nunits;
};
__host__ __device__ inline BufWork buf_decode(const BufFieldGrid &g, uint64_t rows, uint32_t blk) {
    BufWork w{};
    if (g.rows_per_wg) {
        w.row0 = (uint64_t)blk * g.rows_per_wg;
        const uint64_t left = rows - w.row0;
        w.nrows = left < g.rows_per_wg ? (uint32_t)left : g.rows_per_wg;
        w.unit0 = 0;
        w.nunits = g.units;
    } else {
        w.row0 = blk / g.chunks;
        w.nrows = 1;
        w.unit0 = (blk % g.chunks) * BUF_CHUNK_UNITS;
        const uint32_t left = g.units - w.unit0;
        w.nunits = left < BUF_CHUNK_UNITS ? left : BUF_CHUNK_UNITS;
    }
    return w;
}
// An output row o of a field is (step, slice) = (o / B, o % B): time-major, as Buffer._prepare_batch returns the batch.
