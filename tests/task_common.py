"""The task unit (tdmpc2_task_*, include/tdmpc2_task.h) restated for the tests:
  - `renorm32` / `renorm64`: the header's renorm in numpy fp32, addition for addition (lane l sums x[c]^2 over c = l, l + 64, ... in
    rising order; the tree s_l += s_{l + w}, w = 32 .. 1; sqrt; max_norm / (norm + 1e-7); the products), and in fp64;
  - `gather`: out = [x | table[id] | a], NaN in the embedding columns of a row whose id names no table row;
  - `dtable32` / `dtable64`: the table gradient in the header's fixed order (the rows of a task by rising r, chunks of CHUNK rows,
    each chunk summed from 0 row after row, the chunk sums added from 0 in chunk order) and in fp64;
  - the two bounds, from the documented orders alone (u = 2^-24):
      renorm: every addend of the sum of squares is positive, so its relative error is at most depth(T) u with
        depth(T) = 1 (the square) + ceil(T / 64) (the lane's additions) + 6 (the tree); sqrt, the addition of 1e-7, the division and
        the product add one rounding each; doubled as DESIGN 3.4n doubles: |x - x64| <= 2 (depth(T) + 4) u |x64|;
      table gradient: an element passes through at most min(n, CHUNK) additions of its chunk and chunks(n) additions of the total,
        so |s - s64| <= gamma(min(n, CHUNK) + chunks(n)) sum |terms|, gamma(m) = m u / (1 - m u);
  - task_route.h behind a C shim, and the same walks as a stand-alone program.
Nothing here comes from a HIP result, and nothing here reads the reference tree."""
import ctypes

import numpy as np

from tests import route_shim

SYMBOLS = ("tdmpc2_task_forward", "tdmpc2_task_backward", "tdmpc2_task_renorm")
THREADS, WAVE, WAVES, ROWS, COLS, CHUNK, STAGE = 256, 64, 4, 16, 64, 64, 2048  # task_route.h
U = 2.0 ** -24
# (steps, batch, D, T, A): one element; one row with odd widths; widths that are multiples of 4 (the 16-byte path), three row
# blocks; odd batch, more than one column tile, more than one chunk per task
SHAPES = ((1, 1, 1, 1, 0), (1, 1, 5, 64, 3), (4, 12, 8, 64, 4), (3, 43, 24, 96, 6))
ONE_TASK_ROWS = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
NUM_TASKS = 30


# ---------------------------------------------------------------- numpy restatement
def row_ids(steps, batch, ids):
    """The id of every row r = t * batch + b -> int64 [R]; ids holds 1 or batch entries."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    return np.tile(ids if ids.size == batch else np.repeat(ids, batch), steps)


def valid(ids, num_tasks):
    ids = np.asarray(ids, np.int64)
    return (ids >= 0) & (ids < num_tasks)


def norm32(x):
    """The fp32 norm of one row in the header's order."""
    x = np.asarray(x, np.float32)
    pad = np.zeros(-(-x.size // WAVE) * WAVE, np.float32)
    pad[:x.size] = x
    s = np.zeros(WAVE, np.float32)
    for chunk in pad.reshape(-1, WAVE):  # lane l: c = l, l + 64, ...; the padding adds + 0 to a sum that is >= + 0
        s = s + chunk * chunk
    w = WAVE // 2
    while w > 0:
        s[:w] = s[:w] + s[w:2 * w]
        w //= 2
    return np.sqrt(s[0])


def renorm32(table, ids, max_norm):
    """The table after one call's renorm, fp32 [num_tasks, T]: rows named by a valid id, each once."""
    out = np.array(table, np.float32, copy=True)
    if not max_norm > 0:
        return out
    ids = np.asarray(ids, np.int64).reshape(-1)
    for k in np.unique(ids[valid(ids, out.shape[0])]):
        norm = norm32(out[k])
        if norm > np.float32(max_norm):
            out[k] = out[k] * (np.float32(max_norm) / (norm + np.float32(1e-7)))
    return out


def renorm64(table, ids, max_norm):
    out = np.array(table, np.float64, copy=True)
    if not max_norm > 0:
        return out
    ids = np.asarray(ids, np.int64).reshape(-1)
    for k in np.unique(ids[valid(ids, out.shape[0])]):
        norm = np.sqrt((out[k] * out[k]).sum())
        if norm > max_norm:
            out[k] = out[k] * (max_norm / (norm + 1e-7))
    return out


def renorm_depth(T):
    return 1 + -(-T // WAVE) + 6


def renorm_tol(T):
    """Relative, per element."""
    return 2.0 * (renorm_depth(T) + 4) * U


def gather(table, rid, x, a=None):
    """out [R, D + T + A] in the dtype of `table`; rid: the id of every row (row_ids)."""
    table = np.asarray(table)
    ok = valid(rid, table.shape[0])
    emb = np.full((rid.size, table.shape[1]), np.nan, table.dtype)
    emb[ok] = table[rid[ok]]
    parts = [np.asarray(x, table.dtype).reshape(rid.size, -1), emb]
    if a is not None:
        parts.append(np.asarray(a, table.dtype).reshape(rid.size, -1))
    return np.concatenate(parts, axis=1)


def dtable32(g, rid, num_tasks):
    """g [R, T] (dout's embedding block) -> fp32 [num_tasks, T] in the fixed order."""
    g = np.asarray(g, np.float32)
    out = np.zeros((num_tasks, g.shape[1]), np.float32)
    for k in range(num_tasks):
        rows = np.flatnonzero(rid == k)
        total = np.zeros(g.shape[1], np.float32)
        for c0 in range(0, rows.size, CHUNK):
            s = np.zeros(g.shape[1], np.float32)
            for r in rows[c0:c0 + CHUNK]:
                s = s + g[r]
            total = total + s
        out[k] = total
    return out


def dtable64(g, rid, num_tasks):
    g = np.asarray(g, np.float64)
    out = np.zeros((num_tasks, g.shape[1]), np.float64)
    for k in range(num_tasks):
        out[k] = g[rid == k].sum(axis=0)
    return out


def dtable_bound(g, rid, num_tasks):
    """fp64 [num_tasks, T]: the absolute bound of every element (0 for a task without rows)."""
    g = np.abs(np.asarray(g, np.float64))
    out = np.zeros((num_tasks, g.shape[1]), np.float64)
    for k in range(num_tasks):
        n = int((rid == k).sum())
        m = min(n, CHUNK) + -(-n // CHUNK)
        out[k] = m * U / (1.0 - m * U) * g[rid == k].sum(axis=0)
    return out


# ---------------------------------------------------------------- tdmpc2_amd/csrc/task_route.h behind a C shim
SHIM = r"""
#include <string.h>
#include <vector>
#include "task_route.h"
extern "C" void constants(int32_t *out) {
    const int32_t c[8] = {TASK_THREADS, TASK_WAVE, TASK_WAVES, TASK_ROWS, TASK_COLS, TASK_CHUNK, TASK_STAGE, (int32_t)sizeof(TaskDesc)};
    memcpy(out, c, sizeof c);
}
extern "C" int check(const TaskDesc *d, int op, int has) { return task_check(*d, op, has); }
extern "C" int vec(const TaskDesc *d, int aligned) { return task_vec(*d, aligned != 0); }
extern "C" int staged(const TaskDesc *d) { return task_staged(*d); }
extern "C" uint64_t gather_grid(const TaskDesc *d) { return task_gather_grid(*d); }
extern "C" uint64_t renorm_grid(const TaskDesc *d) { return task_renorm_grid(*d); }
extern "C" uint64_t backward_grid(const TaskDesc *d, int copy, int sum) { return task_backward_grid(*d, copy != 0, sum != 0).first[2]; }
extern "C" int32_t id_read(const TaskDesc *d, const void *ids, uint64_t slot) { return task_id_read(*d, ids, slot); }
extern "C" float norm(const float *x, int T) { return task_norm_serial(x, T); }
extern "C" void renorm_row(float *x, int T, float max_norm) { task_renorm_serial(x, T, max_norm); }

// The gather launch walked as the kernel walks it: every workgroup, every thread, every unit.  mark counts the writes of each
// element of out; an element must be written once, from the source the layout names.  Returns the number of violations.
extern "C" uint64_t gather_cover(const TaskDesc *dp, int vec_) {
    const TaskDesc &d = *dp;
    const uint64_t R = task_rows(d), W = task_width(d);
    std::vector<uint8_t> mark(R * W, 0);
    uint64_t bad = 0;
    const int lanes = task_lanes(vec_ != 0);
    bad += vec_ && !task_vec(d, true);
    for (uint64_t g = 0; g < task_gather_grid(d); ++g) {
        const uint64_t r0 = task_block_row0(g);
        const int n = task_block_rows(d, g);
        bad += n < 1 || n > TASK_ROWS || r0 + (uint64_t)n > R;
        const uint64_t units = task_units(n, W, lanes);
        for (int t = 0; t < TASK_THREADS; ++t)
            for (uint64_t u = (uint64_t)t; u < units; u += TASK_THREADS) {
                int row;
                uint64_t c, off;
                task_unit(u, W, lanes, row, c);
                if (row < 0 || row >= n || c + (uint64_t)lanes > W) { ++bad; continue; }
                const int seg = task_segment(d, c, off);
                const uint64_t lo = seg == 0 ? 0 : seg == 1 ? (uint64_t)d.x_dim : (uint64_t)d.x_dim + (uint64_t)d.task_dim;
                const uint64_t len = seg == 0 ? (uint64_t)d.x_dim : seg == 1 ? (uint64_t)d.task_dim : (uint64_t)d.a_dim;
                bad += lo + off != c || off + (uint64_t)lanes > len;  // a unit never straddles two sources
                bad += vec_ && ((((r0 + (uint64_t)row) * W + c) & 3) || (off & 3));
                for (int i = 0; i < lanes; ++i) ++mark[(r0 + (uint64_t)row) * W + c + (uint64_t)i];
            }
    }
    for (uint8_t m : mark) bad += m != 1;
    return bad;
}
// The backward launch: copy workgroups mark dx / da, sum workgroups mark the columns of dtable they own.
extern "C" uint64_t backward_cover(const TaskDesc *dp, int vec_, int want_dx, int want_da, int want_dtable) {
    const TaskDesc &d = *dp;
    const uint64_t R = task_rows(d), D = (uint64_t)d.x_dim, T = (uint64_t)d.task_dim, A = (uint64_t)d.a_dim, W = task_width(d);
    std::vector<uint8_t> mx(R * D, 0), ma(R * A, 0), mt((uint64_t)d.num_tasks * T, 0);
    uint64_t bad = 0;
    const int lanes = task_lanes(vec_ != 0);
    const SeedGrid<2> grid = task_backward_grid(d, want_dx || want_da, want_dtable != 0);
    for (uint64_t g = 0; g < grid.first[2]; ++g) {
        int kind;
        uint64_t local;
        seed_decode(grid, g, kind, local);
        if (kind == 0) {
            bad += !(want_dx || want_da);
            const uint64_t r0 = task_block_row0(local);
            const int n = task_block_rows(d, local);
            bad += n < 1 || n > TASK_ROWS || r0 + (uint64_t)n > R;
            for (int part = 0; part < 2; ++part) {
                if (!(part == 0 ? want_dx : want_da)) continue;
                const uint64_t cols = part == 0 ? D : A, first = part == 0 ? 0 : D + T;
                const uint64_t units = task_units(n, cols, lanes);
                for (int t = 0; t < TASK_THREADS; ++t)
                    for (uint64_t u = (uint64_t)t; u < units; u += TASK_THREADS) {
                        int row;
                        uint64_t c;
                        task_unit(u, cols, lanes, row, c);
                        if (row < 0 || row >= n || c + (uint64_t)lanes > cols || first + c + (uint64_t)lanes > W) { ++bad; continue; }
                        for (int i = 0; i < lanes; ++i) ++(part == 0 ? mx : ma)[(r0 + (uint64_t)row) * cols + c + (uint64_t)i];
                    }
            }
        } else {
            bad += !want_dtable;
            int32_t k;
            uint64_t col0;
            task_sum_decode(d, local, k, col0);
            if (k < 0 || k >= d.num_tasks || col0 >= T) { ++bad; continue; }
            for (int lane = 0; lane < TASK_COLS; ++lane)
                if (col0 + (uint64_t)lane < T) ++mt[(uint64_t)k * T + col0 + (uint64_t)lane];
        }
    }
    for (uint8_t m : mx) bad += m != (want_dx ? 1 : 0);
    for (uint8_t m : ma) bad += m != (want_da ? 1 : 0);
    for (uint8_t m : mt) bad += m != (want_dtable ? 1 : 0);
    return bad;
}
// The rows the chunk walk of task k visits, in the order it visits them, and the chunk of each -> the number of rows.  rows / chunk_of:
// room for R entries.
extern "C" uint64_t chunk_walk(const TaskDesc *dp, const void *ids, int32_t k, uint64_t *rows, uint64_t *chunk_of) {
    const TaskDesc &d = *dp;
    std::vector<uint32_t> member;
    for (uint64_t b = 0; b < (uint64_t)d.batch; ++b)
        if (task_id_read(d, ids, task_id_slot(d, b)) == k) member.push_back((uint32_t)b);
    const uint64_t cnt = member.size(), n = task_positions(d, cnt);
    uint64_t at = 0;
    for (uint64_t ch = 0; ch < task_chunks(n); ++ch) {
        uint64_t t, j;
        task_position(task_chunk_begin(ch), cnt, t, j);
        for (uint64_t p = task_chunk_begin(ch); p < task_chunk_end(ch, n); ++p, task_position_next(cnt, t, j)) {
            rows[at] = t * (uint64_t)d.batch + member[j];
            chunk_of[at++] = ch;
        }
    }
    return at;
}
// dtable [num_tasks, T] by the chunk walk (which = 0) or by the scan (which = 1)
extern "C" void dtable(const TaskDesc *dp, const void *ids, const float *dout, int which, float *out) {
    const TaskDesc &d = *dp;
    std::vector<uint32_t> member((size_t)d.batch);
    for (int32_t k = 0; k < d.num_tasks; ++k)
        for (uint32_t c = 0; c < (uint32_t)d.task_dim; ++c)
            out[(uint64_t)k * (uint64_t)d.task_dim + c] =
                which ? task_dtable_scan(d, ids, dout, k, c) : task_dtable_chunked(d, ids, dout, k, c, member.data());
}
"""
# the same walks as a program of its own (build_walk; with sanitize=True under AddressSanitizer and UBSan): argv[1] names a file of
# int32 words: the number of cases, then (steps, batch, ids_len, D, T, A, one_task) per case
MAIN = r"""
#include <stdio.h>
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    uint64_t bad = 0;
    for (int32_t i = 0; i < count; ++i) {
        int32_t w[7];
        if (fread(w, 4, 7, f) != 7) return 2;
        for (int id_bytes = 4; id_bytes <= 8; id_bytes += 4) {
            TaskDesc d{w[0], w[1], w[2], id_bytes, 30, w[3], w[4], w[5], 1.0f, 0u};
            if (task_check(d, TASK_FORWARD, TASK_HAS_TABLE | TASK_HAS_IDS | TASK_HAS_X | (w[5] ? TASK_HAS_A : 0) | TASK_HAS_OUT) != TASK_OK) return 2;
            std::vector<int64_t> i64((size_t)d.ids_len);
            std::vector<int32_t> i32((size_t)d.ids_len);
            for (int32_t b = 0; b < d.ids_len; ++b) {
                i64[(size_t)b] = w[6] ? 7 : b % 30;
                if (b == 1 && !w[6]) i64[(size_t)b] = -1;  // an id that names no row
                i32[(size_t)b] = (int32_t)i64[(size_t)b];
            }
            const void *ids = id_bytes == 8 ? (const void *)i64.data() : (const void *)i32.data();
            for (int v = 0; v <= (task_vec(d, true) ? 1 : 0); ++v) {
                bad += gather_cover(&d, v);
                for (int want = 1; want < 8; ++want) {
                    if ((want & 2) && !d.a_dim) continue;
                    bad += backward_cover(&d, v, want & 1, want & 2, want & 4);
                }
            }
            const uint64_t R = task_rows(d), W = task_width(d);
            std::vector<uint64_t> rows(R), chunk_of(R);
            std::vector<uint8_t> seen(R, 0);
            std::vector<float> dout(R * W), a((size_t)d.num_tasks * (size_t)d.task_dim), b2(a.size());
            for (uint64_t e = 0; e < R * W; ++e) dout[e] = (float)((e * 2654435761u) % 1000) * 0.001f - 0.5f;
            for (int32_t k = 0; k < d.num_tasks; ++k) {
                const uint64_t n = chunk_walk(&d, ids, k, rows.data(), chunk_of.data());
                for (uint64_t q = 0; q < n; ++q) {
                    bad += rows[q] >= R || (q && rows[q] <= rows[q - 1]) || chunk_of[q] != q / TASK_CHUNK;
                    if (rows[q] < R) bad += task_id_read(d, ids, task_id_slot(d, rows[q])) != k || seen[rows[q]]++;
                }
            }
            for (uint64_t r = 0; r < R; ++r) bad += seen[r] != (task_id_read(d, ids, task_id_slot(d, r)) >= 0 ? 1 : 0);
            dtable(&d, ids, dout.data(), 0, a.data());
            dtable(&d, ids, dout.data(), 1, b2.data());
            bad += memcmp(a.data(), b2.data(), a.size() * 4) != 0;
            std::vector<float> row((size_t)d.task_dim, 0.25f);
            task_renorm_serial(row.data(), d.task_dim, 1.0f);
            bad += !(task_norm_serial(row.data(), d.task_dim) <= 1.0f + 1e-5f);
            printf("(%d, %d, %d, %d, %d) ids_len %d id_bytes %d: %llu + %llu workgroups\n", w[0], w[1], w[3], w[4], w[5], w[2], id_bytes,
                   (unsigned long long)task_gather_grid(d), (unsigned long long)task_backward_grid(d, true, true).first[2]);
        }
    }
    fclose(f);
    printf("bad %llu\n", (unsigned long long)bad);
    return bad ? 1 : 0;
}
"""


class Desc(ctypes.Structure):  # TaskDesc = tdmpc2_task_desc
    _fields_ = [(n, ctypes.c_int32) for n in ("steps", "batch", "ids_len", "id_bytes", "num_tasks", "x_dim", "task_dim", "a_dim")] + \
               [("max_norm", ctypes.c_float), ("reserved", ctypes.c_uint32)]


def desc_of(steps, batch, ids_len, id_bytes, num_tasks, D, T, A=0, max_norm=1.0):
    return Desc(steps, batch, ids_len, id_bytes, num_tasks, D, T, A, max_norm, 0)


FORWARD, BACKWARD, RENORM = range(3)
HAS = dict(table=1, ids=2, x=4, a=8, out=16, dout=4, dx=32, da=8, dtable=64)


def has(*names):
    return sum(HAS[n] for n in names)


def build_route(tmpdir):
    dp, u64, i32, vp = ctypes.POINTER(Desc), ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p
    fp = ctypes.POINTER(ctypes.c_float)
    return route_shim.build_shim(tmpdir, "task_route", SHIM, dict(
        constants=[ctypes.POINTER(i32)], check=[dp, i32, i32], vec=[dp, i32], staged=[dp], gather_grid=([dp], u64),
        renorm_grid=([dp], u64), backward_grid=([dp, i32, i32], u64), id_read=([dp, vp, u64], i32), norm=([fp, i32], ctypes.c_float),
        renorm_row=([fp, i32, ctypes.c_float], None), gather_cover=([dp, i32], u64), backward_cover=([dp, i32, i32, i32, i32], u64),
        chunk_walk=([dp, vp, i32, ctypes.POINTER(u64), ctypes.POINTER(u64)], u64), dtable=([dp, vp, fp, i32, fp], None)))


def build_walk(tmpdir, sanitize=False):
    return route_shim.build_walk(tmpdir, "task_route", SHIM + MAIN, sanitize)


def walk_cases():
    """(steps, batch, ids_len, D, T, A, one_task) of the stand-alone program: the shapes with one id and with an id per batch
    column, and every row on one task at the chunk edges (as steps = 1 rows of their own ids, and as steps > 1 with one id)."""
    cases = []
    for s, b, D, T, A in SHAPES:
        cases += [(s, b, 1, D, T, A, 0), (s, b, b, D, T, A, 0), (s, b, b, D, T, A, 1)]
    for R in ONE_TASK_ROWS:
        cases += [(1, R, R, 3, 5, 0, 1), (1, R, 1, 3, 5, 2, 1)]
    cases.append((3, 43, 1, 4, 8, 0, 1))
    return cases


def walk_input(path):
    cases = walk_cases()
    with open(path, "wb") as f:
        f.write(np.asarray([len(cases)] + [v for c in cases for v in c], np.int32).tobytes())
    return path
