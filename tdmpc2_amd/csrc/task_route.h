// The arithmetic of the task unit (tdmpc2_task_*, include/tdmpc2_task.h): the refusals, the grids, which path a launch takes, the
// walk of a gather / copy workgroup over its rows, the read of an id, the chunk walk of the table gradient and the renorm of one
// row restated serially, as pure functions.  Compilable on the host, no HIP types: tests/test_task_route.py builds it with the
// host compiler.  The host side (k_task.hip) launches what the grids return; the kernels (task_kernels.cuh) walk with the same
// functions.
//
// R = steps * batch rows of W = D + T + A columns; row r = t * batch + b reads id slot 0 (ids_len == 1) or b.
// Gather (forward) and copy (backward): workgroup g owns rows [g * TASK_ROWS, ..) -- a contiguous block of `out` -- and stages their
// ids once; its units are single columns, or quads of columns when D, T and A are multiples of 4 and every pointer is 16-byte
// aligned (each row then starts on 16 bytes); thread i takes units i, i + TASK_THREADS, ...
// Renorm: workgroup g owns table rows [g * TASK_WAVES, ..), one wavefront each; all its threads read the id list once and flag the
// rows it names.  Lane l sums x[c]^2 over c = l, l + 64, ... in rising order, then the tree s_l += s_{l + w}, w = 32 .. 1.
// Table gradient: workgroup (k, ct) owns columns [ct * TASK_COLS, ..) of table row k, one lane per column.  The rows of task k by
// rising r are position p = t * cnt + j <-> r = t * batch + member[j], member the rising list of the batch columns whose id is k
// (cnt of them; every column when ids_len == 1).  Chunk c is positions [c * TASK_CHUNK, ..): wave w of a round sums chunk
// round * TASK_WAVES + w from 0, row after row; wave 0 then adds the round's chunk sums to the total in chunk order.  The member
// list lives in LDS when batch <= TASK_STAGE; past that one wave scans the ids by rising r and makes the same additions.
// TASK_CHUNK: the split rule gives a quarter of one wave's share of a list; with every row of a B 256, H 3 site (768 to 1024 rows)
// on one task, the 4 waves of its workgroup share 192 to 256 rows each, a quarter of which is 48 to 64.
#pragma once
#include "seed_route.h"  // <math.h>, <stdint.h>, the __host__ / __device__ shim for the host compiler of the test, SeedGrid

enum { TASK_THREADS = 256, TASK_WAVE = 64, TASK_WAVES = 4, TASK_ROWS = 16, TASK_COLS = 64, TASK_CHUNK = 64, TASK_STAGE = 2048 };

struct TaskDesc {  // tdmpc2_task_desc
    int32_t steps, batch, ids_len, id_bytes, num_tasks, x_dim, task_dim, a_dim;
    float max_norm;
    uint32_t reserved;
};

// ---- sizes
__host__ __device__ inline uint64_t task_rows(const TaskDesc &d) { return (uint64_t)d.steps * (uint64_t)d.batch; }
__host__ __device__ inline uint64_t task_width(const TaskDesc &d) { return (uint64_t)d.x_dim + (uint64_t)d.task_dim + (uint64_t)d.a_dim; }
__host__ __device__ inline uint64_t task_ceil(uint64_t n, uint64_t per) { return (n + per - 1) / per; }

// ---- what the entry points refuse: 0 = fine, else the index of the message in k_task.hip.  Bits of `has`: the pointer is not null
enum { TASK_FORWARD = 0, TASK_BACKWARD, TASK_RENORM };
enum { TASK_HAS_TABLE = 1, TASK_HAS_IDS = 2, TASK_HAS_X = 4, TASK_HAS_A = 8, TASK_HAS_OUT = 16,           // forward, renorm
       TASK_HAS_DOUT = 4, TASK_HAS_DX = 32, TASK_HAS_DA = 8, TASK_HAS_DTABLE = 64 };                       // backward (ids as above)
enum { TASK_OK = 0, TASK_BAD_STEPS, TASK_BAD_BATCH, TASK_BAD_X, TASK_BAD_T, TASK_BAD_A, TASK_BAD_TASKS, TASK_BAD_IDS_LEN,
       TASK_BAD_ID_BYTES, TASK_NULL_PTR, TASK_A_GIVEN, TASK_A_ABSENT, TASK_NO_OUTPUT, TASK_HUGE, TASK_GRID };
__host__ __device__ inline uint64_t task_gather_grid(const TaskDesc &d) { return task_ceil(task_rows(d), TASK_ROWS); }
__host__ __device__ inline uint64_t task_renorm_grid(const TaskDesc &d) { return task_ceil((uint64_t)d.num_tasks, TASK_WAVES); }
__host__ __device__ inline uint64_t task_col_tiles(const TaskDesc &d) { return task_ceil((uint64_t)d.task_dim, TASK_COLS); }
// the backward's launch: kind 0 = copy workgroups (dx and / or da), kind 1 = sum workgroups (dtable)
__host__ __device__ inline SeedGrid<2> task_backward_grid(const TaskDesc &d, bool copy, bool sum) {
    return seed_grid<2>((copy ? 1 : 0) | (sum ? 2 : 0),
                        [&](int k) { return k == 0 ? task_rows(d) : (uint64_t)d.num_tasks * task_col_tiles(d); },
                        [&](int k) { return k == 0 ? (uint64_t)TASK_ROWS : (uint64_t)1; });
}
__host__ __device__ inline int task_check(const TaskDesc &d, int op, int has) {
    if (d.steps < 1) return TASK_BAD_STEPS;
    if (d.batch < 1) return TASK_BAD_BATCH;
    if (d.x_dim < 1) return TASK_BAD_X;
    if (d.task_dim < 1) return TASK_BAD_T;
    if (d.a_dim < 0) return TASK_BAD_A;
    if (d.num_tasks < 1) return TASK_BAD_TASKS;
    if (d.ids_len != 1 && d.ids_len != d.batch) return TASK_BAD_IDS_LEN;
    if (d.id_bytes != 4 && d.id_bytes != 8) return TASK_BAD_ID_BYTES;
    if (!(has & TASK_HAS_IDS)) return TASK_NULL_PTR;
    if (op == TASK_FORWARD) {
        if (!(has & TASK_HAS_TABLE) || !(has & TASK_HAS_X) || !(has & TASK_HAS_OUT)) return TASK_NULL_PTR;
        if (d.a_dim == 0 && (has & TASK_HAS_A)) return TASK_A_GIVEN;
        if (d.a_dim > 0 && !(has & TASK_HAS_A)) return TASK_A_ABSENT;
    } else if (op == TASK_BACKWARD) {
        if (!(has & (TASK_HAS_DX | TASK_HAS_DA | TASK_HAS_DTABLE))) return TASK_NO_OUTPUT;
        if (!(has & TASK_HAS_DOUT)) return TASK_NULL_PTR;
        if (d.a_dim == 0 && (has & TASK_HAS_DA)) return TASK_A_GIVEN;
    } else if (!(has & TASK_HAS_TABLE)) {
        return TASK_NULL_PTR;
    }
    const uint64_t W = task_width(d), lim = (uint64_t)1 << 62;
    if (task_rows(d) >= (lim + W - 1) / W) return TASK_HUGE;  // R * W >= 2^62
    const uint64_t top = 0x7fffffffull;
    if (op == TASK_FORWARD && task_gather_grid(d) > top) return TASK_GRID;
    if (op == TASK_BACKWARD && task_backward_grid(d, (has & (TASK_HAS_DX | TASK_HAS_DA)) != 0, (has & TASK_HAS_DTABLE) != 0).first[2] > top)
        return TASK_GRID;
    return TASK_OK;
}

// ---- which path: quads of columns (one 16-byte access) or single columns.  aligned: every pointer of the call is 16-byte aligned
__host__ __device__ inline bool task_vec(const TaskDesc &d, bool aligned) {
    return aligned && !(d.x_dim & 3) && !(d.task_dim & 3) && !(d.a_dim & 3);
}
__host__ __device__ inline int task_lanes(bool vec) { return vec ? 4 : 1; }  // columns of a unit
// the member list of the table gradient lives in LDS (else: the scan of one wave)
__host__ __device__ inline bool task_staged(const TaskDesc &d) { return d.ids_len == 1 || d.batch <= TASK_STAGE; }

// ---- ids
__host__ __device__ inline uint64_t task_id_slot(const TaskDesc &d, uint64_t r) { return d.ids_len == 1 ? 0 : r % (uint64_t)d.batch; }
// the id in slot `slot`, or -1 when it names no table row
__host__ __device__ inline int32_t task_id_read(const TaskDesc &d, const void *ids, uint64_t slot) {
    const int64_t v = d.id_bytes == 8 ? ((const int64_t *)ids)[slot] : (int64_t)((const int32_t *)ids)[slot];
    return v >= 0 && v < (int64_t)d.num_tasks ? (int32_t)v : -1;
}

// ---- the rows of a gather / copy workgroup and the decode of a unit over `cols` columns per row (W, D or A), `lanes` columns each
__host__ __device__ inline uint64_t task_block_row0(uint64_t block) { return block * TASK_ROWS; }
__host__ __device__ inline int task_block_rows(const TaskDesc &d, uint64_t block) {
    const uint64_t left = task_rows(d) - task_block_row0(block);
    return left < (uint64_t)TASK_ROWS ? (int)left : (int)TASK_ROWS;
}
// (W can pass 2^32: the column arithmetic is 64-bit)
__host__ __device__ inline uint64_t task_units(int rows, uint64_t cols, int lanes) { return (uint64_t)rows * (cols / (uint64_t)lanes); }
__host__ __device__ inline void task_unit(uint64_t u, uint64_t cols, int lanes, int &row, uint64_t &col) {
    const uint64_t per = cols / (uint64_t)lanes;
    row = (int)(u / per);
    col = (u % per) * (uint64_t)lanes;
}
// column c of an output row: 0 = x[c - 0], 1 = table[id][c - D], 2 = a[c - D - T]
__host__ __device__ inline int task_segment(const TaskDesc &d, uint64_t c, uint64_t &off) {
    if (c < (uint64_t)d.x_dim) { off = c; return 0; }
    if (c < (uint64_t)d.x_dim + (uint64_t)d.task_dim) { off = c - (uint64_t)d.x_dim; return 1; }
    off = c - (uint64_t)d.x_dim - (uint64_t)d.task_dim;
    return 2;
}

// ---- the sum workgroups of the backward: local index -> (table row, first column)
__host__ __device__ inline void task_sum_decode(const TaskDesc &d, uint64_t local, int32_t &k, uint64_t &col0) {
    const uint64_t tiles = task_col_tiles(d);
    k = (int32_t)(local / tiles);
    col0 = (local % tiles) * TASK_COLS;
}
// ---- the chunk walk: n = cnt * steps positions; chunk c is [c * TASK_CHUNK, min(n, (c + 1) * TASK_CHUNK))
__host__ __device__ inline uint64_t task_positions(const TaskDesc &d, uint64_t cnt) { return cnt * (uint64_t)d.steps; }
__host__ __device__ inline uint64_t task_chunks(uint64_t n) { return task_ceil(n, TASK_CHUNK); }
__host__ __device__ inline uint64_t task_chunk_begin(uint64_t c) { return c * TASK_CHUNK; }
__host__ __device__ inline uint64_t task_chunk_end(uint64_t c, uint64_t n) { return (c + 1) * TASK_CHUNK < n ? (c + 1) * TASK_CHUNK : n; }
// position p -> (step t, index j into the member list); the row is t * batch + member[j]
__host__ __device__ inline void task_position(uint64_t p, uint64_t cnt, uint64_t &t, uint64_t &j) { t = p / cnt; j = p % cnt; }
__host__ __device__ inline void task_position_next(uint64_t cnt, uint64_t &t, uint64_t &j) {
    if (++j == cnt) { j = 0; ++t; }
}

// ---- the renorm of one row, serially: the kernel's additions in the kernel's order
__host__ inline float task_norm_serial(const float *x, int T) {
    float s[TASK_WAVE];
    for (int l = 0; l < TASK_WAVE; ++l) {
        float acc = 0.0f;
        for (int c = l; c < T; c += TASK_WAVE) {
            const float sq = x[c] * x[c];
            acc = acc + sq;
        }
        s[l] = acc;
    }
    for (int w = TASK_WAVE / 2; w > 0; w >>= 1)
        for (int l = 0; l < w; ++l) s[l] = s[l] + s[l + w];
    return sqrtf(s[0]);
}
__host__ __device__ inline bool task_scales(float norm, float max_norm) { return norm > max_norm; }
__host__ __device__ inline float task_scale(float norm, float max_norm) { return max_norm / (norm + 1e-7f); }
__host__ inline void task_renorm_serial(float *x, int T, float max_norm) {
    const float norm = task_norm_serial(x, T);
    if (!task_scales(norm, max_norm)) return;
    const float scale = task_scale(norm, max_norm);
    for (int c = 0; c < T; ++c) x[c] = x[c] * scale;
}

// ---- dtable[k, c] serially, two ways that make the same additions: by the chunk walk over a member list (`member`: room for batch
// entries) and by the scan of the rows in rising order (the path past TASK_STAGE)
__host__ inline float task_dtable_chunked(const TaskDesc &d, const void *ids, const float *dout, int32_t k, uint32_t c, uint32_t *member) {
    uint64_t cnt = 0;
    for (uint64_t b = 0; b < (uint64_t)d.batch; ++b)
        if (task_id_read(d, ids, task_id_slot(d, b)) == k) member[cnt++] = (uint32_t)b;
    const uint64_t n = task_positions(d, cnt), W = task_width(d);
    float total = 0.0f;
    for (uint64_t ch = 0; ch < task_chunks(n); ++ch) {
        float s = 0.0f;
        uint64_t t, j;
        task_position(task_chunk_begin(ch), cnt, t, j);
        for (uint64_t p = task_chunk_begin(ch); p < task_chunk_end(ch, n); ++p, task_position_next(cnt, t, j))
            s = s + dout[(t * (uint64_t)d.batch + member[j]) * W + (uint64_t)d.x_dim + c];
        total = total + s;
    }
    return total;
}
__host__ inline float task_dtable_scan(const TaskDesc &d, const void *ids, const float *dout, int32_t k, uint32_t c) {
    const uint64_t W = task_width(d);
    float total = 0.0f, s = 0.0f;
    int in_chunk = 0;
    for (uint64_t r = 0; r < task_rows(d); ++r) {
        if (task_id_read(d, ids, task_id_slot(d, r)) != k) continue;
        s = s + dout[r * W + (uint64_t)d.x_dim + c];
        if (++in_chunk == TASK_CHUNK) { total = total + s; s = 0.0f; in_chunk = 0; }
    }
    if (in_chunk) total = total + s;
    return total;
}
