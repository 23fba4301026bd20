// Kernels of the task unit (tdmpc2_task_*), included by k_task.hip alone.  Every decision (the rows of a workgroup, the decode of a
// unit, the read of an id, the chunk walk, when a row is scaled and by what) is task_route.h's.  The unit is compiled without fp
// contraction: the renorm is a chain of separately rounded fp32 operations that tests/task_common.py restates in numpy.
#pragma once

struct TaskParams {
    TaskDesc d;
    int vec;              // 1: units are quads of columns (16-byte accesses), 0: single columns
    int staged;           // backward: the member list lives in LDS (task_staged)
    SeedGrid<2> grid;     // backward: copy workgroups, then sum workgroups
    float *table;         // [num_tasks, T]: renormed in place (renorm), read (gather)
    const void *ids;      // ids_len words of id_bytes
    const float *x, *a;   // [R, D], [R, A] or null
    float *out;           // [R, W]
    const float *dout;    // [R, W]
    float *dx, *da, *dtable;  // [R, D], [R, A], [num_tasks, T]; each may be null
};

__device__ __forceinline__ void task_move(float *dst, const float *src, int vec) {
    if (vec) *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(src);
    else *dst = *src;
}

// one wavefront per table row: the workgroup reads the id list once and flags which of its TASK_WAVES rows it names; a named row's
// squares are summed in the documented order and the row is scaled when its norm exceeds max_norm
__global__ __launch_bounds__(TASK_THREADS) void k_task_renorm(TaskParams p) {
    __shared__ int named[TASK_WAVES];
    const TaskDesc &d = p.d;
    const int wave = (int)threadIdx.x / TASK_WAVE, lane = (int)threadIdx.x % TASK_WAVE;
    const int64_t k0 = (int64_t)blockIdx.x * TASK_WAVES;
    if (threadIdx.x < TASK_WAVES) named[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t s = threadIdx.x; s < (uint64_t)d.ids_len; s += TASK_THREADS) {
        const int64_t id = task_id_read(d, p.ids, s);
        if (id >= k0 && id < k0 + TASK_WAVES) named[id - k0] = 1;
    }
    __syncthreads();
    const int64_t k = k0 + wave;
    if (k >= (int64_t)d.num_tasks || !named[wave]) return;
    float *row = p.table + (uint64_t)k * (uint64_t)d.task_dim;
    float s = 0.0f;
    for (int c = lane; c < d.task_dim; c += TASK_WAVE) {
        const float v = row[c];
        s = __fadd_rn(s, __fmul_rn(v, v));
    }
    for (int w = TASK_WAVE / 2; w > 0; w >>= 1) s = __fadd_rn(s, __shfl_down(s, w, TASK_WAVE));  // lane l < w: s_l + s_{l + w}
    const float norm = sqrtf(__shfl(s, 0, TASK_WAVE));
    if (!task_scales(norm, d.max_norm)) return;
    const float scale = task_scale(norm, d.max_norm);
    for (int c = lane; c < d.task_dim; c += TASK_WAVE) row[c] = __fmul_rn(row[c], scale);
}

// out[r, :] = [ x[r] | table[id(r)] | a[r] ] for the TASK_ROWS rows of the workgroup, whose ids are staged once
__global__ __launch_bounds__(TASK_THREADS) void k_task_gather(TaskParams p) {
    __shared__ int32_t id_of[TASK_ROWS];
    const TaskDesc &d = p.d;
    const uint64_t r0 = task_block_row0(blockIdx.x);
    const int n = task_block_rows(d, blockIdx.x);
    if ((int)threadIdx.x < n) id_of[threadIdx.x] = task_id_read(d, p.ids, task_id_slot(d, r0 + threadIdx.x));
    __syncthreads();
    const uint64_t W = task_width(d), D = (uint64_t)d.x_dim, T = (uint64_t)d.task_dim, A = (uint64_t)d.a_dim;
    const int lanes = task_lanes(p.vec != 0);
    const uint64_t units = task_units(n, W, lanes);
    const float nan = __int_as_float(0x7fc00000);
    for (uint64_t u = threadIdx.x; u < units; u += TASK_THREADS) {
        int row;
        uint64_t c, off;
        task_unit(u, W, lanes, row, c);
        const uint64_t r = r0 + (uint64_t)row;
        float *dst = p.out + r * W + c;
        const int seg = task_segment(d, c, off);
        if (seg == 1 && id_of[row] < 0) {  // an id that names no table row: loud, and no access
            for (int i = 0; i < lanes; ++i) dst[i] = nan;
            continue;
        }
        const float *src = seg == 0 ? p.x + r * D + off : seg == 2 ? p.a + r * A + off : p.table + (uint64_t)id_of[row] * T + off;
        task_move(dst, src, p.vec);
    }
}

// copy workgroups: dx / da of TASK_ROWS rows; sum workgroups: TASK_COLS columns of one table row's gradient, one lane per column
__global__ __launch_bounds__(TASK_THREADS) void k_task_backward(TaskParams p) {
    __shared__ int32_t stage[TASK_STAGE];
    __shared__ uint32_t member[TASK_STAGE];
    __shared__ uint32_t count[TASK_THREADS];
    __shared__ float part[TASK_WAVES][TASK_COLS];
    const TaskDesc &d = p.d;
    const uint64_t W = task_width(d), D = (uint64_t)d.x_dim, T = (uint64_t)d.task_dim, A = (uint64_t)d.a_dim, B = (uint64_t)d.batch;
    int kind;
    uint64_t local;
    seed_decode(p.grid, blockIdx.x, kind, local);
    if (kind == 0) {
        const uint64_t r0 = task_block_row0(local);
        const int n = task_block_rows(d, local);
        const int lanes = task_lanes(p.vec != 0);
        for (int part_i = 0; part_i < 2; ++part_i) {
            float *dst = part_i == 0 ? p.dx : p.da;
            if (!dst) continue;
            const uint64_t cols = part_i == 0 ? D : A, first = part_i == 0 ? 0 : D + T;
            const uint64_t units = task_units(n, cols, lanes);
            for (uint64_t u = threadIdx.x; u < units; u += TASK_THREADS) {
                int row;
                uint64_t c;
                task_unit(u, cols, lanes, row, c);
                const uint64_t r = r0 + (uint64_t)row;
                task_move(dst + r * cols + c, p.dout + r * W + first + c, p.vec);
            }
        }
        return;
    }
    int32_t k;
    uint64_t col0;
    task_sum_decode(d, local, k, col0);
    const int tid = (int)threadIdx.x, wave = tid / TASK_WAVE, lane = tid % TASK_WAVE;
    const uint64_t col = col0 + (uint64_t)lane;
    const bool live = col < T;
    const float *src = p.dout + D + col;  // + r * W
    float total = 0.0f;
    if (!p.staged) {  // past TASK_STAGE batch columns: one wave scans the rows in rising order and makes the same additions
        if (wave != 0 || !live) return;
        float s = 0.0f;
        int in_chunk = 0;
        for (uint64_t t = 0; t < (uint64_t)d.steps; ++t)
            for (uint64_t b = 0; b < B; ++b) {
                if (task_id_read(d, p.ids, b) != k) continue;
                s = s + src[(t * B + b) * W];
                if (++in_chunk == TASK_CHUNK) { total = total + s; s = 0.0f; in_chunk = 0; }
            }
        if (in_chunk) total = total + s;
        p.dtable[(uint64_t)k * T + col] = total;
        return;
    }
    uint64_t cnt;
    const bool one = d.ids_len == 1;
    if (one) {
        cnt = task_id_read(d, p.ids, 0) == k ? B : 0;  // member[j] = j
    } else {  // the rising list of the batch columns whose id is k: ids staged once, counted per thread, then written at the offsets
        for (uint64_t b = (uint64_t)tid; b < B; b += TASK_THREADS) stage[b] = task_id_read(d, p.ids, b);
        __syncthreads();
        const uint32_t per = (uint32_t)task_ceil(B, TASK_THREADS);
        const uint32_t b0 = (uint32_t)tid * per, b1 = b0 + per < (uint32_t)B ? b0 + per : (uint32_t)B;
        uint32_t mine = 0;
        for (uint32_t b = b0; b < b1; ++b) mine += stage[b] == k ? 1u : 0u;
        count[tid] = mine;
        __syncthreads();
        uint32_t at = 0, all = 0;
        for (int i = 0; i < TASK_THREADS; ++i) {
            const uint32_t v = count[i];
            at += i < tid ? v : 0u;
            all += v;
        }
        for (uint32_t b = b0; b < b1; ++b)
            if (stage[b] == k) member[at++] = b;
        __syncthreads();
        cnt = all;
    }
    const uint64_t n = task_positions(d, cnt), chunks = task_chunks(n);
    for (uint64_t c0 = 0; c0 < chunks; c0 += TASK_WAVES) {
        const uint64_t ch = c0 + (uint64_t)wave;
        float s = 0.0f;
        if (ch < chunks && live) {
            uint64_t t, j;
            task_position(task_chunk_begin(ch), cnt, t, j);
            const uint64_t end = task_chunk_end(ch, n);
            for (uint64_t q = task_chunk_begin(ch); q < end; ++q, task_position_next(cnt, t, j))
                s = s + src[(t * B + (one ? j : (uint64_t)member[j])) * W];
        }
        part[wave][lane] = s;
        __syncthreads();
        if (wave == 0)
            for (int w = 0; w < TASK_WAVES && c0 + (uint64_t)w < chunks; ++w) total = total + part[w][lane];
        __syncthreads();
    }
    if (wave == 0 && live) p.dtable[(uint64_t)k * T + col] = total;
}
