// Translation unit of the replay buffer (tdmpc2_buffer_*): the kernels of buffer_kernels.cuh and the whole host side of the
// handle -- it shares nothing with a planner handle, so its C ABI lives here and not in the planner's host units (plan_*.hip).  Every decision
// (ring / table arithmetic, draws, access widths, grids, offsets) is buffer_route.h's; this file checks arguments, walks what the
// header returns and launches.
#include "handle.h"
#include "dev_guard.h"
#include "buffer_route.h"

namespace {
using namespace tdk;
#include "buffer_kernels.cuh"
}  // namespace

struct tdmpc2_buffer {
    tdmpc2_buffer_cfg cfg{};
    BufRing ring{};
    std::vector<BufEntry> table;          // host mirror of the device table
    uint64_t field_base[BUF_MAX_FIELDS]{};
    unsigned char *dev = nullptr;         // the one allocation: fields | table | state words | slice starts
    unsigned char *storage = nullptr;
    BufEntry *d_table = nullptr;
    uint32_t *d_state = nullptr;
    unsigned long long *d_starts = nullptr;
    int max_batch = 0;
    uint64_t fields_bytes = 0, table_bytes = 0, state_bytes = 0, starts_bytes = 0;
    uint32_t pending_call = 0;            // set_call_counter before the first write
    std::atomic<bool> busy{false};
};

namespace {
struct BusyGuard {
    tdmpc2_buffer *b;
    bool ok;
    explicit BusyGuard(tdmpc2_buffer *b_) : b(b_), ok(!b_->busy.exchange(true)) {}
    ~BusyGuard() {
        if (ok) b->busy.store(false);
    }
};

// The one device allocation of a handle, made by its first write (create only validates and sizes: it never touches the device).
int buf_reserve(tdmpc2_buffer *b) {
    if (b->dev) return 0;
    const uint64_t tail = b->table_bytes + b->state_bytes + b->starts_bytes, total = b->fields_bytes + tail;
    unsigned char *dev = nullptr;
    hipError_t e = hipMalloc((void **)&dev, total);
    // table, state and starts must read as zero before the first update (an empty table); the storage needs no clearing
    if (e == hipSuccess) e = hipMemset(dev + b->fields_bytes, 0, tail);
    if (e != hipSuccess) {
        if (dev) (void)hipFree(dev);
        (void)hipGetLastError();
        return fail(TDMPC2_ERR_HIP, "replay buffer: %llu bytes of device storage: %s (storage is device memory only)",
                    (unsigned long long)total, hipGetErrorString(e));
    }
    b->dev = b->storage = dev;
    b->d_table = (BufEntry *)(dev + b->fields_bytes);
    b->d_state = (uint32_t *)(dev + b->fields_bytes + b->table_bytes);
    b->d_starts = (unsigned long long *)(dev + b->fields_bytes + b->table_bytes + b->state_bytes);
    if (b->pending_call) {
        e = hipMemcpy(b->d_state + BST_CALL, &b->pending_call, sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(TDMPC2_ERR_HIP, "replay buffer: setting the call counter: %s", hipGetErrorString(e));
    }
    return 0;
}

int buf_write_episodes(tdmpc2_buffer *b, uint64_t n_eps, uint32_t steps, const void *const *fields, void *stream, const char *what) {
    if (!b || !fields) return fail(TDMPC2_ERR_INVALID, "%s: null argument", what);
    if (n_eps < 1 || steps < 1) return fail(TDMPC2_ERR_INVALID, "%s: needs at least one episode of at least one step", what);
    if (steps > b->cfg.capacity)
        return fail(TDMPC2_ERR_INVALID, "%s: an episode of %u steps is longer than the capacity of %llu steps", what, steps,
                    (unsigned long long)b->cfg.capacity);
    if (n_eps > (1ull << 40)) return fail(TDMPC2_ERR_INVALID, "%s: too many episodes", what);
    for (int f = 0; f < b->cfg.n_fields; ++f)
        if (!fields[f]) return fail(TDMPC2_ERR_INVALID, "%s: null pointer for field %d", what, f);
    BusyGuard bg(b);
    if (!bg.ok) return fail(TDMPC2_ERR_STATE, "%s: the handle is in use by another thread", what);
    DevGuard dg(b->cfg.device);
    if (!dg.ok) return fail(TDMPC2_ERR_HIP, "%s: cannot select device %d", what, b->cfg.device);
    if (int rc = buf_reserve(b)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t cursor_before = b->ring.cursor;
    BufUpdateParams up{};
    up.u = buf_write(b->ring, b->table.data(), n_eps, steps);
    up.tcap = b->ring.tcap;
    up.table = b->d_table;
    up.state = b->d_state;
    uint64_t src[2], dst[2], n[2];
    const int pieces = buf_copy_pieces(b->cfg.capacity, cursor_before, up.u, src, dst, n);
    for (int f = 0; f < b->cfg.n_fields; ++f) {
        const uint32_t rb = b->cfg.field[f].row_bytes;
        for (int k = 0; k < pieces; ++k)
            HIP_TRY(hipMemcpyAsync(b->storage + buf_offset(b->field_base[f], dst[k], rb),
                                   (const unsigned char *)fields[f] + src[k] * (uint64_t)rb, n[k] * (uint64_t)rb,
                                   hipMemcpyDeviceToDevice, st));
    }
    const uint32_t blocks = up.u.n_push > BUF_THREADS ? (up.u.n_push + BUF_THREADS - 1) / BUF_THREADS : 1u;
    hipLaunchKernelGGL(k_buf_update, dim3(blocks), dim3(BUF_THREADS), 0, st, up);
    LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" {

int tdmpc2_buffer_create(const tdmpc2_buffer_cfg *cfg, tdmpc2_buffer_t **out) {
    if (!cfg || !out) return fail(TDMPC2_ERR_INVALID, "buffer_create: null argument");
    *out = nullptr;
    const tdmpc2_buffer_cfg &c = *cfg;
    if (c.slice_len < 2) return fail(TDMPC2_ERR_INVALID, "buffer_create: slice_len %d < 2 (horizon + 1)", c.slice_len);
    if (c.capacity < (uint64_t)c.slice_len)
        return fail(TDMPC2_ERR_INVALID, "buffer_create: capacity %llu < slice_len %d", (unsigned long long)c.capacity, c.slice_len);
    if (c.capacity > (1ull << 40)) return fail(TDMPC2_ERR_INVALID, "buffer_create: capacity %llu too large", (unsigned long long)c.capacity);
    if (c.n_fields < 1 || c.n_fields > TDMPC2_BUFFER_MAX_FIELDS)
        return fail(TDMPC2_ERR_INVALID, "buffer_create: n_fields %d outside [1, %d]", c.n_fields, TDMPC2_BUFFER_MAX_FIELDS);
    if (c.max_batch < 0) return fail(TDMPC2_ERR_INVALID, "buffer_create: max_batch %d < 0", c.max_batch);
    uint32_t rbs[BUF_MAX_FIELDS];
    for (int f = 0; f < c.n_fields; ++f) {
        const tdmpc2_buffer_field &fd = c.field[f];
        if (fd.row_bytes == 0) return fail(TDMPC2_ERR_INVALID, "buffer_create: field %d has row_bytes 0", f);
        if (fd.step_first < 0 || fd.step_count < 1 || fd.step_first + (int64_t)fd.step_count > c.slice_len)
            return fail(TDMPC2_ERR_INVALID, "buffer_create: field %d delivers steps [%d, %d + %d) outside the slice of %d", f,
                        fd.step_first, fd.step_first, fd.step_count, c.slice_len);
        rbs[f] = fd.row_bytes;
    }
    tdmpc2_buffer *b = new (std::nothrow) tdmpc2_buffer();
    if (!b) return fail(TDMPC2_ERR_HIP, "buffer_create: out of host memory");
    b->cfg = c;
    b->max_batch = c.max_batch ? c.max_batch : 4096;
    b->ring = buf_ring_init(c.capacity, (uint32_t)c.slice_len);
    const uint64_t fields_bytes = buf_field_bases(c.capacity, c.n_fields, rbs, b->field_base);
    const uint64_t table_bytes = buf_align_up((uint64_t)b->ring.tcap * sizeof(BufEntry));
    const uint64_t state_bytes = buf_align_up(BST_WORDS * sizeof(uint32_t));
    const uint64_t starts_bytes = buf_align_up((uint64_t)b->max_batch * sizeof(unsigned long long));
    try {
        b->table.assign(b->ring.tcap, BufEntry{});
    } catch (...) {
        delete b;
        return fail(TDMPC2_ERR_HIP, "buffer_create: out of host memory for the table mirror");
    }
    b->fields_bytes = fields_bytes;
    b->table_bytes = table_bytes;
    b->state_bytes = state_bytes;
    b->starts_bytes = starts_bytes;
    *out = b;
    return 0;
}

void tdmpc2_buffer_destroy(tdmpc2_buffer_t *b) {
    if (!b) return;
    {
        DevGuard dg(b->cfg.device);
        if (b->dev) (void)hipFree(b->dev);
    }
    delete b;
}

int tdmpc2_buffer_add(tdmpc2_buffer_t *b, uint32_t steps, const void *const *fields, void *stream) {
    return buf_write_episodes(b, 1, steps, fields, stream, "buffer_add");
}

int tdmpc2_buffer_load(tdmpc2_buffer_t *b, uint64_t n_episodes, uint32_t steps, const void *const *fields, void *stream) {
    return buf_write_episodes(b, n_episodes, steps, fields, stream, "buffer_load");
}

int tdmpc2_buffer_sample(tdmpc2_buffer_t *b, int32_t batch, void *const *outs, int64_t *index_out, uint64_t seed, void *stream) {
    if (!b || !outs) return fail(TDMPC2_ERR_INVALID, "buffer_sample: null argument");
    if (batch < 1 || batch > b->max_batch)
        return fail(TDMPC2_ERR_INVALID, "buffer_sample: batch %d outside [1, %d] (max_batch of the handle)", batch, b->max_batch);
    BusyGuard bg(b);
    if (!bg.ok) return fail(TDMPC2_ERR_STATE, "buffer_sample: the handle is in use by another thread");
    if (b->ring.count == 0)
        return fail(TDMPC2_ERR_STATE, "buffer_sample: no episode with at least %d live steps (%llu episodes written)", b->cfg.slice_len,
                    (unsigned long long)b->ring.num_eps);
    DevGuard dg(b->cfg.device);
    if (!dg.ok) return fail(TDMPC2_ERR_HIP, "buffer_sample: cannot select device %d", b->cfg.device);
    hipStream_t st = (hipStream_t)stream;

    BufDrawParams dp{};
    dp.table = b->d_table;
    dp.state = b->d_state;
    dp.tcap = b->ring.tcap;
    dp.S = b->ring.S;
    dp.B = (uint32_t)batch;
    dp.seed = seed;
    dp.starts = b->d_starts;
    dp.index_out = (long long *)index_out;
    hipLaunchKernelGGL(k_buf_draw, dim3((batch + BUF_THREADS - 1) / BUF_THREADS), dim3(BUF_THREADS), 0, st, dp);
    LAUNCH_CHECK();

    BufGatherParams gp{};
    gp.n_fields = (uint32_t)b->cfg.n_fields;
    gp.B = (uint32_t)batch;
    gp.cap = b->cfg.capacity;
    gp.starts = b->d_starts;
    gp.state = b->d_state;
    uint64_t blocks = 0;
    for (int f = 0; f < b->cfg.n_fields; ++f) {
        const tdmpc2_buffer_field &fd = b->cfg.field[f];
        BufGatherField &g = gp.f[f];
        g.src = b->storage + b->field_base[f];
        g.dst = (unsigned char *)outs[f];
        g.row_bytes = fd.row_bytes;
        g.step_first = (uint32_t)fd.step_first;
        gp.rows[f] = outs[f] ? (uint64_t)fd.step_count * (uint64_t)batch : 0;
        g.g = buf_field_grid(fd.row_bytes, (uint64_t)(uintptr_t)g.src | (uint64_t)(uintptr_t)g.dst, gp.rows[f]);
        gp.blk0[f] = (uint32_t)blocks;
        blocks += g.g.blocks;
    }
    if (blocks > 0x7fffffffull) return fail(TDMPC2_ERR_UNSUPPORTED, "buffer_sample: %llu workgroups in one launch", (unsigned long long)blocks);
    gp.blk0[b->cfg.n_fields] = (uint32_t)blocks;
    // (a call that wants no field still advances the counter: one workgroup)
    hipLaunchKernelGGL(k_buf_gather, dim3(blocks ? (uint32_t)blocks : 1u), dim3(BUF_THREADS), 0, st, gp);
    LAUNCH_CHECK();
    return 0;
}

int tdmpc2_buffer_stats(tdmpc2_buffer_t *b, tdmpc2_buffer_info *info, void *stream) {
    if (!b || !info) return fail(TDMPC2_ERR_INVALID, "buffer_stats: null argument");
    uint32_t words[BST_WORDS] = {0, 0, b->pending_call, 0};
    if (b->dev) {
    DevGuard dg(b->cfg.device);
    if (!dg.ok) return fail(TDMPC2_ERR_HIP, "buffer_stats: cannot select device %d", b->cfg.device);
    HIP_TRY(hipMemcpyAsync(words, b->d_state, sizeof words, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    }
    info->num_eps = b->ring.num_eps;
    info->live_steps = b->ring.cursor - b->ring.floor;
    info->cursor = b->ring.cursor;
    info->eligible = b->ring.count;
    info->next_call = words[BST_CALL];
    return 0;
}

int tdmpc2_buffer_set_call_counter(tdmpc2_buffer_t *b, uint32_t next_call, void *stream) {
    if (!b) return fail(TDMPC2_ERR_INVALID, "buffer_set_call_counter: null argument");
    if (!b->dev) {  // nothing on the device yet: the first write carries it over
        b->pending_call = next_call;
        return 0;
    }
    DevGuard dg(b->cfg.device);
    if (!dg.ok) return fail(TDMPC2_ERR_HIP, "buffer_set_call_counter: cannot select device %d", b->cfg.device);
    hipLaunchKernelGGL(k_buf_set_call, dim3(1), dim3(64), 0, (hipStream_t)stream, b->d_state, next_call);
    LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
