// Kernels of the replay buffer (included by k_buffer.hip inside its anonymous namespace).  Geometry and arithmetic: buffer_route.h.
//   k_buf_update  the table / state words after an add or a bulk load: the new values arrive BY VALUE (stream-ordered, no host
//                 staging buffer); new entries are filled arithmetically, one thread each
//   k_buf_draw    one thread per slice: Philox draw -> table entry -> logical start of the slice, to the workspace and index_out
//   k_buf_gather  ONE grouped launch over every field: workgroup -> (field, output row(s), chunk) through the table in the
//                 kernel arguments; 16-byte, 4-byte or byte accesses per field; advances the call counter
// No workgroup waits for another, no atomics: every word has one writer per launch.

// device state words (uint32): head, count of the table ring, and the call counter mixed into the Philox counter
enum { BST_HEAD = 0, BST_COUNT = 1, BST_CALL = 2, BST_WORDS = 4 };
constexpr unsigned long long BUF_NO_SLICE = ~0ull;  // a draw that met an empty table

struct BufUpdateParams {
    BufUpdate u;
    uint32_t tcap;
    BufEntry *table;
    uint32_t *state;
};
__global__ __launch_bounds__(BUF_THREADS) void k_buf_update(const BufUpdateParams p) {
    const uint32_t i = blockIdx.x * BUF_THREADS + threadIdx.x;
    if (i < p.u.n_push) p.table[(p.u.push_slot + i) % p.tcap] = buf_pushed_entry(p.u, i);
    if (i == 0) {
        if (p.u.shrink) p.table[p.u.head] = BufEntry{p.u.shrink_first, p.u.shrink_len, 0u};
        p.state[BST_HEAD] = p.u.head;
        p.state[BST_COUNT] = p.u.count;
    }
}
__global__ void k_buf_set_call(uint32_t *state, uint32_t call) {
    if (blockIdx.x == 0 && threadIdx.x == 0) state[BST_CALL] = call;
}

struct BufDrawParams {
    const BufEntry *table;
    const uint32_t *state;
    uint32_t tcap, S, B;
    unsigned long long seed;
    unsigned long long *starts;  // [B] logical index of step 0 of every slice (BUF_NO_SLICE: empty table)
    long long *index_out;        // [B] or null
};
__global__ __launch_bounds__(BUF_THREADS) void k_buf_draw(const BufDrawParams p) {
    const uint32_t b = blockIdx.x * BUF_THREADS + threadIdx.x;
    if (b >= p.B) return;
    const uint32_t head = p.state[BST_HEAD], count = p.state[BST_COUNT], call = p.state[BST_CALL];
    if (count == 0 || count > p.tcap || head >= p.tcap) {  // nothing eligible: the gather leaves the outputs untouched
        p.starts[b] = BUF_NO_SLICE;
        if (p.index_out) p.index_out[b] = -1;
        return;
    }
    const uint4 r = rng_raw(p.seed, call, SITE_BUFFER, 0, 0, b);
    const BufEntry e = p.table[(head + buf_draw_episode(r.x, count)) % p.tcap];
    const unsigned long long start = e.first + (e.len >= p.S ? buf_draw_start(r.y, e.len, p.S) : 0u);
    p.starts[b] = start;
    if (p.index_out) p.index_out[b] = (long long)start;
}

struct BufGatherField {
    const unsigned char *src;  // the field's storage: [cap][row_bytes]
    unsigned char *dst;        // [step_count, B, row_bytes]
    uint32_t row_bytes, step_first;
    BufFieldGrid g;
};
struct BufGatherParams {
    BufGatherField f[BUF_MAX_FIELDS];
    uint32_t blk0[BUF_MAX_FIELDS + 1];  // first workgroup of every field; [n_fields] = the grid
    uint64_t rows[BUF_MAX_FIELDS];      // output rows of the field: step_count x B
    uint32_t n_fields, B;
    uint64_t cap;
    const unsigned long long *starts;
    uint32_t *state;
};
template <typename V>
__device__ __forceinline__ void buf_copy_rows(const BufGatherParams &p, const BufGatherField &fd, const BufWork w) {
    // the access of index u: row w.row0 + u / nunits, unit w.unit0 + u % nunits; up to 3 loads in flight per thread
    const uint32_t total = w.nrows * w.nunits;
    constexpr int U = BUF_CHUNK_UNITS / BUF_THREADS;
    for (uint32_t u0 = threadIdx.x; u0 < total; u0 += U * BUF_THREADS) {
        V v[U];
        unsigned char *d[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const uint32_t u = u0 + k * BUF_THREADS;
            d[k] = nullptr;
            if (u >= total) continue;
            const uint64_t o = w.row0 + u / w.nunits;
            const uint32_t unit = w.unit0 + u % w.nunits;
            const unsigned long long start = p.starts[o % p.B];
            if (start == BUF_NO_SLICE) continue;
            const uint64_t phys = (start + fd.step_first + o / p.B) % p.cap;
            v[k] = *reinterpret_cast<const V *>(fd.src + buf_offset(0, phys, fd.row_bytes) + (uint64_t)unit * sizeof(V));
            d[k] = fd.dst + o * (uint64_t)fd.row_bytes + (uint64_t)unit * sizeof(V);
        }
#pragma unroll
        for (int k = 0; k < U; ++k)
            if (d[k]) *reinterpret_cast<V *>(d[k]) = v[k];
    }
}
__global__ __launch_bounds__(BUF_THREADS) void k_buf_gather(const BufGatherParams p) {
    const uint32_t blk = blockIdx.x;
    if (blk == 0 && threadIdx.x == 0) p.state[BST_CALL] = p.state[BST_CALL] + 1u;  // nothing in this launch reads it
    uint32_t f = 0;
    while (f + 1 < p.n_fields && blk >= p.blk0[f + 1]) ++f;
    const BufGatherField &fd = p.f[f];
    const BufWork w = buf_decode(fd.g, p.rows[f], blk - p.blk0[f]);
    if (w.row0 >= p.rows[f]) return;
    if (fd.g.width == 16) buf_copy_rows<uint4>(p, fd, w);
    else if (fd.g.width == 4) buf_copy_rows<uint32_t>(p, fd, w);
    else buf_copy_rows<unsigned char>(p, fd, w);
}
