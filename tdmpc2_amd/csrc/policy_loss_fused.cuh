// ks_value_ent: update_pi's forward per row (tdmpc2/tdmpc2.py:221-222) on the fused family -- ks_value (fused_kernels.cuh) for
// the online ensemble with 'avg', plus the entropy terms of WorldModel.pi per row and the row -> task map of a [steps + 1, B]
// batch.  A kernel of its own so that ks_value and the planner's kernels keep the code they have.  Same chains, same order: the
// action and q carry policy_value's bits.  Included by k_policy_loss.hip after fused_kernels.cuh.
#pragma once

// head_pi_rows_s on a training batch, with the entropy terms of WorldModel.pi (world_model.py:165-182; math.py:16-29) per row:
// each of a row's 8 lanes sums its action dimensions, three xor-shuffles finish the row.  The action takes head_pi_rows_s's
// expressions (the same bits); the sums are written in the forms of pol_head (policy_kernels.cuh) -- which the compiler may still
// contract into FMAs (the __f*_rn forms are plain operators in the HIP headers): these terms are gated by tolerance, not by bits.
template <class CT, typename EpsFn>
__device__ __forceinline__ void head_pi_rows_ent_s(const CT &c, int A, int Apad, float lsmin, float lsdif, EpsFn eps, float *gdst,
                                                   int nvalid, const float *mask_tab, const int *row_task, float *entropy,
                                                   float *scaled_entropy) {
    const int row = c.tid >> 3, part = c.tid & 7;
    const bool live = row < CT::TROWS;
    const float *rp = c.f32() + (live ? row : 0) * c.RSF();
    const float *mask = (mask_tab && live) ? mask_tab + (size_t)row_task[row] * A : nullptr;
    float lp = 0.f, sq = 0.f, size = 0.f;
    if (live)
    for (int a = part; a < Apad; a += 8) {
        float out = 0.f;
        if (a < A) {
            float mu = rp[a], lsr = rp[A + a];
            float ls = lsmin + 0.5f * lsdif * (tanhf(lsr) + 1.f);  // math.log_std, math.py:12-13
            float e = eps(row, a);
            float mk = 1.f;
            if (mask) {
                mk = mask[a];
                mu *= mk;
                ls *= mk;
                e *= mk;
            }
            out = tanhf(mu + e * expf(ls));
            if (gdst && row < nvalid) gdst[row * A + a] = out;
            size += mk;
            lp += __fsub_rn(__fsub_rn(__fmul_rn(-0.5f, __fmul_rn(e, e)), ls), 0.9189385175704956f);
            sq += logf(__fadd_rn(fmaxf(__fsub_rn(1.f, __fmul_rn(out, out)), 0.f), 1e-6f));
        }
        put_action(c, row, a, out);
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {  // (every lane of the wavefront takes part: rows >= TROWS carry zeros)
        lp += __shfl_xor(lp, o);
        sq += __shfl_xor(sq, o);
        size += __shfl_xor(size, o);
    }
    if (part == 0 && row < nvalid) {
        const float slp = __fmul_rn(lp, size);  // log_prob * (A | action_dims)
        const float lq = __fsub_rn(lp, sq);     // math.squash
        entropy[row] = -lq;
        scaled_entropy[row] = __fmul_rn(-lq, __fdiv_rn(slp, __fadd_rn(lq, 1e-8f)));
    }
    __syncthreads();
}

template <int APAD, int AR>
__global__ __launch_bounds__(NTHREADS, 2) void ks_value_ent(ValueEntParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    typedef CtxT<APAD, 2, 8, AR> CT;
    constexpr int TROWS = CT::TROWS, ZKB16 = CT::ZKB;
    CT c{reinterpret_cast<_Float16 *>(smem), smem + TROWS * CT::RSF(), smem + TROWS * CT::RSF() + 1024, tid,
         __builtin_amdgcn_readfirstlane(tid >> 6), tid & 63};
    int *s_task = reinterpret_cast<int *>(smem + TROWS * CT::RSF() + 2048);  // [TROWS] task of each row (multitask)
    const int row0 = blockIdx.x * TROWS;
    const int nvalid = min(TROWS, p.rows - row0);
    const float *zsrc = p.z + (size_t)row0 * WIDTH;
    const int KBA = ZKB16 + p.Apad / CT::KBLK;
    int q0, q1;
    if (p.qidx) {
        q0 = p.qidx[0];
        q1 = p.qidx[1];
    } else {  // randperm(num_q)[:2] (world_model.py:212), one draw per call
        const uint4 r = rng_raw(p.seed, p.call, SITE_QIDX, 0, 0, 0);
        q0 = (int)(r.x % (unsigned)p.nq);
        q1 = (int)(r.y % (unsigned)(p.nq - 1));
        if (q1 >= q0) ++q1;
    }
    if (p.task_ids && tid < TROWS) s_task[tid] = tid < nvalid ? p.task_ids[(row0 + tid) % p.task_mod] : 0;  // rows are [steps + 1, B]
    tile_from_rows_s(c, zsrc, nvalid);
    gb_prefetch(c, p.pi.l[0].g, p.pi.l[0].b);
    epi_barrier(c);
    // first-layer bias vectors of this lane's two sample rows
    const int j = c.lane & 31;
    auto first_layer = [&](const LayerS &ly, int slot, int kb1, GB next) {
        if (!p.task_ids) {
            layer_full_s<0>(c, ly, ly.bias, 0, kb1, next);
            return;
        }
        const float *brow[CT::NST];
#pragma unroll
        for (int st = 0; st < CT::NST; ++st) brow[st] = p.beff_tab + ((size_t)s_task[32 * st + j] * p.nnets + slot) * WIDTH;
        f32x16 acc[CT::NST][CT::FT];
        zero_acc(acc);
        if (next.g) gb_prefetch(c, next.g, next.b);
        kloop_s(c, ly, 0, kb1, acc);
        add_row_bias(c, acc, *ly.oscale, brow);
        epi_t<0, CT, false>(c, acc, 1.f, *ly.ascale, nullptr, next, nullptr);
        epi_barrier(c);
    };
    first_layer(p.pi.l[0], BE_PI, ZKB16, gb_of(p.pi.l[1]));
    layer_full_s<0>(c, p.pi.l[1], p.pi.l[1].bias, 0, ZKB16, gb_of(p.q[q0].l[0]));
    {
        auto eps = [&](int row, int a) -> float {
            const unsigned ridx = (unsigned)((size_t)(row0 + row) * p.A + a);
            if (p.pi_eps) return row < nvalid ? p.pi_eps[ridx] : 0.f;
            return rng_normal(p.seed, p.call, SITE_PI, 0, 0, ridx);
        };
        head_logits_s(c, p.pi.l[2]);
        head_pi_rows_ent_s(c, p.A, p.Apad, p.log_std_min, p.log_std_dif, eps, p.action ? p.action + (size_t)row0 * p.A : nullptr,
                           nvalid, p.task_ids ? p.mask_tab : nullptr, s_task, p.entropy + row0, p.scaled_entropy + row0);
    }
    tile_from_rows_s(c, zsrc, nvalid);  // the hidden layers overwrote the z columns; the action columns stay
    __syncthreads();
    first_layer(p.q[q0].l[0], BE_Q0 + q0, KBA, gb_of(p.q[q0].l[1]));
    layer_full_s<0>(c, p.q[q0].l[1], p.q[q0].l[1].bias, 0, ZKB16, gb_of(p.q[q1].l[0]));
    const float qa = head_twohot_s(c, p.q[q0].l[2], p.bins, p.num_bins);
    tile_from_rows_s(c, zsrc, nvalid);
    __syncthreads();
    first_layer(p.q[q1].l[0], BE_Q0 + q1, KBA, gb_of(p.q[q1].l[1]));
    layer_full_s<0>(c, p.q[q1].l[1], p.q[q1].l[1].bias, 0, ZKB16, GB{});
    const float qb = head_twohot_s(c, p.q[q1].l[2], p.bins, p.num_bins);
    const int row = tid >> 3;
    if ((tid & 7) == 0 && row < nvalid) p.out[row0 + row] = (qa + qb) / 2.f;  // 'avg' (world_model.py:216), unscaled
}
