// Fused 512-wide family: the open-loop latent rollout and the prediction chains of TDMPC2._update's forward half
// (tdmpc2/tdmpc2.py:268-283) on the layer code of fused_kernels.cuh (layer_full_s, kloop_s, head_logits_s, tile_from_rows_s).
//   ks_value_roll    one workgroup per 64-row tile: zs[t+1] = next(zs[t], a[t]) (world_model.py:114-121) on RECORDED actions, every
//                   new latent stored to zs in HBM.  The only loop over steps of the whole call.
//   ks_value_chain  one workgroup per (row tile, step, chain): a chain is the reward head (world_model.py:123-130), ONE of the
//                   num_q Q heads (world_model.py:186-210, return_type='all') or the termination head (world_model.py:132-141) on
//                   [zs[t] | a[t]] read back from HBM.  A training batch of 256 rows and H = 3 with 5 Q heads is 4 x 3 x 6 = 72
//                   workgroups here instead of 4 walking 18 chains each.  The head's logits are stored when asked for; the
//                   value (two_hot_inv) and the row's loss term come from the logits while they are still in LDS.
// No workgroup waits for another: the two launches are ordered by the stream.
// Both kernels are members of the ks_value family (rows of a training batch on the fused layer code, one task per row) and carry
// its name: they inline the same hand-ordered weight ring (kloop_asm), whose flag-dependent counted waits the ISA scan
// (tools/isa_hazards.py) cannot follow and tests/test_isa_hazards.py therefore exempts per family; the ring's schedule is checked by
// tests/test_ring_schedule.py.  They add no inline assembly of their own.
// Included by k_model.hip inside its anonymous namespace, after fused_kernels.cuh and model_rows.cuh.
#pragma once

// recorded actions of one step -> the operand-form action columns (zero past A and for rows >= nvalid)
template <class CT>
__device__ __forceinline__ void model_put_actions(const CT &c, const float *src, int A, int Apad, int nvalid) {
    for (int idx = c.tid; idx < CT::TROWS * Apad; idx += CT::NTHR) {
        const int row = idx / Apad, a = idx % Apad;
        put_action(c, row, a, (a < A && row < nvalid) ? src[(size_t)row * A + a] : 0.f);
    }
}

// operand-form z columns of the tile -> fp32 rows in global (split arithmetic: hi + lo, the 22 bits the next layer contracts)
template <class CT>
__device__ __forceinline__ void model_store_z(const CT &c, float *dst, int nvalid) {
    for (int idx = c.tid; idx < CT::TROWS * (WIDTH / 4); idx += CT::NTHR) {
        const int row = idx / (WIDTH / 4), c4 = idx % (WIDTH / 4);
        if (row >= nvalid) continue;
        f32x4 y;
        if constexpr (CT::ARITH == 1) {
            y = *reinterpret_cast<const f32x4 *>(c.f32() + row * CT::RSF() + 4 * c4);
        } else {
            const _Float16 *hp = c.act + row * c.RSH + 4 * c4;
            const f16x4 hi = *reinterpret_cast<const f16x4 *>(hp), lo = *reinterpret_cast<const f16x4 *>(hp + c.SH);
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = ((float)hi[e] + (float)lo[e]) * (1.0f / ACT_SCALE);
        }
        *reinterpret_cast<f32x4 *>(dst + (size_t)row * WIDTH + 4 * c4) = y;
    }
}

// a first layer over [z | a] (kb1 k-blocks): the layer's own bias, or -- multitask batches, one task per row
// (world_model.py:95-97) -- the row's vector of the per-task table, as ks_value does
template <class CT>
__device__ __forceinline__ void model_first_layer_s(const CT &c, const LayerS &ly, const float *beff_tab, const int *s_task, int nnets,
                                                    int slot, int kb1, GB next) {
    if (!beff_tab) {
        layer_full_s<0>(c, ly, ly.bias, 0, kb1, next);
        return;
    }
    const int j = c.lane & 31;
    const float *brow[CT::NST];
#pragma unroll
    for (int st = 0; st < CT::NST; ++st) brow[st] = beff_tab + ((size_t)s_task[32 * st + j] * nnets + slot) * WIDTH;
    f32x16 acc[CT::NST][CT::FT];
    zero_acc(acc);
    if (next.g) gb_prefetch(c, next.g, next.b);
    kloop_s(c, ly, 0, kb1, acc);
    add_row_bias(c, acc, *ly.oscale, brow);
    epi_t<0, CT, false>(c, acc, 1.f, *ly.ascale, nullptr, next, nullptr);
    epi_barrier(c);
}

template <int APAD, int AR>
__global__ __launch_bounds__(NTHREADS, 2) void ks_value_roll(ModelParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    typedef CtxT<APAD, 2, 8, AR> CT;
    constexpr int TROWS = CT::TROWS, ZKB16 = CT::ZKB;
    CT c{reinterpret_cast<_Float16 *>(smem), smem + TROWS * CT::RSF(), smem + TROWS * CT::RSF() + 1024, tid,
         __builtin_amdgcn_readfirstlane(tid >> 6), tid & 63};
    int *s_task = reinterpret_cast<int *>(smem + TROWS * CT::RSF() + 2048);  // [TROWS] task of each row (multitask)
    const int row0 = blockIdx.x * TROWS;
    const int nvalid = min(TROWS, p.B - row0);
    const int KBA = ZKB16 + p.Apad / CT::KBLK;
    if (p.task_ids && tid < TROWS) s_task[tid] = tid < nvalid ? p.task_ids[row0 + tid] : 0;
    tile_from_rows_s(c, p.z0 + (size_t)row0 * WIDTH, nvalid);
    gb_prefetch(c, p.dyn.l[0].g, p.dyn.l[0].b);
    for (int t = 0; t < p.steps; ++t) {
        model_put_actions(c, p.actions + ((size_t)t * p.B + row0) * p.A, p.A, p.Apad, nvalid);
        if (t == 0) epi_barrier(c);
        else __syncthreads();
        model_first_layer_s(c, p.dyn.l[0], p.beff_tab, s_task, p.nnets, BE_DYN, KBA, gb_of(p.dyn.l[1]));
        layer_full_s<0>(c, p.dyn.l[1], p.dyn.l[1].bias, 0, ZKB16, gb_of(p.dyn.l[2]));
        layer_full_s<1>(c, p.dyn.l[2], p.dyn.l[2].bias, 0, ZKB16, gb_of(p.dyn.l[0]));
        model_store_z(c, p.zs + ((size_t)(t + 1) * p.B + row0) * WIDTH, nvalid);
    }
}

template <int APAD, int AR>
__global__ __launch_bounds__(NTHREADS, 2) void ks_value_chain(ModelParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    typedef CtxT<APAD, 2, 8, AR> CT;
    constexpr int TROWS = CT::TROWS, ZKB16 = CT::ZKB;
    CT c{reinterpret_cast<_Float16 *>(smem), smem + TROWS * CT::RSF(), smem + TROWS * CT::RSF() + 1024, tid,
         __builtin_amdgcn_readfirstlane(tid >> 6), tid & 63};
    int *s_task = reinterpret_cast<int *>(smem + TROWS * CT::RSF() + 2048);
    const int t = blockIdx.y, chain = p.chain[blockIdx.z];
    const int row0 = blockIdx.x * TROWS;
    const int nvalid = min(TROWS, p.B - row0);
    const bool is_term = chain == MC_TERM;
    LayerS l0, l1, l2;
    int slot = -1, kind = MK_TERM;
    if (is_term) {
        l0 = p.term.l[0]; l1 = p.term.l[1]; l2 = p.term.l[2];
    } else if (chain == MC_REWARD) {
        l0 = p.rew.l[0]; l1 = p.rew.l[1]; l2 = p.rew.l[2];
        slot = BE_REW; kind = MK_REW;
    } else {
        const int i = chain - MC_Q0;
        l0 = p.q[i].l[0]; l1 = p.q[i].l[1]; l2 = p.q[i].l[2];
        slot = BE_Q0 + i; kind = MK_Q0 + i;
    }
    if (p.task_ids && tid < TROWS) s_task[tid] = tid < nvalid ? p.task_ids[row0 + tid] : 0;
    tile_from_rows_s(c, p.zs + ((size_t)t * p.B + row0) * WIDTH, nvalid);
    if (!is_term) model_put_actions(c, p.actions + ((size_t)t * p.B + row0) * p.A, p.A, p.Apad, nvalid);
    gb_prefetch(c, l0.g, l0.b);
    epi_barrier(c);
    // the termination head reads the latent alone (world_model.py:137-140) and has no task columns (single-task handles only)
    model_first_layer_s(c, l0, is_term ? nullptr : p.beff_tab, s_task, p.nnets, slot, is_term ? ZKB16 : ZKB16 + p.Apad / CT::KBLK,
                        gb_of(l1));
    layer_full_s<0>(c, l1, l1.bias, 0, ZKB16, GB{});
    head_logits_s(c, l2);  // fp32 logits in the staging view of the tile; ends with a barrier
    const int row = tid >> 3, part = tid & 7;
    const bool ok = row < nvalid;
    const float *rp = c.f32() + row * c.RSF();
    const size_t grow = (size_t)t * p.B + row0 + row;  // row of the [H (+1), B] outputs
    const ModelLossArgs &ls = p.ls;
    if (is_term) {
        if (ok && part == 0) {
            const float x = rp[0];
            if (p.out.term_logit) p.out.term_logit[grow] = x;
            if (ls.rowloss && t > 0) ls.rowloss[(size_t)MK_TERM * ls.HB + grow - p.B] = model_bce(x, ls.t_term[grow - p.B]);
        }
        return;
    }
    const int nbc = ls.num_bins > 1 ? ls.num_bins : 1;
    const size_t orow = chain == MC_REWARD ? grow : (size_t)(chain - MC_Q0) * p.H * p.B + grow;  // q outputs: [num_q, H, B]
    float *lg_out = chain == MC_REWARD ? p.out.rew_logits : p.out.q_logits;
    float *val_out = chain == MC_REWARD ? p.out.rew : p.out.q;
    if (lg_out && ok)
        for (int j = part; j < nbc; j += 8) lg_out[orow * nbc + j] = rp[j];
    float lse, val;
    model_row_stats<8>(rp, part, ls.num_bins, ls.bins, lse, val);
    if (ok && part == 0) {
        if (val_out) val_out[orow] = val;
        if (ls.rowloss) ls.rowloss[(size_t)kind * ls.HB + grow] = model_soft_ce(rp, lse, (chain == MC_REWARD ? ls.t_reward : ls.t_td)[grow], ls);
    }
}
