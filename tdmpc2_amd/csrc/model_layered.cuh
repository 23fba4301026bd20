// Layered family: row kernels of the model rollout / loss entry points (host side: model_layered_host.cuh; row math:
// model_rows.cuh).  Included by k_layered.hip inside its anonymous namespace, after layered_split.cuh.
#pragma once
#include "model_rows.cuh"

// The latent a dynamics step wrote into X's z columns -> fp32 rows of zs (world_model.py:114-121).  Split arithmetic: X is the
// fragment-packed operand buffer, the value is hi + lo (the 22 bits the next layer contracts).  One thread per element.
__global__ void l_model_get_z(ModelGetZParams p) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)p.rows * p.L) return;
    const size_t row = idx / p.L;
    const int col = (int)(idx % p.L);
    float v;
    if (p.split) {
        const _Float16 *o = reinterpret_cast<const _Float16 *>(reinterpret_cast<const char *>(p.X) + opnd_off(row, col, p.ldx / 16));
        v = ((float)o[0] + (float)o[512]) * (1.0f / ACT_SCALE);
    } else {
        v = p.X[row * p.ldx + col];
    }
    if (p.err && __hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) v = __builtin_nanf("");
    p.out[idx] = v;
}

// One head's logits (reward, one Q head, or the termination logit in column 0) -> the optional logits / value outputs and the
// row's loss term.  One wavefront per row.
__global__ __launch_bounds__(RW_THREADS) void l_model_head_rows(ModelHeadRowsParams p) {
    const int row = blockIdx.x * (RW_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= p.rows) return;
    const float *rp = p.lg + (size_t)row * p.ld;
    const ModelLossArgs &ls = p.ls;
    const bool bad = ls.err && __hip_atomic_load(ls.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
    const float nan = __builtin_nanf("");
    const long grow = p.row0 + row;
    if (p.kind == MK_TERM) {
        if (lane != 0) return;
        const float x = bad ? nan : rp[0];
        if (p.val_out) p.val_out[grow] = x;
        if (ls.rowloss && grow >= p.B) ls.rowloss[(size_t)MK_TERM * ls.HB + grow - p.B] = model_bce(x, ls.t_term[grow - p.B]);
        return;
    }
    const int nbc = ls.num_bins > 1 ? ls.num_bins : 1;
    if (p.logits_out)
        for (int j = lane; j < nbc; j += 64) p.logits_out[(size_t)grow * nbc + j] = bad ? nan : rp[j];
    float lse, val;
    model_row_stats<64>(rp, lane, ls.num_bins, ls.bins, lse, val);
    if (lane != 0) return;
    if (p.val_out) p.val_out[grow] = bad ? nan : val;
    if (ls.rowloss)
        ls.rowloss[(size_t)p.kind * ls.HB + grow] = bad ? nan : model_soft_ce(rp, lse, (p.kind == MK_REW ? ls.t_reward : ls.t_td)[grow], ls);
}
