// l_pi_head_ent: the layered family's policy head row kernel (l_pi_head / l_pi_head_s) with the entropy terms of WorldModel.pi
// (world_model.py:165-182; math.py:16-29) per row, for tdmpc2_plan_policy_loss.  One wavefront per row instead of one thread per
// (row, a): the action takes l_pi_head's expressions (the same bits), the row's sums finish with a wavefront butterfly.  A kernel
// of its own: the planner's, td_target's and policy_value's launches keep l_pi_head.  Included by k_layered.hip.
#pragma once

template <bool SPLIT>
__global__ __launch_bounds__(256) void l_pi_head_ent(PiHeadParams p, float *entropy, float *scaled_entropy) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= p.rows) return;  // (wavefront-uniform)
    const int e = row / p.rows_per_env, n = row % p.rows_per_env;
    const float *lr = p.lg + (size_t)row * p.ld;
    float lp = 0.f, sq = 0.f, size = 0.f;
    for (int a = lane; a < p.A; a += 64) {
        float mu = lr[a];
        float ls = p.lsmin + 0.5f * p.lsdif * (tanhf(lr[p.A + a]) + 1.f);
        float eps = 0.f;
        if (n < p.nvalid) {
            const unsigned ridx = (unsigned)((size_t)(n + p.n_off) * p.A + a);
            eps = p.eps ? p.eps[(size_t)e * p.eps_estride + ridx] : rng_normal(p.seed, p.call, p.site, p.iter, e, ridx);
        }
        float mk = 1.f;
        if (p.mask) {
            mk = p.mask[(size_t)(p.row_env ? p.row_env[row] : e) * p.A + a];
            mu *= mk;
            ls *= mk;
            eps *= mk;
        }
        const float act = tanhf(mu + eps * expf(ls));
        if constexpr (SPLIT) put_split(reinterpret_cast<char *>(p.X), p.ldx / 16, (size_t)row, p.L + a, act);
        else p.X[(size_t)row * p.ldx + p.L + a] = act;
        if (p.actions && n < p.nvalid) p.actions[(((size_t)e * p.H + p.t) * p.N + n) * p.A + a] = act;
        size += mk;
        lp += (-0.5f * (eps * eps) - ls) - 0.9189385175704956f;             // math.gaussian_logprob
        sq += logf(fmaxf(1.f - act * act, 0.f) + 1e-6f);                    // math.squash
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lp += __shfl_xor(lp, o);
        sq += __shfl_xor(sq, o);
        size += __shfl_xor(size, o);
    }
    if (lane == 0 && n < p.nvalid) {
        const float slp = lp * size;  // log_prob * (A | action_dims)
        const float lq = lp - sq;
        entropy[row] = -lq;
        scaled_entropy[row] = -lq * (slp / (lq + 1e-8f));
    }
}
