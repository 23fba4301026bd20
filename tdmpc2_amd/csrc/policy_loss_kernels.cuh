// The tail of TDMPC2.update_pi's forward (tdmpc2/tdmpc2.py:223-239) and the termination statistics of TDMPC2._update
// (common/math.py:97-109), each as ONE workgroup with a fixed order of operations: no float atomics, no workgroup waits for another.
//   k_running_scale      RunningScale.update (common/scale.py): the 5th / 95th percentile of n floats by rank selection, lerp
//   k_policy_loss_tail   qs / scale, the rho-weighted pi_loss and the per-step / overall means
//   k_termination_stats  rate and F1 from integer tp / fn / fp counts
// Included by k_policy_loss.hip inside its anonymous namespace.
#pragma once

// The reference rounds every product and sum of these formulas separately.  hipcc's default contraction fuses a * b + c * d into
// an FMA even through the __f*_rn forms (plain operators in the HIP headers, compiled under that default whatever the caller's
// pragma says), so the forms used here carry the pragma themselves.
__device__ __forceinline__ float pl_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float pl_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float pl_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float pl_div(float a, float b) {
#pragma clang fp contract(off)
    return a / b;
}

// sum over the workgroup in a fixed order (wavefront butterfly, then the wavefronts' sums in index order); every thread gets it
template <typename T>
__device__ __forceinline__ T pl_block_sum(T v, T *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();  // `red` may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
    return s;
}

// torch.sort's order as an unsigned key: -inf < ... < -0 < +0 < ... < +inf < NaN (every NaN, whatever its sign, last)
__device__ __forceinline__ unsigned pl_sort_key(float v) {
    if (v != v) return 0xffffffffu;
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pl_key_value(unsigned k) {
    if (k == 0xffffffffu) return __builtin_nanf("");
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// RunningScale.update.  The keys of x sit in LDS (dynamic: n words); the four order statistics the two percentiles touch are
// found together, bit by bit from the top: the k-th smallest key is the largest v with #{key < v} <= k (32 counting passes,
// integer counts).  Positions and weights in fp32 as scale.py:21-28 forms them; products and sum unfused (scale.py:35-37).
__global__ __launch_bounds__(PL_THREADS) void k_running_scale(RunningScaleParams p) {
#pragma clang fp contract(off)
    extern __shared__ unsigned pl_keys[];
    __shared__ int red[4][PL_THREADS / 64];
    const int tid = threadIdx.x, n = p.n;
    for (int i = tid; i < n; i += PL_THREADS) pl_keys[i] = pl_sort_key(p.x[i]);
    const float last = (float)(n - 1);
    int rank[4];
    float wf[2], wc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float pos = pl_div(pl_mul(j ? 95.f : 5.f, last), 100.f);
        const float fl = floorf(pos);
        float ce = pl_add(fl, 1.f);
        if (ce > last) ce = last;
        wc[j] = pl_sub(pos, fl);
        wf[j] = pl_sub(1.f, wc[j]);
        rank[2 * j] = (int)fl;
        rank[2 * j + 1] = (int)ce;
    }
    unsigned pre[4] = {0u, 0u, 0u, 0u};
    __syncthreads();
    for (int b = 31; b >= 0; --b) {
        unsigned cand[4];
        int cnt[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) cand[j] = pre[j] | (1u << b);
        for (int i = tid; i < n; i += PL_THREADS) {
            const unsigned k = pl_keys[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) cnt[j] += k < cand[j] ? 1 : 0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt[j] += __shfl_xor(cnt[j], o);
        }
        __syncthreads();  // the previous pass's sums have been read
        if ((tid & 63) == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) red[j][tid >> 6] = cnt[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int s = 0;
            for (int w = 0; w < PL_THREADS / 64; ++w) s += red[j][w];
            if (s <= rank[j]) pre[j] = cand[j];
        }
    }
    if (tid != 0) return;
    if (p.err && __hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) {
        // a bounded wait of the layered GEMMs gave up in this call (q is NaN): RunningScale.value keeps its state
        if (p.percentiles) p.percentiles[0] = p.percentiles[1] = __builtin_nanf("");
        return;
    }
    float pc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
        pc[j] = pl_add(pl_mul(pl_key_value(pre[2 * j]), wf[j]), pl_mul(pl_key_value(pre[2 * j + 1]), wc[j]));
    const float d = pl_sub(pc[1], pc[0]);
    const float v = d != d ? d : fmaxf(d, 1.f);  // torch.clamp(min = 1): a NaN stays a NaN
    const float s = *p.scale;
    *p.scale = pl_add(s, pl_mul(p.tau, pl_sub(v, s)));  // lerp_(value, tau)
    if (p.percentiles) {
        p.percentiles[0] = pc[0];
        p.percentiles[1] = pc[1];
    }
}

// tdmpc2.py:224-228: qs / scale, pi_loss = mean_t(-mean_B(entropy_coef * scaled_entropy + qs) * rho^t); the means of the info dict
__global__ __launch_bounds__(256) void k_policy_loss_tail(PolicyLossTailParams p) {
#pragma clang fp contract(off)
    __shared__ float red[256 / 64];
    const float scale = *p.scale;
    float loss = 0.f, ent = 0.f, sent = 0.f;
    // a bounded wait of the layered GEMMs gave up somewhere in this call: EVERY output is NaN (tdmpc2_plan_take_fault)
    if (p.err && __hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) {
        const float nan = __builtin_nanf("");
        for (int i = threadIdx.x; i < p.T * p.B; i += 256) p.q[i] = p.entropy[i] = p.scaled_entropy[i] = nan;
        if (p.action)
            for (size_t i = threadIdx.x; i < (size_t)p.T * p.B * p.A; i += 256) p.action[i] = nan;
        if (p.step_means)
            for (int i = threadIdx.x; i < 3 * p.T; i += 256) p.step_means[i] = nan;
        if (threadIdx.x < 4) p.loss[threadIdx.x] = nan;
        return;
    }
    for (int t = 0; t < p.T; ++t) {
        const size_t o = (size_t)t * p.B;
        float a = 0.f, b = 0.f, c = 0.f, d = 0.f;
        for (int i = threadIdx.x; i < p.B; i += 256) {
            const float qs = pl_div(p.q[o + i], scale), se = p.scaled_entropy[o + i];
            a += pl_add(pl_mul(p.entropy_coef, se), qs);
            b += qs;
            c += se;
            d += p.entropy[o + i];
        }
        a = pl_block_sum(a, red);
        b = pl_block_sum(b, red);
        c = pl_block_sum(c, red);
        d = pl_block_sum(d, red);
        loss += pl_mul(-(a / (float)p.B), p.rho_pow[t]);
        sent += c;
        ent += d;
        if (p.step_means && threadIdx.x == 0) {
            p.step_means[0 * p.T + t] = b / (float)p.B;
            p.step_means[1 * p.T + t] = c / (float)p.B;
            p.step_means[2 * p.T + t] = d / (float)p.B;
        }
    }
    if (threadIdx.x != 0) return;
    const float rows = (float)p.T * (float)p.B;
    p.loss[0] = loss / (float)p.T;
    p.loss[1] = ent / rows;
    p.loss[2] = sent / rows;
    p.loss[3] = scale;
}

// math.termination_statistics(sigmoid(logit), target).  pred = sigmoid > 0.5 with the fp32 sigmoid of the termination heads
// (fused_kernels.cuh head_term_s: 1 / (1 + expf(-x)); x > 0 is not the same set: sigmoid(1e-8f) == 0.5f).
__global__ __launch_bounds__(256) void k_termination_stats(TerminationStatsParams p) {
#pragma clang fp contract(off)
    __shared__ int redi[256 / 64];
    __shared__ float redf[256 / 64];
    int tp = 0, fn = 0, fp = 0;
    float ys = 0.f;
    for (int i = threadIdx.x; i < p.n; i += 256) {
        const float y = p.target[i];
        const bool pred = 1.f / (1.f + expf(-p.logit[i])) > 0.5f;
        tp += (pred && y == 1.f) ? 1 : 0;
        fn += (!pred && y == 1.f) ? 1 : 0;
        fp += (pred && y == 0.f) ? 1 : 0;
        ys += y;
    }
    tp = pl_block_sum(tp, redi);
    fn = pl_block_sum(fn, redi);
    fp = pl_block_sum(fp, redi);
    ys = pl_block_sum(ys, redf);
    if (threadIdx.x != 0) return;
    const float eps = 1e-9f;
    const float recall = pl_div((float)tp, pl_add((float)(tp + fn), eps));
    const float precision = pl_div((float)tp, pl_add((float)(tp + fp), eps));
    p.stats[0] = pl_div(ys, (float)p.n);
    p.stats[1] = pl_div(pl_mul(2.f, pl_mul(precision, recall)), pl_add(pl_add(precision, recall), eps));
}
