// Row math of the model rollout / loss entry points, shared by the fused family's chain kernel (8 lanes per row, logits in
// LDS) and the layered family's row kernels (64 lanes per row, logits in HBM).  Plain fp32 in plain C++ whatever the handle's
// contraction arithmetic.  Reference: tdmpc2/common/math.py:5-9 (soft_ce), 42-47 (symlog), 58-71 (two_hot), 74-83
// (two_hot_inv); torch.nn.functional.binary_cross_entropy_with_logits (tdmpc2/tdmpc2.py:297).
// Included inside an anonymous namespace by k_model.hip and k_layered.hip.
#pragma once

// log-sum-exp of one row of logits and two_hot_inv of it; G lanes of a row, lane `part` reads columns part, part + G, ...
// Every lane of the group gets both results.  num_bins <= 1: the regression heads (lse is unused there: 0).
template <int G>
__device__ __forceinline__ void model_row_stats(const float *rp, int part, int num_bins, const float *bins, float &lse, float &val) {
    if (num_bins <= 1) {
        lse = 0.f;
        val = num_bins == 0 ? rp[0] : symexp_f(rp[0]);
        return;
    }
    float m = -INFINITY;
    for (int j = part; j < num_bins; j += G) m = fmaxf(m, rp[j]);
    m = group_max<G>(m);
    float es = 0.f, x = 0.f;
    for (int j = part; j < num_bins; j += G) {
        const float ev = expf(rp[j] - m);
        es += ev;
        x = fmaf(ev, bins[j], x);
    }
    es = group_sum<G>(es);
    x = group_sum<G>(x);
    lse = m + logf(es);
    val = symexp_f(x / es);
}

// math.py:42-47: sign(x) * log(1 + |x|); +-0 and NaN come back as they are.  The log of the fp32 sum is taken in fp64 and rounded
// once: near a bin boundary soft_ce amplifies an ulp of it by (l[i0] - l[i1]) / bin_size (4.8e-6 x 1e4 on a one-hot row at the
// clamp), and logf is only good to an ulp.  Measured on the MI355X with logf: target -22025.4 (symlog -9.999997) on the row
// "hot0" (-1e4 but bin 0) is 0.043 off, 3.9 x the gate of tests/test_gpu_model_edges.py, which the reference's fp32 meets
// (DESIGN 3.4d).  One call per row and head, by one lane; ks_value_chain keeps its registers (145 / 174 VGPRs either way).
__device__ __forceinline__ float symlog_f(float x) {
    const float m = (float)log((double)(1.f + fabsf(x)));
    return x > 0.f ? m : (x < 0.f ? -m : x);
}

// soft_ce(logits, target) of one row (math.py:5-9) with the two target bins picked by index (math.py:58-71): no two-hot
// row is materialised.  The upper bin wraps to 0 at vmax, where its weight is 0, exactly as the reference's scatter does.
// +-Inf targets clamp to vmin / vmax like any other; a NaN target gives a NaN term (fminf / fmaxf alone would drop it: every
// torch op of the reference propagates it), read from bin 0 so that nothing indexes outside the row.
__device__ __forceinline__ float model_soft_ce(const float *rp, float lse, float target, const ModelLossArgs &a) {
    const float s = symlog_f(target);
    const float x = s != s ? s : fminf(fmaxf(s, a.vmin), a.vmax);
    const float u = (x - a.vmin) / a.bin_size;
    const float fl = floorf(u);
    const float off = u - fl;
    int i0 = fl == fl ? (int)fl : 0;
    i0 = i0 < 0 ? 0 : (i0 > a.num_bins - 1 ? a.num_bins - 1 : i0);
    const int i1 = (i0 + 1) % a.num_bins;
    return -((1.f - off) * (rp[i0] - lse) + off * (rp[i1] - lse));
}

// binary_cross_entropy_with_logits of one element, the stable form: max(x, 0) - x y + log(1 + exp(-|x|))
__device__ __forceinline__ float model_bce(float x, float y) { return fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x))); }

// ---- shared by the seed units (k_loss_grad.hip, k_pi_grad.hip)
// max and sum of exp(x - max) of one row of logits by one wavefront (the order of model_row_stats); every lane gets both
__device__ __forceinline__ float row_max(const float *rp, int lane, int num_bins) {
    float m = -INFINITY;
    for (int j = lane; j < num_bins; j += 64) m = fmaxf(m, rp[j]);
    return group_max<64>(m);
}
__device__ __forceinline__ void row_max_sum(const float *rp, int lane, int num_bins, float &m, float &es) {
    m = row_max(rp, lane, num_bins);
    es = 0.f;
    for (int j = lane; j < num_bins; j += 64) es += expf(rp[j] - m);
    es = group_sum<64>(es);
}
// seed_ordered_sum of seed_route.h on a workgroup of 256 threads: block_tree takes each thread's partial, block_sum forms it from src
__device__ __forceinline__ float block_tree(float s, float *red) {
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + w];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ float block_sum(const float *src, uint64_t n, float *red) {
    float s = 0.f;
    for (uint64_t i = threadIdx.x; i < n; i += 256) s = s + src[i];
    return block_tree(s, red);
}

// ---------------------------------------------------------------- generic kernels (instantiated by k_model.hip's generic unit)
#ifdef MODEL_GENERIC_KERNELS
// one wavefront per row
__global__ __launch_bounds__(RW_THREADS) void k_model_cons_rows(ModelConsParams p) {
    const int row = blockIdx.x * (RW_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= p.rows) return;
    const float *a = p.zs1 + (size_t)row * p.L, *b = p.next_z + (size_t)row * p.L;
    float s = 0.f;
    for (int c = lane; c < p.L; c += 64) {
        const float d = a[c] - b[c];
        s = fmaf(d, d, s);
    }
    s = group_sum<64>(s);
    if (lane == 0) p.rowloss[(size_t)MK_CONS * p.rows + row] = s;
}

// sum of B floats by 256 threads in a fixed order: thread-strided partials, then an LDS tree
__device__ __forceinline__ float model_block_sum(const float *src, int n, float *red) {
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += src[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// tdmpc2/tdmpc2.py:285-304 from the per-row terms.  One workgroup of 256 threads.
__global__ __launch_bounds__(256) void k_model_tail(ModelTailParams p) {
    __shared__ float red[256];
    const long HB = (long)p.H * p.B;
    float cons = 0.f, rew = 0.f, val = 0.f, term = 0.f;
    // a bounded wait of the layered GEMMs gave up somewhere in this call: EVERY output is NaN (tdmpc2_plan_take_fault)
    const bool bad = p.err && __hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
    const float nan = __builtin_nanf("");
    for (int t = 0; t < p.H; ++t) {
        const float c_t = model_block_sum(p.rowloss + (size_t)MK_CONS * HB + (size_t)t * p.B, p.B, red) / ((float)p.B * (float)p.L);
        const float r_t = model_block_sum(p.rowloss + (size_t)MK_REW * HB + (size_t)t * p.B, p.B, red) / (float)p.B;
        float v_t = 0.f;
        for (int i = 0; i < p.nq; ++i)
            v_t += model_block_sum(p.rowloss + (size_t)(MK_Q0 + i) * HB + (size_t)t * p.B, p.B, red) / (float)p.B;
        const float e_t = p.episodic ? model_block_sum(p.rowloss + (size_t)MK_TERM * HB + (size_t)t * p.B, p.B, red) / (float)p.B : 0.f;
        cons += c_t * p.rho_pow[t];
        rew += r_t * p.rho_pow[t];
        val += v_t * p.rho_pow[t];
        term += e_t;
        if (p.step_means && threadIdx.x == 0) {
            p.step_means[0 * p.H + t] = bad ? nan : c_t;
            p.step_means[1 * p.H + t] = bad ? nan : r_t;
            p.step_means[2 * p.H + t] = bad ? nan : v_t / (float)p.nq;
            p.step_means[3 * p.H + t] = bad ? nan : e_t;
        }
    }
    if (threadIdx.x != 0) return;
    cons /= (float)p.H;
    rew /= (float)p.H;
    val /= (float)(p.H * p.nq);
    term /= (float)p.H;
    float total = p.coef[0] * cons + p.coef[1] * rew + p.coef[3] * term + p.coef[2] * val;
    if (bad) cons = rew = val = term = total = nan;
    p.losses[0] = cons;
    p.losses[1] = rew;
    p.losses[2] = val;
    p.losses[3] = term;
    p.losses[4] = total;
}

// task of row r of the flattened [n, B] rows = task_ids[r % B]; rows in [rows, rows_p) take task 0
__global__ void k_model_tile_tasks(const int *task_ids, int B, int rows, int rows_p, int *out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows_p) out[r] = r < rows ? task_ids[r % B] : 0;
}
#endif  // MODEL_GENERIC_KERNELS
