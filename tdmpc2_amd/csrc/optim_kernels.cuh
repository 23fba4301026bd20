// Kernels of the optimiser step (included by k_optim.hip inside its namespace): the norm's chunk pass, its total pass with the
// step's device scalars, and the update pass.  Three launches per step whatever the number of segments.  Every decision (chunks,
// quads, the segment of a quad, the order of the norm) is optim_route.h's.
//
// The element math is a chain of separately rounded fp32 operations (include/tdmpc2_plan.h): this file is compiled with
// contraction off -- hipcc at -O3 fuses __fadd_rn(__fmul_rn(a, b), c) into v_fma_f32 otherwise -- and fp32 `/` and sqrt keep
// hipcc's correctly rounded expansions (v_div_scale / v_div_fmas / v_div_fixup): no flag of the unit relaxes them.
#pragma clang fp contract(off)

struct OptHyper {
    float beta1, beta2, eps, max_norm;
    float a1, a2;  // fp32(1 - beta1), fp32(1 - beta2), each rounded once from the fp64 difference
};

struct OptNormParams {
    const float *grad;
    float *partial;
    uint64_t arena_quads;
};

struct OptTotalParams {
    const float *partial;
    uint64_t chunks;
    OptState *state;
    float *ss;        // [groups]
    const float *lr;  // [groups]
    int32_t n_groups;
    OptHyper h;
    float *norm_out;  // may be null
};

struct OptUpdateParams {
    float *grad, *exp_avg, *exp_avg_sq;
    const OptSeg *segs;
    const int32_t *chunk_seg;
    const OptState *state;
    const float *ss;
    uint64_t arena_quads;
    OptHyper h;
    int32_t zero_grad;
};

// wave and workgroup steps of the norm's order; the value is valid in thread 0 (every lane of a wave holds its wave's sum)
__device__ inline float opt_block_sum(float acc, float *wave_sums) {
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) acc = acc + __shfl_xor(acc, w, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = acc;
    __syncthreads();
    float total = wave_sums[0];
#pragma unroll
    for (int w = 1; w < OPT_WAVES; ++w) total = total + wave_sums[w];
    return total;
}

__global__ __launch_bounds__(OPT_THREADS) void k_opt_norm(const OptNormParams p) {
    __shared__ float wave_sums[OPT_WAVES];
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < OPT_QUADS_PER_THREAD; ++j) {
        const uint64_t q = opt_quad(blockIdx.x, (int)threadIdx.x, j);
        if (q < p.arena_quads) {
            const float4 g = *reinterpret_cast<const float4 *>(p.grad + q * OPT_QUAD);
            acc = acc + g.x * g.x;
            acc = acc + g.y * g.y;
            acc = acc + g.z * g.z;
            acc = acc + g.w * g.w;
        }
    }
    const float total = opt_block_sum(acc, wave_sums);
    if (threadIdx.x == 0) p.partial[blockIdx.x] = total;
}

// one workgroup: the total of the partials, then the scalars of this step
__global__ __launch_bounds__(OPT_THREADS) void k_opt_total(const OptTotalParams p) {
    __shared__ float wave_sums[OPT_WAVES];
    __shared__ double s_b1p;
    float acc = 0.0f;
    for (uint64_t k = threadIdx.x; k < p.chunks; k += OPT_THREADS) acc = acc + p.partial[k];
    const float total = opt_block_sum(acc, wave_sums);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(total);
        const float r = p.h.max_norm / (norm + 1e-6f);
        const float clip = r > 1.0f ? 1.0f : r;  // min(1, r) that keeps a NaN, as torch's clamp does
        OptState s = *p.state;
        s.step += 1;
        s.b1p *= (double)p.h.beta1;
        s.b2p *= (double)p.h.beta2;
        s.norm = norm;
        s.clip = clip;
        s.bc = (float)sqrt(1.0 - s.b2p);
        *p.state = s;
        s_b1p = s.b1p;
        if (p.norm_out) *p.norm_out = norm;
    }
    __syncthreads();
    const double bc1 = 1.0 - s_b1p;
    for (int32_t g = (int32_t)threadIdx.x; g < p.n_groups; g += OPT_THREADS) p.ss[g] = (float)((double)p.lr[g] / bc1);
}

__device__ inline void opt_element(float &g, float &m, float &v, float &w, float clip, float ss, float bc, const OptHyper &h) {
    g = g * clip;
    m = m + (g - m) * h.a1;
    v = v * h.beta2 + (g * h.a2) * g;
    const float d = sqrtf(v) / bc + h.eps;
    w = w - ss * (m / d);
}

__global__ __launch_bounds__(OPT_THREADS) void k_opt_update(const OptUpdateParams p) {
    const float clip = p.state->clip, bc = p.state->bc;
    const int32_t seg_lo = p.chunk_seg[blockIdx.x], seg_hi = p.chunk_seg[blockIdx.x + 1];
#pragma unroll
    for (int j = 0; j < OPT_QUADS_PER_THREAD; ++j) {
        const uint64_t q = opt_quad(blockIdx.x, (int)threadIdx.x, j);
        if (q >= p.arena_quads) continue;
        const int32_t si = opt_seg_of_quad(&p.segs[0].quad0, sizeof(OptSeg), seg_lo, seg_hi, q);
        const OptSeg seg = p.segs[si];
        const float ss = p.ss[seg.group];
        const uint64_t e0 = (q - seg.quad0) * OPT_QUAD;  // first element of the quad inside its segment
        float *w = seg.param + e0;
        float4 g4 = *reinterpret_cast<const float4 *>(p.grad + q * OPT_QUAD);
        float4 m4 = *reinterpret_cast<const float4 *>(p.exp_avg + q * OPT_QUAD);
        float4 v4 = *reinterpret_cast<const float4 *>(p.exp_avg_sq + q * OPT_QUAD);
        float g[4] = {g4.x, g4.y, g4.z, g4.w}, m[4] = {m4.x, m4.y, m4.z, m4.w}, v[4] = {v4.x, v4.y, v4.z, v4.w}, x[4];
        if (e0 + OPT_QUAD <= seg.count) {  // a whole quad of the parameter: one 16-byte access where the tensor allows it
            const bool vec = ((uintptr_t)w & 15) == 0;
            if (vec) {
                const float4 x4 = *reinterpret_cast<const float4 *>(w);
                x[0] = x4.x; x[1] = x4.y; x[2] = x4.z; x[3] = x4.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) x[i] = w[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) opt_element(g[i], m[i], v[i], x[i], clip, ss, bc, p.h);
            if (vec) {
                *reinterpret_cast<float4 *>(w) = make_float4(x[0], x[1], x[2], x[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) w[i] = x[i];
            }
        } else {  // the segment's tail: 1 .. 3 elements, then padding that stays zero whatever clip is
            const int rem = (int)(seg.count - e0);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                if (i < rem) {
                    x[i] = w[i];
                    opt_element(g[i], m[i], v[i], x[i], clip, ss, bc, p.h);
                    w[i] = x[i];
                } else {
                    g[i] = 0.0f; m[i] = 0.0f; v[i] = 0.0f;
                }
            }
            g[3] = 0.0f; m[3] = 0.0f; v[3] = 0.0f;
        }
        if (p.zero_grad) g4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        else g4 = make_float4(g[0], g[1], g[2], g[3]);
        *reinterpret_cast<float4 *>(p.grad + q * OPT_QUAD) = g4;
        *reinterpret_cast<float4 *>(p.exp_avg + q * OPT_QUAD) = make_float4(m[0], m[1], m[2], m[3]);
        *reinterpret_cast<float4 *>(p.exp_avg_sq + q * OPT_QUAD) = make_float4(v[0], v[1], v[2], v[3]);
    }
}
