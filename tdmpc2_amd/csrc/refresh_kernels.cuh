// The weight packer: caller's fp32 tensors -> the handle's packed storage, in at most four launches over a job table (RfParams,
// refresh_params.h; the launch list is refresh_route.h).  Every entry point that stores weights runs these kernels and no
// others: tdmpc2_plan_refresh_weights / tdmpc2_plan_soft_update_target with a table of jobs, tdmpc2_plan_bind_weights /
// bind_encoder / bind_policy with one job (one layer, every ensemble member).  This file is therefore the definition of the
// scale rule, the source-column map, the fragment layouts and the transposed copies; tests/golden/packed_digests.json pins
// the bytes.  Included by k_refresh.hip inside its anonymous namespace.  No inline assembly, no waits between workgroups; the
// only atomic is the integer atomicMax on the bits of a non-negative float (order preserving on the uint pattern, order
// independent).
#pragma once

typedef _Float16 rf_half8 __attribute__((ext_vector_type(8)));

// job of a workgroup: the last one whose first workgroup is <= blk (absent jobs are empty ranges)
__device__ __forceinline__ int rf_find(const int *blk0, int njobs, int blk) {
    int job = 0;
    while (job + 1 < njobs && blk >= blk0[job + 1]) ++job;
    return job;
}

// ---------------------------------------------------------------- RO_RESET
__global__ __launch_bounds__(RF_THREADS) void k_rf_reset(RfParams p) {
    for (int item = threadIdx.x; item < RF_NETS * MAXQ * 3; item += RF_THREADS) {
        const int net = item / (MAXQ * 3), hd = (item / 3) % MAXQ, l = item % 3;
        const RfNet &N = p.net[net];
        if (!(N.mask >> l & 1) || !N.scal || hd >= N.heads) continue;
        LayerScal *s = N.scal + hd * 3 + l;
        s->maxbits = 0u;
        if (N.l[l].has_ln) {
            s->gmax = 0u;
            s->bmax = 0u;
        }
    }
}

// ---------------------------------------------------------------- RO_SCAN (+ the lerp of a soft update)
// torch.lerp (WorldModel.soft_update_target_Q, world_model.py:82-86): t + w (o - t) for |w| < 0.5, else o - (o - t) (1 - w)
__device__ __forceinline__ float rf_lerp(float t, float o, float w) {
    const float d = o - t;
    return w < 0.5f ? t + w * d : o - d * (1.f - w);
}
// max over the FINITE |v|: NaN and Inf entries do not take part in a scale
__device__ __forceinline__ float rf_absmax(float m, float v) {
    const float a = fabsf(v);
    return (a == a && a < INFINITY) ? fmaxf(m, a) : m;
}
// max over one vector (all threads of the workgroup), lerped in place first when `on` is given; out: the word to raise, or null
__device__ __forceinline__ void rf_scan_vec(const float *src, const float *on, float w, size_t n, size_t i0, size_t stride,
                                            unsigned int *out) {
    float m = 0.f;
    for (size_t i = i0; i < n; i += stride) {
        float v = src[i];
        if (on) {
            v = rf_lerp(v, on[i], w);
            const_cast<float *>(src)[i] = v;  // written once; the maximum is over what was written
        }
        m = rf_absmax(m, v);
    }
    if (out) {
        m = group_max<64>(m);
        if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));
    }
}
__global__ __launch_bounds__(RF_THREADS) void k_rf_scan(RfParams p) {
    const int blk = blockIdx.x;
    const int job = rf_find(p.scan_blk0, 3 * RF_NETS, blk);
    const int net = job / 3, l = job % 3;
    const RfNet &N = p.net[net];
    const RfLayer &L = N.l[l];
    const int per_head = L.scan_nbw + 1;
    const int local = blk - p.scan_blk0[job];
    const int hd = local / per_head, r = local % per_head;
    if (hd >= N.heads) return;
    const bool lerp = p.lerp_net == net;
    LayerScal *s = N.scal ? N.scal + hd * 3 + l : nullptr;
    if (r < L.scan_nbw) {
        const size_t n = (size_t)L.out * L.in;
        rf_scan_vec(L.W + hd * n, lerp ? p.online[l][0] + hd * n : nullptr, p.tau, n, (size_t)r * RF_THREADS + threadIdx.x,
                    (size_t)L.scan_nbw * RF_THREADS, s ? &s->maxbits : nullptr);
        return;
    }
    // the vectors of this member: the bias only moves (soft update), the LayerNorm vectors are scanned as well
    const size_t o = (size_t)hd * L.out;
    if (lerp) rf_scan_vec(L.b + o, p.online[l][1] + o, p.tau, (size_t)L.out, threadIdx.x, RF_THREADS, nullptr);
    if (L.has_ln) {
        rf_scan_vec(L.g + o, lerp ? p.online[l][2] + o : nullptr, p.tau, (size_t)L.out, threadIdx.x, RF_THREADS, s ? &s->gmax : nullptr);
        rf_scan_vec(L.beta + o, lerp ? p.online[l][3] + o : nullptr, p.tau, (size_t)L.out, threadIdx.x, RF_THREADS, s ? &s->bmax : nullptr);
    }
}

// ---------------------------------------------------------------- RO_SCALES
// One thread per (net, head).  Named layers get their exponents from the maxima of RO_SCAN:
//   kw such that max|W| 2^kw in [2^13, 2^14); wscale = 2^kw multiplies the matrix before its hi / lo split.
//   ka, the output scale of a LayerNorm + Mish layer of `width` features: |LayerNorm(x)_i| <= sqrt(width - 1) for any x, so
//   |Mish(g x + b)| <= sqrt(width - 1) max|g| + max|b| =: B.  ka = the largest exponent <= 5 with B 2^ka < 2^15 (half of the
//   f16 maximum: rounding of the hi piece cannot reach Inf).  Trained checkpoints (g ~ 1) keep ka = 5.
// Then oscale of ALL three layers from the stored kw / ka, so that a job naming one layer leaves its neighbours' exponents
// alone and still corrects the next layer's oscale: layer 0 reads [z | a] (scale 2^5), layer l > 0 reads layer l - 1's output.
__global__ __launch_bounds__(RF_THREADS) void k_rf_scales(RfParams p) {
    for (int item = threadIdx.x; item < RF_NETS * MAXQ; item += RF_THREADS) {
        const int net = item / MAXQ, hd = item % MAXQ;
        const RfNet &N = p.net[net];
        if (!N.mask || !N.scal || hd >= N.heads) continue;
        LayerScal *s3 = N.scal + hd * 3;
        for (int l = 0; l < 3; ++l) {
            if (!(N.mask >> l & 1)) continue;
            LayerScal *s = s3 + l;
            const float m = __uint_as_float(s->maxbits);
            int ex = 0;
            if (m > 0.f) frexpf(m, &ex);  // m = f 2^ex, f in [0.5, 1)
            int kw = 14 - ex;
            kw = kw > 40 ? 40 : (kw < -40 ? -40 : kw);
            s->kw = kw;
            s->wscale = ldexpf(1.f, kw);
            int ka = ACT_SCALE_LOG2;
            if (N.l[l].has_ln && N.l[l].mish) {
                const int width = N.l[l].out;
                const float bound = sqrtf((float)(width > 1 ? width - 1 : 1)) * __uint_as_float(s->gmax) + __uint_as_float(s->bmax);
                if (bound > 0.f) {
                    int eb = 0;
                    frexpf(bound, &eb);  // bound < 2^eb
                    ka = 15 - eb < ka ? 15 - eb : ka;
                }
                ka = ka < -24 ? -24 : ka;
            }
            s->ka = ka;
            s->ascale = ldexpf(1.f, ka);
        }
        for (int l = 0; l < 3; ++l) {
            const int kin = l == 0 ? ACT_SCALE_LOG2 : s3[l - 1].ka;
            s3[l].oscale = ldexpf(1.f, -(s3[l].kw + kin));
        }
    }
}

// ---------------------------------------------------------------- RO_PACK
constexpr int RF_LDT = RF_TILE_K + 1;  // LDS row stride of the 32 x RF_TILE_K tile (odd: the fragment reads walk rows conflict-free)

// 32 rows x RF_TILE_K packed columns of one matrix: source rows read coalesced into LDS (scaled for the split arithmetic), then
// written in MFMA fragment order, 16 bytes per (k block, lane) and plane:
//   split  dst[ct][kb][plane][lane][e] = W[row = ct*32 + (lane & 31)][k = kb*16 + 8 (lane >> 5) + e] * wscale, hi / lo f16 planes
//   fp32   dst[ct][kb][lane][r]        = W[row = ct*32 + (lane & 31)][k = kb*8 + 4 (lane >> 5) + r]
// The packed k axis is [z columns (nz) | action columns (na, zero padded)], the source columns are [z (nz) | task_emb (nt) |
// action (na)] (tdmpc2/common/world_model.py:118-120); rows beyond `out` are zero.
__device__ __forceinline__ void rf_pack_tile(const RfLayer &L, const float *W, char *dst, int ct, int kc, int split, float sc, float *tile) {
    const int tid = threadIdx.x;
    const int kp = L.KB * (split ? 16 : 8);
    for (int i = tid; i < 32 * RF_TILE_K; i += RF_THREADS) {
        const int rl = i / RF_TILE_K, kl = i % RF_TILE_K;
        const int row = ct * 32 + rl, k = kc * RF_TILE_K + kl;
        float v = 0.f;
        if (row < L.out && k < kp) {
            int src = -1;
            if (k < L.nz) src = k;
            else if (k - L.nz < L.na) src = L.nz + L.nt + (k - L.nz);
            if (src >= 0 && src < L.in) {
                v = W[(size_t)row * L.in + src];
                if (split) v = v * sc;
            }
        }
        tile[rl * RF_LDT + kl] = v;
    }
    __syncthreads();
    if (split) {
        _Float16 *d = reinterpret_cast<_Float16 *>(dst);
        for (int j = tid; j < (RF_TILE_K / 16) * 64; j += RF_THREADS) {
            const int kbl = j >> 6, lane = j & 63;
            const int kb = kc * (RF_TILE_K / 16) + kbl;
            if (kb >= L.KB) continue;
            const float *t = tile + (lane & 31) * RF_LDT + kbl * 16 + 8 * (lane >> 5);
            rf_half8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = t[e];
                const _Float16 h = (_Float16)v;
                hi[e] = h;
                lo[e] = (_Float16)(v - (float)h);
            }
            _Float16 *base = d + ((size_t)ct * L.KB + kb) * 1024;  // 2 planes x 64 lanes x 8
            *reinterpret_cast<rf_half8 *>(base + lane * 8) = hi;
            *reinterpret_cast<rf_half8 *>(base + 512 + lane * 8) = lo;
        }
    } else {
        float *d = reinterpret_cast<float *>(dst);
        for (int j = tid; j < (RF_TILE_K / 8) * 64; j += RF_THREADS) {
            const int kbl = j >> 6, lane = j & 63;
            const int kb = kc * (RF_TILE_K / 8) + kbl;
            if (kb >= L.KB) continue;
            const float *t = tile + (lane & 31) * RF_LDT + kbl * 8 + 4 * (lane >> 5);
            *reinterpret_cast<float4 *>(d + (((size_t)ct * L.KB + kb) * 64 + lane) * 4) = make_float4(t[0], t[1], t[2], t[3]);
        }
    }
}

// nn.Linear [out][in] -> [in][out], one 32 x 32 tile, + the vectors by the first workgroup
__device__ __forceinline__ void rf_transpose_tile(const RfTrans &T, int local, float *tile) {
    const int tid = threadIdx.x;
    const int tiles_k = (T.in + 31) / 32;
    const int f0 = (local / tiles_k) * 32, k0 = (local % tiles_k) * 32;
    for (int i = tid; i < 1024; i += RF_THREADS) {
        const int fl = i >> 5, kl = i & 31;
        if (f0 + fl < T.out && k0 + kl < T.in) tile[fl * 33 + kl] = T.W[(size_t)(f0 + fl) * T.in + k0 + kl];
    }
    __syncthreads();
    for (int i = tid; i < 1024; i += RF_THREADS) {
        const int kl = i >> 5, fl = i & 31;
        if (f0 + fl < T.out && k0 + kl < T.in) T.wt[(size_t)(k0 + kl) * T.out + f0 + fl] = tile[fl * 33 + kl];
    }
    if (local == 0)
        for (int i = tid; i < T.out; i += RF_THREADS) {
            T.bias[i] = T.b[i];
            if (T.g) T.gd[i] = T.g[i];
            if (T.beta) T.bd[i] = T.beta[i];
        }
}

__global__ __launch_bounds__(RF_THREADS) void k_rf_pack(RfParams p) {
    __shared__ float tile[32 * RF_LDT];
    const int blk = blockIdx.x, tid = threadIdx.x;
    const int seg = rf_find(p.pack_blk0, RF_SEGS, blk);
    const int local = blk - p.pack_blk0[seg];
    if (seg >= 3 * RF_NETS) {
        rf_transpose_tile(p.tr[seg - 3 * RF_NETS], local, tile);
        return;
    }
    const int net = seg / 3, l = seg % 3;
    const RfNet &N = p.net[net];
    const RfLayer &L = N.l[l];
    const int kp = L.KB * (p.split ? 16 : 8);
    const int nkc = rf_pack_kchunks(kp);
    const int n_w = L.CT * nkc;
    const int per_head = n_w + 1 + (L.nt > 0 ? L.CT : 0);
    const int hd = local / per_head, r = local % per_head;
    if (hd >= N.heads) return;
    const float *W = L.W + (size_t)hd * L.out * L.in;
    if (r < n_w) {
        const size_t wsz = (size_t)L.CT * L.KB * (p.split ? 512 : 256);  // floats' worth per member (layer_shape)
        const float sc = p.split ? N.scal[hd * 3 + l].wscale : 1.f;
        rf_pack_tile(L, W, reinterpret_cast<char *>(L.wdst + hd * wsz), r / nkc, r % nkc, p.split, sc, tile);
    } else if (r == n_w) {
        const int npad = L.CT * 32;
        const float *b = L.b + (size_t)hd * L.out;
        for (int i = tid; i < npad; i += RF_THREADS) L.bias[(size_t)hd * npad + i] = i < L.out ? b[i] : 0.f;
        if (L.has_ln) {
            const size_t gsz = ((size_t)L.out + 3) / 4 * 4;
            for (int i = tid; i < L.out; i += RF_THREADS) {
                L.gd[hd * gsz + i] = L.g[(size_t)hd * L.out + i];
                L.bd[hd * gsz + i] = L.beta[(size_t)hd * L.out + i];
            }
        }
    } else {  // task-embedding columns of 32 rows: wemb[row][c] = W[row][nz + c]
        const int ct = r - n_w - 1;
        float *e = L.wemb + (size_t)hd * L.out * L.nt;
        for (int i = tid; i < 32 * L.nt; i += RF_THREADS) {
            const int row = ct * 32 + i / L.nt, c = i % L.nt;
            if (row < L.out) e[(size_t)row * L.nt + c] = W[(size_t)row * L.in + L.nz + c];
        }
    }
}
