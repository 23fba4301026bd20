// Translation unit of the planner's kernels that belong to no family of their own, behind their launchers of launch.h:
//   k_refit              elite selection + refit + final pick of one plan per workgroup (refit_plan, common.cuh;
//                        tdmpc2/tdmpc2.py:184-206): the layered family, the fused family when it does not fold the refit,
//                        tdmpc2_plan_refit, shard_refit
//   ks_task_bias         the per-task effective first-layer biases of the fused family's multitask value calls (plan_train.hip)
//   encoder_kernels.cuh  state observations (WorldModel.encode, tdmpc2/common/world_model.py:103-112): k_encode, k_enc_gemv,
//                        k_enc_norm -- the policy prior's spread route normalises its rows with k_enc_norm through the same launcher
//   pixel_kernels.cuh    pixel observations, planning routes (tdmpc2/common/layers.py:36-71, 136-150): k_pix_image,
//                        k_pix_spread<0..3> and the bind-time re-pack k_pix_pack (the batch route is k_pixel_batch.hip)
//   k_export_noise       the in-kernel generator written out as a noise tape (tdmpc2_plan_export_noise, plan_run.hip)
// One unit, in the order these kernels had inside the former host unit: the code object then lays them out as before.  Their host
// sides are plan_run.hip, plan_train.hip, plan_obs.hip and plan_weights.hip.  Apart from launch_refit the launchers do not check:
// the host asks hipGetLastError once after a call's launches, as it always has.
#include "launch.h"

namespace {

// one workgroup per plan (layered family; tdmpc2_plan_refit)
__global__ void k_refit(RefitParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    refit_plan(p, blockIdx.x, smem, threadIdx.x, blockDim.x);
}

// beff_tab[task][net][WIDTH] = b + W[:, L:L+T] . task_emb[task] for the policy and the Q heads (online or target):
// the per-task effective first-layer biases ks_value indexes per row.  grid = n_tasks, block = WIDTH threads.
__global__ void ks_task_bias(TaskBiasParams p) {
    const int task = blockIdx.x, f = threadIdx.x;
    const float *emb = p.task_emb + (size_t)task * p.T;
    for (int net = 0; net < p.nnets; ++net) {
        if (!p.wemb[net]) continue;
        const float *w = p.wemb[net] + (size_t)f * p.T;
        float sacc = 0.f;
        for (int k = 0; k < p.T; ++k) sacc = fmaf(w[k], emb[k], sacc);
        p.beff_tab[((size_t)task * p.nnets + net) * WIDTH + f] = p.bias[net][f] + sacc;
    }
}

#include "encoder_kernels.cuh"
#include "pixel_kernels.cuh"

// ================================================================ the in-kernel generator as a noise tape (tdmpc2_plan_export_noise)
// Every draw of a tape = NULL plan, written with the index formulas and device functions of the kernels that consume them
// (ks_rollout / ks_rollout_cl / ks_pitraj / l_sample / l_pi_head / l_qidx / refit_plan), for environments [e0, e0 + n).
struct NoiseExportParams : NoiseExportArgs {};  // the kernel's own name for the block of launch.h ("kernel parameter types" there)
__global__ void k_export_noise(NoiseExportParams p) {
    const size_t gtid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, gsz = (size_t)gridDim.x * blockDim.x;
    const int NS = p.N - p.P, hpa = (p.A + 1) / 2;
    if (p.o.pi_traj_eps)  // [n,H,P,A]: rng_normal(SITE_PITRAJ, iter = t, row * A + a)
        for (size_t i = gtid; i < (size_t)p.n * p.H * p.P * p.A; i += gsz) {
            const unsigned ra = (unsigned)(i % ((size_t)p.P * p.A));
            const size_t r = i / ((size_t)p.P * p.A);
            const int t = (int)(r % p.H), e = (int)(r / p.H);
            p.o.pi_traj_eps[i] = rng_normal(p.seed, p.call, SITE_PITRAJ, t, p.e0 + e, ra);
        }
    if (p.o.sample_eps)  // [n,I,H,N-P,A]: Philox pairs over (t, n, a / 2) with the fused tile's action padding
        for (size_t i = gtid; i < (size_t)p.n * p.I * p.H * NS * hpa; i += gsz) {
            const int a0 = 2 * (int)(i % hpa);
            size_t r = i / hpa;
            const int ns = (int)(r % NS);
            r /= NS;
            const int t = (int)(r % p.H);
            r /= p.H;
            const int it = (int)(r % p.I), e = (int)(r / p.I);
            float z0, z1;
            rng_normal2(p.seed, p.call, SITE_SAMPLE, it, p.e0 + e, (unsigned)(((size_t)t * NS + ns) * p.hp + a0 / 2), z0, z1);
            float *dst = p.o.sample_eps + ((((size_t)e * p.I + it) * p.H + t) * NS + ns) * p.A + a0;
            dst[0] = z0;
            if (a0 + 1 < p.A) dst[1] = z1;
        }
    if (p.o.pi_eps)  // [n,I,N,A]: rng_normal(SITE_PI, iter, n * A + a)
        for (size_t i = gtid; i < (size_t)p.n * p.I * p.N * p.A; i += gsz) {
            const unsigned ra = (unsigned)(i % ((size_t)p.N * p.A));
            const size_t r = i / ((size_t)p.N * p.A);
            const int it = (int)(r % p.I), e = (int)(r / p.I);
            p.o.pi_eps[i] = rng_normal(p.seed, p.call, SITE_PI, it, p.e0 + e, ra);
        }
    if (p.o.qidx)  // [n,I,2]: two distinct heads, uniform over ordered pairs (the randperm(nq)[:2] of world_model.py:212)
        for (size_t i = gtid; i < (size_t)p.n * p.I; i += gsz) {
            const int it = (int)(i % p.I), e = (int)(i / p.I);
            const uint4 r = rng_raw(p.seed, p.call, SITE_QIDX, it, p.e0 + e, 0);
            int q0 = (int)(r.x % (unsigned)p.nq), q1 = (int)(r.y % (unsigned)(p.nq - 1));
            if (q1 >= q0) ++q1;
            p.o.qidx[2 * i] = q0;
            p.o.qidx[2 * i + 1] = q1;
        }
    if (p.o.gumbel_exp)  // [n,K]
        for (size_t i = gtid; i < (size_t)p.n * p.K; i += gsz)
            p.o.gumbel_exp[i] = rng_exponential(p.seed, p.call, SITE_GUMBEL, 0, p.e0 + (int)(i / p.K), (unsigned)(i % p.K));
    if (p.o.final_eps)  // [n,A]
        for (size_t i = gtid; i < (size_t)p.n * p.A; i += gsz)
            p.o.final_eps[i] = rng_normal(p.seed, p.call, SITE_FINAL, 0, p.e0 + (int)(i / p.A), (unsigned)(i % p.A));
}

}  // namespace

int tdk::launch_refit(const RefitParams &fp, int E, int N, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL(k_refit, dim3(E), dim3(refit_threads(N)), lds, st, fp);
    LAUNCH_CHECK();
    return 0;
}

void tdk::launch_task_bias(const TaskBiasParams &p, int n_tasks, hipStream_t st) {
    hipLaunchKernelGGL(ks_task_bias, dim3(n_tasks), dim3(WIDTH), 0, st, p);
}

void tdk::launch_export_noise(const NoiseExportArgs &p, int grid, int threads, hipStream_t st) {
    hipLaunchKernelGGL(k_export_noise, dim3(grid), dim3(threads), 0, st, NoiseExportParams{p});
}

void tdk::enc_launch_encode(const EncodeArgs &p, int grid, int threads, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL(k_encode, dim3(grid), dim3(threads), lds, st, EncodeParams{p});
}

void tdk::enc_launch_gemv(const EncGemvArgs &p, int gx, int gy, int threads, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL(k_enc_gemv, dim3(gx, gy), dim3(threads), lds, st, EncGemvParams{p});
}

void tdk::enc_launch_norm(const EncNormArgs &p, int grid, int threads, hipStream_t st) {
    hipLaunchKernelGGL(k_enc_norm, dim3(grid), dim3(threads), 0, st, EncNormParams{p});
}

void tdk::pix_launch_image(const PixArgs &p, const PixGrid &g, hipStream_t st) {
    hipLaunchKernelGGL(k_pix_image, dim3(g.x), dim3(g.threads), g.lds, st, PixParams{p});
}

void tdk::pix_launch_spread(int layer, const PixArgs &p, const PixGrid &g, hipStream_t st) {
    const dim3 grid(g.x, g.y, g.z), block(g.threads);
    switch (layer) {
        case 0: hipLaunchKernelGGL(k_pix_spread<0>, grid, block, 0, st, PixParams{p}); break;
        case 1: hipLaunchKernelGGL(k_pix_spread<1>, grid, block, 0, st, PixParams{p}); break;
        case 2: hipLaunchKernelGGL(k_pix_spread<2>, grid, block, 0, st, PixParams{p}); break;
        default: hipLaunchKernelGGL(k_pix_spread<3>, grid, block, 0, st, PixParams{p}); break;
    }
}

void tdk::pix_launch_pack(const float *w, float *wp, int C, int cin, int kk, int grid, int threads, hipStream_t st) {
    hipLaunchKernelGGL(k_pix_pack, dim3(grid), dim3(threads), 0, st, w, wp, C, cin, kk);
}
