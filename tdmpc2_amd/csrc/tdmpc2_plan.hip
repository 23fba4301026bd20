// MI355X (gfx950 / CDNA4) native TD-MPC2 MPPI/CEM planner.
//
// What this file implements (reference: nicklashansen/tdmpc2, paths relative to its root):
//   TDMPC2._plan after encode()            tdmpc2/tdmpc2.py:154-206
//   TDMPC2._estimate_value                 tdmpc2/tdmpc2.py:122-136
//   WorldModel.next / reward / pi / Q      tdmpc2/common/world_model.py:114-216
//   NormedLinear / SimNorm                 tdmpc2/common/layers.py:74-118
//   two_hot_inv / symexp / log_std / gumbel_softmax_sample   tdmpc2/common/math.py
//
// This file: the C ABI, the handle, the weight packer's job tables, the elite-refit kernel shared by every path, and the host side of
// the fused family.  Kernels:
//   fused_kernels.cuh    fused 512-wide family (ks_setup / ks_pitraj / ks_rollout): one persistent workgroup keeps 32 or
//                        64 sample rows of one plan in LDS for a whole CEM iteration; templated on the arithmetic
//                        (f16x2 split on the f16 matrix pipe -- the default -- or exact fp32 MFMA), the action padding
//                        and the workgroup geometry
//                        + ks_value: pi + two Q heads on a batch of latent rows (TDMPC2._td_target, tdmpc2.py:239-254,
//                        and the forward half of update_pi, tdmpc2.py:208-225)
//   layered_kernels.cuh, layered_split.cuh, layered_host.cuh
//                        layer-at-a-time family for every other model size and for episodic planning
//   encoder_kernels.cuh  WorldModel.encode for state observations (world_model.py:103-112)
// The policy prior's kernels (WorldModel.pi, act() with mpc = False) are in k_policy.hip; its host side is here.
// Weights are re-packed (bind / refresh: refresh_kernels.cuh) into MFMA fragment order so that a wave's global_load_dwordx4
// reads 1 KiB contiguous; one small workgroup per plan does nan_to_num + top-k + score + mean/std refit (+ the final Gumbel pick)
// between rollout launches (k_refit below).  DESIGN.md has the full account.
#include <cstdarg>
#include <cstring>
#include <new>

#include "handle.h"
#include "launch.h"

namespace {

// one workgroup per plan (layered family; tdmpc2_plan_refit)
__global__ void k_refit(RefitParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    refit_plan(p, blockIdx.x, smem, threadIdx.x, blockDim.x);
}

}  // namespace
int tdk::launch_refit(const RefitParams &fp, int E, int N, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL(k_refit, dim3(E), dim3(refit_threads(N)), lds, st, fp);
    LAUNCH_CHECK();
    return 0;
}
namespace {

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
struct NoiseExportParams {
    int e0, n, H, N, P, A, K, I, nq, hp;
    unsigned long long seed;
    unsigned int call;
    tdmpc2_noise_out o;
};
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

// ================================================================ host side
thread_local std::string g_err;
}  // namespace
int tdk::fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
namespace {

// Every entry point that allocates or launches runs on the handle's device and restores the caller's current device
// (a C caller with several GPUs may have another one current).
struct DevGuard {
    int prev = -1;
    bool ok = true;
    explicit DevGuard(int dev) {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) cur = -1;
        if (cur != dev) {
            ok = hipSetDevice(dev) == hipSuccess;
            if (ok) prev = cur;
        }
    }
    ~DevGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DevGuard(const DevGuard &) = delete;
    DevGuard &operator=(const DevGuard &) = delete;
};


}  // namespace


// The layered path's second stream and its three events come from a process-wide pool and go back to it when a handle is
// destroyed (creating a stream costs a hardware-queue set-up; handles come and go in a training script's evaluation loop).
// (Round 3 believed the pool also cured garbage plans seen after hipStreamDestroy -- profiles/README.md r03k.  It did not: the
// cause was a test moving ONE handle between two streams without ordering them, see StreamTurn below; tools/gpu_r4n.sh
// reproduced the failure with and without the destroys.)
struct SideRes {
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
};
struct SidePool {
    std::mutex mu;
    std::vector<SideRes> free_list[64];
};
static SidePool g_side_pool;
static bool side_acquire(int dev, SideRes *out) {
    const int d = dev >= 0 && dev < 64 ? dev : 0;
    {
        std::lock_guard<std::mutex> lk(g_side_pool.mu);
        if (!g_side_pool.free_list[d].empty()) {
            *out = g_side_pool.free_list[d].back();
            g_side_pool.free_list[d].pop_back();
            return true;
        }
    }
    SideRes r;
    if (hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking) != hipSuccess) return false;  // (a priority above / below the caller's stream loses 2-13 %: profiles/README.md r4u)
    for (int i = 0; i < 3; ++i)
        if (hipEventCreateWithFlags(&r.ev[i], hipEventDisableTiming) != hipSuccess) return false;  // (a failed create leaks what it made)
    *out = r;
    return true;
}
static void side_release(int dev, const SideRes &r) {
    if (!r.stream) return;
    (void)hipStreamSynchronize(r.stream);
    std::lock_guard<std::mutex> lk(g_side_pool.mu);
    g_side_pool.free_list[dev >= 0 && dev < 64 ? dev : 0].push_back(r);
}


namespace {

// A handle owns one workspace and one call counter: two threads inside the same handle would corrupt both.  The second
// caller gets TDMPC2_ERR_STATE instead (use one handle per thread / stream; handles share nothing).
struct Busy {
    tdmpc2_plan *h;
    bool ok;
    explicit Busy(tdmpc2_plan *hh) : h(hh), ok(false) {
        int expected = 0;
        ok = h->busy.compare_exchange_strong(expected, 1, std::memory_order_acquire);
    }
    ~Busy() {
        if (ok) h->busy.store(0, std::memory_order_release);
    }
    Busy(const Busy &) = delete;
    Busy &operator=(const Busy &) = delete;
};
#define ENTER(h)                                                                                                   \
    Busy busy_(h);                                                                                                 \
    if (!busy_.ok) return fail(TDMPC2_ERR_STATE, "the handle is in use by another call (handles are not reentrant)"); \
    DevGuard dev_((h)->cfg.device);                                                                                \
    if (!dev_.ok) return fail(TDMPC2_ERR_HIP, "hipSetDevice(%d) failed", (h)->cfg.device)

// One workspace also means one stream at a time.  A caller that moves a handle to another stream owes the ordering between the
// two (as with any stream-bound workspace); the handle nevertheless orders its own calls: every call on a stream leaves an event
// behind, and the first call on a DIFFERENT stream waits for it.  (Found the hard way, profiles/README.md "r03k, root cause": a
// test planned on the NULL stream and warmed up a graph capture on a non-blocking stream right behind it -- the second plan's
// set-up kernels overwrote the first plan's workspace whenever a second hardware queue already existed.)  Not while the
// stream is capturing: a captured call replays wherever its graph is launched, which the handle cannot see.
struct StreamTurn {
    tdmpc2_plan *h;
    hipStream_t st;
    bool live;
    hipError_t err;
    StreamTurn(tdmpc2_plan *hh, hipStream_t s) : h(hh), st(s), live(false), err(hipSuccess) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
#ifdef TDMPC2_TEST_HOOKS
        static const bool off = getenv("TDMPC2_DEBUG_NO_TURN") != nullptr;  // negative control of the test that pins this (hooks build only)
#else
        constexpr bool off = false;
#endif
        if (!h->turn_ev || off) return;
        if (hipStreamIsCapturing(st, &cap) != hipSuccess) {
            (void)hipGetLastError();
            return;
        }
        if (cap != hipStreamCaptureStatusNone) return;
        live = true;
        if (h->turn_valid && h->turn_stream != st) err = hipStreamWaitEvent(st, h->turn_ev, 0);
    }
    ~StreamTurn() {
        if (!live) return;
        if (hipEventRecord(h->turn_ev, st) == hipSuccess) {
            h->turn_stream = st;
            h->turn_valid = true;
        }
    }
    StreamTurn(const StreamTurn &) = delete;
    StreamTurn &operator=(const StreamTurn &) = delete;
};
#define ENTER_ON(h, stream)                                \
    ENTER(h);                                              \
    StreamTurn turn_((h), (hipStream_t)(stream));          \
    if (turn_.err != hipSuccess) return fail(TDMPC2_ERR_HIP, "hipStreamWaitEvent (stream hand-over of the handle) failed: %s", hipGetErrorString(turn_.err))

int dev_alloc(tdmpc2_plan *h, void **p, size_t bytes) {
    HIP_TRY(hipMalloc(p, bytes ? bytes : 16));
    h->allocs.push_back(*p);
    h->bytes += bytes;
    // TDMPC2_POISON=1 (tests): every allocation starts as NaN bit patterns instead of whatever the allocator hands out
    // (fresh pages read as zero and hide a read of memory that was never written; recycled memory does not)
#ifdef TDMPC2_TEST_HOOKS
    static const bool poison = getenv("TDMPC2_POISON") != nullptr;
    if (poison) HIP_TRY(hipMemset(*p, 0xFF, bytes ? bytes : 16));
#endif
    return 0;
}

void dev_release(tdmpc2_plan *h, void *p) {  // free one allocation made with dev_alloc (tables that are re-grown)
    if (!p) return;
    for (size_t i = 0; i < h->allocs.size(); ++i)
        if (h->allocs[i] == p) {
            h->allocs.erase(h->allocs.begin() + (long)i);
            break;
        }
    (void)hipFree(p);
}

// g_gemm_w's K-split workspaces, one per chain, of ksws_slots(..., mode) slots (plan_layout.h).  Called at create and when
// tdmpc2_plan_set_tuning raises the mode (grows, never shrinks; the smaller buffers stay with the handle until destroy).  `mode`: the
// K-split mode the workspaces are for -- the caller stores it only once they are there; a failed second allocation releases the first.
int ksws_ensure(tdmpc2_plan *h, int mode) {
    Layered &L = h->lay;
    const size_t want = ksws_slots(L.ks_tiles, h->num_cus, mode);
    if (want <= L.ksws_slots) return 0;
    float *a = nullptr, *b = nullptr;
    int rc;
    if ((rc = dev_alloc(h, (void **)&a, want * KS_SLOT_FLOATS * 4))) return rc;
    if (L.side && (rc = dev_alloc(h, (void **)&b, want * KS_SLOT_FLOATS * 4))) {
        dev_release(h, a);
        h->bytes -= want * KS_SLOT_FLOATS * 4;
        return rc;
    }
    L.ksws = a; L.ksws2 = b; L.ksws_slots = want;
    return 0;
}

NetS to_dev(const HostNet &n) {  // split: hi/lo f16 packing + per-matrix scale; exact fp32: fp32 packing, scale 1
    NetS w;
    for (int i = 0; i < 3; ++i)
        w.l[i] = LayerS{n.l[i].wps ? n.l[i].wps : reinterpret_cast<const _Float16 *>(n.l[i].wp), n.l[i].bias, n.l[i].g, n.l[i].b,
                        n.l[i].oscale, n.l[i].ascale, n.l[i].KB, n.l[i].CT};
    return w;
}

HostNet *net_of(tdmpc2_plan *h, int net, int head) {
    switch (net) {
        case TDMPC2_NET_DYNAMICS: return &h->dyn;
        case TDMPC2_NET_REWARD: return &h->rew;
        case TDMPC2_NET_PI: return &h->pi;
        case TDMPC2_NET_Q: return &h->q[head];
        case TDMPC2_NET_TERMINATION: return &h->term;
        case TDMPC2_NET_TARGET_Q: return &h->tq[head];
    }
    return nullptr;
}

int check_ready(tdmpc2_plan *h) {
    for (int i = 0; i < 3; ++i) {
        if (!h->dyn.l[i].bound || !h->rew.l[i].bound || !h->pi.l[i].bound)
            return fail(TDMPC2_ERR_STATE, "weights of layer %d of dynamics/reward/pi are not bound", i);
        for (int qh = 0; qh < h->cfg.num_q; ++qh)
            if (!h->q[qh].l[i].bound) return fail(TDMPC2_ERR_STATE, "weights of Q head %d layer %d are not bound", qh, i);
        if (h->cfg.episodic && !h->term.l[i].bound)
            return fail(TDMPC2_ERR_STATE, "weights of layer %d of the termination head are not bound", i);
    }
    return 0;
}


// The fused kernels are instantiated per action padding (compile-time LDS strides) and arithmetic (AR 0 = f16x2 split,
// 1 = exact fp32 MFMA); ks_rollout / ks_pitraj also per workgroup geometry -- one translation unit per padding (k_fused.hip,
// k_cluster.hip, k_model.hip, k_policy_loss.hip), reached through the tables of launch.h.  Experiment builds (tools/ablate.sh,
// TDMPC2_ONLY_APAD) hold one action padding only, a quarter of the compile time.
#define TDK_CAT_(a, b) a##b
#define TDK_CAT(a, b) TDK_CAT_(a, b)
#ifdef TDMPC2_ONLY_APAD
#define TDK_OPS_BY_APAD(OPS, name) \
    const OPS &name(int) { return TDK_CAT(name##_ap, TDMPC2_ONLY_APAD)(); }
#else
#define TDK_OPS_BY_APAD(OPS, name)         \
    const OPS &name(int apad) {            \
        switch (apad) {                    \
            case 16: return name##_ap16(); \
            case 32: return name##_ap32(); \
            case 48: return name##_ap48(); \
            default: return name##_ap64(); \
        }                                  \
    }
#endif
TDK_OPS_BY_APAD(ModelOps, model_ops)
TDK_OPS_BY_APAD(PolicyLossOps, policy_loss_ops)
TDK_OPS_BY_APAD(FusedOps, fused_ops)
TDK_OPS_BY_APAD(ClusterOps, cluster_ops)

// What fused_route.h decides from: the handle's scalars and the call's plan count.
FusedIn fused_in(const tdmpc2_plan *h, int E) {
    const tdmpc2_plan_cfg &c = h->cfg;
    FusedIn in{};
    in.E = E; in.tiles = h->tiles; in.N = c.num_samples; in.K = c.num_elites; in.H = c.horizon; in.A = c.action_dim;
    in.P = c.num_pi_trajs; in.num_cus = h->num_cus; in.cluster_mode = h->cluster_mode; in.cl_max_clusters = h->cl_max_clusters;
    in.cl2 = h->cl2_xbuf && h->cl2_mode; in.episodic = c.episodic != 0; in.cl_fault = h->cl_fault != 0;
    in.force_rows = h->force_rows; in.fold_refit = h->fold_refit;
    in.lds_bytes = h->lds_bytes; in.row_bytes = h->row_bytes; in.cl_lds = h->cl_lds;
    return in;
}

// Cluster launches of different streams are serialised per device: a launch whose workgroups are only partly resident
// spins on members that wait for a CU, and two such launches could wait for each other.  (Other kernels may share the
// device: they finish without the cluster's help.)  The lock covers [wait for the previous plan's event, this plan's
// launches, record]; nothing here blocks the host on the GPU.
struct ClusterGate {
    std::mutex mu;
    hipEvent_t ev[64] = {};
    bool have[64] = {};
    hipStream_t last[64] = {};
};
ClusterGate g_cluster_gate;

int launch_setup(tdmpc2_plan *h, const FusedRoute &r, int E, const float *z0, const float *task_emb, const float *prev_mean,
                 const unsigned char *t0, hipStream_t st) {
    SetupParams p{};
    p.E = E; p.H = h->cfg.horizon; p.A = h->cfg.action_dim; p.T = h->cfg.task_dim; p.multitask = h->cfg.multitask;
    p.nq = h->cfg.num_q; p.nnets = h->nnets; p.stride = h->stride; p.max_std = h->cfg.max_std;
    p.dyn = to_dev(h->dyn); p.rew = to_dev(h->rew); p.pi = to_dev(h->pi);
    for (int i = 0; i < h->cfg.num_q; ++i) p.q[i] = to_dev(h->q[i]);
    p.wemb[BE_DYN] = h->dyn.l[0].wemb; p.wemb[BE_REW] = h->rew.l[0].wemb; p.wemb[BE_PI] = h->pi.l[0].wemb;
    for (int i = 0; i < h->cfg.num_q; ++i) p.wemb[BE_Q0 + i] = h->q[i].l[0].wemb;
    p.z0 = z0; p.task_emb = task_emb; p.prev_mean = prev_mean; p.t0 = t0;
    p.beff = h->beff; p.cvec = h->cvec; p.mean = h->mean; p.std = h->std;
    p.cl_flags = r.arm_cl ? h->cl_flags : nullptr;
    p.cl_flag_words = h->tiles * 2 * CL_FLAG_STRIDE;
    p.cl2_flags = r.arm_cl2 ? h->cl2_flags : nullptr;
    p.cl2_flag_words = h->tiles * 4 * CL_FLAG_STRIDE;
    p.skip_cvec = r.skip_cvec ? 1 : 0;
    p.err_clear = h->cl_err_dev;  // word 0 of the error line back to zero, in stream order (fault_fresh)
    fused_ops(h->Apad).setup(h->split ? 0 : 1, p, E, h->lds_bytes, st);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the policy-prior pass of its own (whole plans that do not fold it into the first rollout launch, sharded plans)
int launch_pitraj(tdmpc2_plan *h, const FusedRoute &r, int E, const float *z0, const float *act_mask, const tdmpc2_noise *tape,
                  uint64_t seed, unsigned call, hipStream_t st) {
    const tdmpc2_plan_cfg &c = h->cfg;
    PiTrajParams p{};
    p.E = E; p.N = c.num_samples; p.H = c.horizon; p.A = c.action_dim; p.Apad = h->Apad; p.P = c.num_pi_trajs; p.stride = h->stride;
    p.multitask = c.multitask; p.nnets = h->nnets; p.log_std_min = c.log_std_min; p.log_std_dif = c.log_std_dif;
    p.dyn = to_dev(h->dyn); p.pi = to_dev(h->pi);
    p.z0 = z0; p.beff = h->beff; p.act_mask = act_mask; p.pi_traj_eps = tape ? tape->pi_traj_eps : nullptr;
    p.seed = seed; p.call = call; p.actions = h->actions; p.zscratch = h->zscratch;
    p.zscratch_estride = (long)h->tiles * ROWS * WIDTH;
    fused_ops(h->Apad).pitraj(h->split ? 0 : 1, r.pitraj_nst, p, E, r.pitraj_lds, st);
    HIP_TRY(hipGetLastError());
    return 0;
}

// what every rollout launch of a call shares; the route's row tiles
void fill_rollout(tdmpc2_plan *h, const FusedRoute &r, RolloutParams &p, int E) {
    const tdmpc2_plan_cfg &c = h->cfg;
    p.E = E; p.N = c.num_samples; p.H = c.horizon; p.A = c.action_dim; p.Apad = h->Apad; p.P = c.num_pi_trajs;
    p.stride = h->stride; p.tiles = r.tiles; p.tile_off = r.tile_off; p.nq = c.num_q; p.num_bins = c.num_bins; p.multitask = c.multitask;
    p.nnets = h->nnets; p.log_std_min = c.log_std_min; p.log_std_dif = c.log_std_dif;
    p.dyn = to_dev(h->dyn); p.rew = to_dev(h->rew); p.pi = to_dev(h->pi);
    if (c.episodic) p.term = to_dev(h->term);
    for (int i = 0; i < c.num_q; ++i) p.q[i] = to_dev(h->q[i]);
    p.bins = h->bins; p.beff = h->beff; p.cvec = h->cvec; p.mean = h->mean; p.std = h->std;
    p.actions = h->actions; p.value = h->value; p.zscratch = h->zscratch;
    p.ticket = h->ticket; p.fold_refit = 0;
    p.iters_total = c.iterations;
    p.timing = h->timing;
}
// the per-tile rollout launch of a route (ks_rollout; a trace call runs its tracing instantiation)
int launch_rollout(tdmpc2_plan *h, const FusedRoute &r, const RolloutParams &p, hipStream_t st) {
    fused_ops(h->Apad).rollout(h->split ? 0 : 1, r.nst, h->cfg.episodic != 0, p.trace_tiles || p.trace_scalars, p, r.grid, r.lds, st);
    HIP_TRY(hipGetLastError());
    return 0;
}

// A bounded inter-workgroup wait gave up (the handle's error word is set): the plan / call in flight returned NaN.  Switch to
// the paths without such waits, remember when, and let fault_clean() switch back after `rearm_after` clean calls.
// What the kernels run = what the caller asked for (user_*: environment at create, tdmpc2_plan_set_tuning) unless the handle is
// downgraded (a reported wait) or asked to plan once without inter-workgroup waits (TDMPC2_TUNE_SAFE_ONCE: the re-plan of a
// sharded plan).  The one place that writes cluster_mode / lay.fuse_ln after create.
void apply_modes(tdmpc2_plan *h) {
    const bool safe = h->degraded || h->safe_once;
    h->cluster_mode = safe ? 0 : h->user_cluster_mode;
    h->lay.fuse_ln = safe ? false : h->user_fuse_ln;
}
void fault_note(tdmpc2_plan *h) {
    if (h->degraded && h->rearm_after > 0 && h->rearm_after < 4096)
        h->rearm_after *= 2;  // (a fault on the downgraded paths cannot happen; this branch is a fault right after a re-arm raced in)
    h->degraded = true;
    apply_modes(h);
    h->clean_calls = 0;
    h->faults++;
    h->faults_total++;
    h->last_fault = std::chrono::steady_clock::now();
}
void fault_clean(tdmpc2_plan *h) {  // a call is about to be enqueued and no fault is pending
    if (!h->degraded) {  // a long clean run on the fast paths forgets the back-off
        if (h->rearm_after > h->rearm_base && ++h->clean_calls >= 16 * h->rearm_after) {
            h->rearm_after = h->rearm_base;
            h->clean_calls = 0;
        }
        return;
    }
    if (h->rearm_after <= 0 || h->in_shard) return;
    if (h->clean_calls < h->rearm_after) {  // this call still runs on the downgraded paths: rearm_after of them in all
        ++h->clean_calls;
        return;
    }
    h->degraded = false;
    apply_modes(h);
    h->clean_calls = 0;
    h->rearms++;
    if (h->rearm_after < 4096) h->rearm_after *= 2;  // the next downgrade lasts twice as long; a long clean run resets it (above)
}

// The host's look at the sticky word (common.cuh: raise_fault).  It never touches word 0 -- the verdict of the call in flight,
// which that call's own last kernel reads and the NEXT call clears in stream order (fault_fresh): calls of one handle may be
// pipelined without a sync and each still gets its own verdict.
bool fault_poll(tdmpc2_plan *h) {
    unsigned int *w = h->cl_err_host;
    // read-and-clear in ONE step: a device store that lands between a separate read and clear would be lost
    if (!w || !__atomic_exchange_n(w + 8, 0u, __ATOMIC_RELAXED)) return false;
    if (getenv("TDMPC2_DEBUG_FAULT")) fprintf(stderr, "[tdmpc2_plan] a bounded wait gave up: code 0x%08x (kind = code & 15)\n", w[0]);
    fault_note(h);
    return true;
}
// Start of a call that stands for itself (a plan, an estimate_value, a td_target ...; NOT the later calls of a sharded plan, whose
// final pick must still see a wait that gave up in its first iteration): word 0 back to zero, in stream order.  The fused
// family's ks_setup does it itself (SetupParams::err_clear).
int fault_fresh(tdmpc2_plan *h, hipStream_t st) {
    if (h->cl_err_dev) HIP_TRY(hipMemsetAsync(h->cl_err_dev, 0, 4, st));
    return 0;
}

int validate_envs(tdmpc2_plan *h, int E) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    if (E < 1 || E > h->cfg.max_envs) return fail(TDMPC2_ERR_INVALID, "n_envs=%d outside [1, max_envs=%d]", E, h->cfg.max_envs);
    // a cluster hand-over / fused-epilogue wait of an EARLIER call gave up (bounded wait): that plan returned NaN actions and kept
    // its prev_mean (refit_plan), that td_target / policy_value returned NaN; the handle now runs the paths without waits
    // until fault_clean() re-arms the fast ones.  tdmpc2_plan_take_fault / tdmpc2_plan_fault_info report it.
    if (!fault_poll(h)) fault_clean(h);
    return check_ready(h);
}


// The opening the training calls share (policy_value / td_target, model_rollout / model_losses, policy_loss), in this order: the
// task tables against the handle's kind (then `own`: the call's own refusals that sit there), bound weights, the sticky fault word,
// a fresh verdict word, the target ensemble, the call-counter tick.  `needs`: the call's name(s) and verb as the refusal words them.
template <class Own>
int begin_value_call(tdmpc2_plan *h, const char *needs, const tdmpc2_task_tables *tk, bool target, hipStream_t st, unsigned *call,
                     Own own) {
    const tdmpc2_plan_cfg &c = h->cfg;
    if (c.multitask) {
        if (!tk || !tk->task_ids || !tk->task_emb || !tk->act_mask || tk->n_tasks < 1)
            return fail(TDMPC2_ERR_INVALID, "multitask %s the row -> task map and the per-task tables", needs);
    } else if (tk) {
        return fail(TDMPC2_ERR_INVALID, "task tables given to a single-task handle");
    }
    int rc = own();
    if (rc) return rc;
    if ((rc = check_ready(h))) return rc;
    (void)fault_poll(h);  // (a wait that gave up in an earlier call: this one already runs on the paths without waits)
    // between the calls of a sharded plan word 0 is that plan's verdict (its final pick reads it): keep it
    if (!h->in_shard && (rc = fault_fresh(h, st))) return rc;
    if (target)
        for (int i = 0; i < 3; ++i)
            for (int qh = 0; qh < c.num_q; ++qh)
                if (!h->tq[qh].l[i].bound)
                    return fail(TDMPC2_ERR_STATE, "layer %d of target Q head %d is not bound (net TDMPC2_NET_TARGET_Q)", i, qh);
    *call = h->call++;  // (model_rollout / model_losses draw nothing: their tick keeps the siblings' numbering uniform)
    return 0;
}

// Everything of TDMPC2._plan after encode() (tdmpc2/tdmpc2.py:154-206) on the fused 512-wide path: fused_route_plan decides,
// this launches.
int fused_run(tdmpc2_plan *h, hipStream_t st, int E, const float *z0, const float *task_emb, const float *act_mask,
              const float *disc_pow, float *prev_mean, const uint8_t *t0, int eval_mode, const tdmpc2_noise *tape,
              uint64_t seed, float *action, const tdmpc2_debug *dbg) {
    const tdmpc2_plan_cfg &c = h->cfg;
    const int H = c.horizon, N = c.num_samples, A = c.action_dim, P = c.num_pi_trajs, I = c.iterations;
    const unsigned call = h->call++;
    int rc;
    const FusedRoute r = fused_route_plan(fused_in(h, E));
    const bool cluster = r.kind != FR_TILE;
    if ((rc = launch_setup(h, r, E, z0, task_emb, prev_mean, t0, st))) return rc;
    if (r.pitraj && (rc = launch_pitraj(h, r, E, z0, act_mask, tape, seed, call, st))) return rc;
    RolloutParams rp{};
    fill_rollout(h, r, rp, E);
    rp.z0 = z0; rp.act_mask = act_mask; rp.disc_pow = disc_pow; rp.seed = seed; rp.call = call; rp.given_actions = 0;
    rp.pi_fold = r.pi_fold ? 1 : 0;
    rp.pi_traj_eps = tape ? tape->pi_traj_eps : nullptr;
    rp.cl_xbuf = h->cl_xbuf; rp.cl_flags = h->cl_flags; rp.cl_err = h->cl_err_dev; rp.cl_zs = h->cl_zs;
    rp.cl_fault = h->cl_fault;
    rp.cl2_xbuf = h->cl2_xbuf; rp.cl2_flags = h->cl2_flags; rp.cl2_zs = h->cl2_zs; rp.cl2_mail = h->cl2_mail;
    rp.fold_refit = r.fold ? 1 : 0;
    std::unique_lock<std::mutex> gate;
    bool gate_record = false;
    const int gdev = c.device >= 0 && c.device < 64 ? c.device : 0;
    if (cluster) {
        gate = std::unique_lock<std::mutex>(g_cluster_gate.mu);
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(st, &cap);
        if (cap == hipStreamCaptureStatusNone) {  // (a captured plan replays on one stream: ordered by the graph itself)
            if (!g_cluster_gate.have[gdev]) {
                HIP_TRY(hipEventCreateWithFlags(&g_cluster_gate.ev[gdev], hipEventDisableTiming));
                g_cluster_gate.have[gdev] = true;
                g_cluster_gate.last[gdev] = st;
            } else if (g_cluster_gate.last[gdev] != st) {
                HIP_TRY(hipStreamWaitEvent(st, g_cluster_gate.ev[gdev], 0));
            }
            gate_record = true;
        }
    }
    for (int it = 0; it < I; ++it) {
        rp.iter = it;
        if (tape) {
            rp.sample_eps = tape->sample_eps + (size_t)it * H * (N - P) * A;
            rp.sample_eps_estride = (long)I * H * (N - P) * A;
            rp.pi_eps = tape->pi_eps + (size_t)it * N * A;
            rp.pi_eps_estride = (long)I * N * A;
            rp.qidx = tape->qidx + (size_t)it * 2;
            rp.qidx_estride = (long)I * 2;
        }
        RefitParams &fp = rp.rf;
        fill_refit(h, fp, E, it, eval_mode, h->value, act_mask, tape, seed, call, prev_mean, action, dbg, r.refit_stage,
                   cluster ? h->cl_err_dev : nullptr);
        if (r.fold) {
            fp.regen = 1; fp.P = P; fp.Apad = h->Apad;
            fp.sample_eps = rp.sample_eps; fp.sample_eps_estride = rp.sample_eps_estride;
        }
        if (h->profiling && h->ev_used + 2 <= (int)h->ev.size()) HIP_TRY(hipEventRecord(h->ev[h->ev_used], st));
        if (r.kind == FR_TILE) {
            if ((rc = launch_rollout(h, r, rp, st))) return rc;
        } else {
            if (r.kind == FR_CLUSTER2) cluster_ops(h->Apad).rollout_cl2(rp, r.grid, r.lds, st);
            else cluster_ops(h->Apad).rollout_cl(c.episodic != 0, rp, r.grid, r.lds, st);
            HIP_TRY(hipGetLastError());
        }
        if (h->profiling && h->ev_used + 2 <= (int)h->ev.size()) {
            HIP_TRY(hipEventRecord(h->ev[h->ev_used + 1], st));
            h->ev_used += 2;
        }
        if (!r.fold && (rc = launch_refit(fp, E, N, r.refit_lds, st))) return rc;
        // the per-iteration action dump reads h->actions after the refit (which does not write them)
        if ((rc = dump_actions(h, dbg, E, it, st))) return rc;
    }
    if (gate_record) {
        HIP_TRY(hipEventRecord(g_cluster_gate.ev[gdev], st));
        g_cluster_gate.last[gdev] = st;
    }
    return TDMPC2_OK;
}

// TDMPC2._estimate_value (tdmpc2/tdmpc2.py:122-136) on given action sequences, fused path.
int fused_estimate_value(tdmpc2_plan *h, hipStream_t st, int E, const float *z0, const float *task_emb,
                         const float *act_mask, const float *disc_pow, const float *actions, const float *pi_eps,
                         const int32_t *qidx, float *value, float *trace_tiles, float *trace_scalars) {
    const tdmpc2_plan_cfg &c = h->cfg;
    const int N = c.num_samples, A = c.action_dim;
    int rc;
    const FusedRoute r = fused_route_value(fused_in(h, E), trace_tiles != nullptr || trace_scalars != nullptr);
    // setup needs prev_mean / t0 only for mean/std init, which this entry does not use: feed dummies
    HIP_TRY(hipMemsetAsync(h->mean, 0, (size_t)E * c.horizon * A * 4, st));
    HIP_TRY(hipMemsetAsync(h->value, 1, (size_t)E, st));  // E bytes of ones used as t0 = 1 flags (no warm start read)
    if ((rc = launch_setup(h, r, E, z0, task_emb, h->mean, reinterpret_cast<const unsigned char *>(h->value), st))) return rc;
    RolloutParams rp{};
    fill_rollout(h, r, rp, E);
    rp.z0 = z0; rp.act_mask = act_mask; rp.disc_pow = disc_pow; rp.given_actions = 1; rp.iter = 0;
    rp.actions = const_cast<float *>(actions);
    rp.value = value;
    rp.pi_eps = pi_eps; rp.pi_eps_estride = (long)N * A;
    rp.qidx = qidx; rp.qidx_estride = 2;
    rp.trace_tiles = trace_tiles; rp.trace_scalars = trace_scalars;
    return launch_rollout(h, r, rp, st);
}

}  // namespace

namespace {
int run_impl(tdmpc2_plan *h, int n_envs, const float *z0, const float *task_emb, const float *act_mask, const float *disc_pow,
             float *prev_mean, const uint8_t *t0, int eval_mode, const tdmpc2_noise *tape, uint64_t seed, float *action,
             const tdmpc2_debug *dbg, void *stream);
}

namespace {
// ---- what tdmpc2_plan_create does around plan_layout (plan_layout.h decides; these touch the process and the device)
// The creation-time switches of this process's environment, read once at the top of create.
CreateEnv read_create_env() {
    CreateEnv e;
    e.one_stream = getenv("TDMPC2_ONE_STREAM") != nullptr;
    if (const char *fl = getenv("TDMPC2_FUSE_LN")) e.fuse_ln = atoi(fl) != 0;
    if (const char *ks = getenv("TDMPC2_KSPLIT")) e.ksplit = std::min(2, std::max(0, atoi(ks)));
    if (const char *fr = getenv("TDMPC2_FEWROW")) e.fewrow = atoi(fr) != 0;
    if (const char *cm = getenv("TDMPC2_CLUSTER")) e.cluster = atoi(cm);
#ifdef GW_TIMING
    e.gw_timing = getenv("TDMPC2_GW_TIMING") != nullptr;
#endif
#ifdef SPLIT_TIMING
    e.timing = getenv("TDMPC2_TIMING") != nullptr;
#endif
    return e;
}

// The handle's field for a buffer of the layout.
void **buf_field(tdmpc2_plan *h, PlanBufId id) {
    Layered &L = h->lay;
#define PB_FIELD(ID, FIELD) case ID: return (void **)&(FIELD)
    switch (id) {
        PB_FIELD(PB_BINS, h->bins); PB_FIELD(PB_ACTIONS, h->actions); PB_FIELD(PB_VALUE, h->value); PB_FIELD(PB_MEAN, h->mean);
        PB_FIELD(PB_STD, h->std); PB_FIELD(PB_TICKET, h->ticket); PB_FIELD(PB_QIDX_BUF, h->qidx_buf); PB_FIELD(PB_ONE, h->one);
        PB_FIELD(PB_BEFF, h->beff); PB_FIELD(PB_CVEC, h->cvec); PB_FIELD(PB_ZSCRATCH, h->zscratch);
        PB_FIELD(PB_CL_XBUF, h->cl_xbuf); PB_FIELD(PB_CL_ZS, h->cl_zs); PB_FIELD(PB_CL_FLAGS, h->cl_flags);
        PB_FIELD(PB_CL2_XBUF, h->cl2_xbuf); PB_FIELD(PB_CL2_ZS, h->cl2_zs); PB_FIELD(PB_CL2_FLAGS, h->cl2_flags); PB_FIELD(PB_CL2_MAIL, h->cl2_mail);
        PB_FIELD(PB_X, L.X); PB_FIELD(PB_HA, L.HA); PB_FIELD(PB_HB, L.HB); PB_FIELD(PB_LG, L.LG); PB_FIELD(PB_G, L.G); PB_FIELD(PB_QT, L.QT);
        PB_FIELD(PB_TERM, L.TERM); PB_FIELD(PB_QIDX, L.qidx); PB_FIELD(PB_Z0X, L.Z0X); PB_FIELD(PB_LCVEC, L.cvec);
        PB_FIELD(PB_HA2, L.HA2); PB_FIELD(PB_HB2, L.HB2); PB_FIELD(PB_LG2, L.LG2);
        PB_FIELD(PB_STATS, L.stats); PB_FIELD(PB_STATS2, L.stats2); PB_FIELD(PB_ARRIVE, L.arrive); PB_FIELD(PB_MWS0, L.mws[0]);
        PB_FIELD(PB_MWS1, L.mws[1]); PB_FIELD(PB_PRE, L.PRE); PB_FIELD(PB_PRE2, L.PRE2);
        case PB_COUNT: break;
    }
#undef PB_FIELD
    return nullptr;
}

// The host-mapped error line of the bounded waits (cluster path, fused NormedLinear epilogue): allocated, zeroed, mapped.
int err_line_create(tdmpc2_plan *h) {
    if (hipHostMalloc((void **)&h->cl_err_host, 64, hipHostMallocMapped) != hipSuccess)
        return fail(TDMPC2_ERR_HIP, "allocating the error line of the bounded waits failed");
    memset(h->cl_err_host, 0, 64);  // hipHostMalloc does not zero: word 0 (verdict) AND word 8 (sticky, fault_poll)
    if (hipHostGetDevicePointer((void **)&h->cl_err_dev, h->cl_err_host, 0) != hipSuccess)
        return fail(TDMPC2_ERR_HIP, "hipHostGetDevicePointer failed");
    return 0;
}
}  // namespace

extern "C" {

int tdmpc2_plan_abi_version(void) { return TDMPC2_PLAN_ABI_VERSION; }
const char *tdmpc2_last_error(void) { return g_err.c_str(); }

int tdmpc2_plan_create(const tdmpc2_plan_cfg *cfg, tdmpc2_plan_t **out) {
    if (!cfg || !out) return fail(TDMPC2_ERR_INVALID, "null argument");
    *out = nullptr;
    const tdmpc2_plan_cfg &c = *cfg;
    const CreateEnv env = read_create_env();
    int num_cus = 0;  // (a property of the device, read without making it current; plan_layout falls back where there is none)
    if (hipDeviceGetAttribute(&num_cus, hipDeviceAttributeMultiprocessorCount, c.device) != hipSuccess) num_cus = 0;
    // every configuration check, the kernel family, the arithmetic and every size: plan_layout.h
    const PlanLayout lo = plan_layout(c, num_cus, env);
    if (lo.err) return fail(lo.err, "%s", lo.msg);
    DevGuard dev_(c.device);
    if (!dev_.ok) return fail(TDMPC2_ERR_HIP, "hipSetDevice(%d) failed", c.device);

    tdmpc2_plan *h = new (std::nothrow) tdmpc2_plan();
    if (!h) return fail(TDMPC2_ERR_INVALID, "out of host memory");
    Layered &L = h->lay;
    h->cfg = c;
    h->cfg.path = lo.path;
    h->cfg.precision = lo.precision;
    L.on = lo.layered;
    L.qarr = h->q;
    h->split = lo.split;
    h->num_cus = num_cus;
    h->Apad = lo.Apad; h->tiles = lo.tiles; h->nnets = lo.nnets; h->stride = lo.stride;
    h->row_bytes = lo.row_bytes; h->lds_bytes = lo.lds_bytes; h->cl_lds = lo.cl_lds; h->cl_max_clusters = lo.cl_max_clusters;
    L.Kin = lo.Kin; L.Mp = lo.Mp; L.ldl = lo.ldl; L.Ppad = lo.Ppad; L.ldpre = lo.ldpre;
    L.cvec_rows = lo.cvec_rows; L.stats_cap = lo.stats_cap; L.arrive_cap = lo.arrive_cap; L.ks_tiles = lo.ks_tiles; L.mws_cap = lo.mws_cap;

    struct Undo {  // whatever follows fails: the handle and all it owns so far go
        tdmpc2_plan *h;
        ~Undo() { if (h) tdmpc2_plan_destroy(h); }
    } undo{h};
    int rc = 0;
    for (int i = 0; i < lo.nbuf; ++i) {
        const PlanBuf &b = lo.buf[i];
        void **p = buf_field(h, b.id);
        if ((rc = dev_alloc(h, p, b.bytes))) return rc;
        if (b.zero && hipMemset(*p, 0, b.bytes) != hipSuccess) return fail(TDMPC2_ERR_HIP, "hipMemset(%s) failed", b.name);
    }
    if (L.on) L.bias_tab = h->beff;
    // torch.linspace(vmin, vmax, num_bins) in fp32 (math.py:80): float step, product rounded once
    std::vector<float> bins(c.num_bins > 1 ? c.num_bins : 2, 0.f);
    if (c.num_bins > 1) {
        const float step = (c.vmax - c.vmin) / (float)(c.num_bins - 1);
        for (int i = 0; i < c.num_bins; ++i)
            bins[i] = (i < c.num_bins / 2) ? (float)((double)c.vmin + (double)step * i)
                                           : (float)((double)c.vmax - (double)step * (c.num_bins - 1 - i));
    }
    if (hipMemcpy(h->bins, bins.data(), bins.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail(TDMPC2_ERR_HIP, "hipMemcpy(bins) failed");
    const float one = 1.f;
    if (h->one && hipMemcpy(h->one, &one, 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail(TDMPC2_ERR_HIP, "allocating the unit output scale failed");
    if (lo.second_chain) {
        SideRes sr;
        if (!side_acquire(c.device, &sr)) return fail(TDMPC2_ERR_HIP, "creating the second stream of the layered path failed");
        L.side = sr.stream; L.ev_fork = sr.ev[0]; L.ev_side = sr.ev[1]; L.ev_xread = sr.ev[2];
    }
    if (lo.err_line && (rc = err_line_create(h))) return rc;
    if (hipEventCreateWithFlags(&h->turn_ev, hipEventDisableTiming) != hipSuccess) {  // (StreamTurn)
        h->turn_ev = nullptr;
        return fail(TDMPC2_ERR_HIP, "hipEventCreate failed");
    }
    if (pl_set_lds()) return TDMPC2_ERR_HIP;  // (both families: the running scale's key array)
    if (!L.on) {
        const int ar = h->split ? 0 : 1;
        rc = fused_ops(h->Apad).set_lds(ar, c.episodic, h->lds_bytes);
        if (!rc) rc = model_ops(h->Apad).set_lds(ar, h->lds_bytes);
        if (!rc) rc = policy_loss_ops(h->Apad).set_lds(ar, h->lds_bytes);
        if (!rc && h->cl_max_clusters) rc = cluster_ops(h->Apad).set_lds(c.episodic, h->cl_lds);
        if (rc) return TDMPC2_ERR_HIP;
    }
    if (L.on && h->split) {
        L.fuse_ln = env.fuse_ln;
        L.ksplit = env.ksplit;
        L.mid = env.fewrow;
        if ((rc = ksws_ensure(h, L.ksplit))) return rc;
        if (env.gw_timing) {
            if ((rc = dev_alloc(h, (void **)&L.gw_timing, 32 * 8))) return rc;
            if (hipMemset(L.gw_timing, 0, 32 * 8) != hipSuccess) return fail(TDMPC2_ERR_HIP, "hipMemset failed");
        }
    }
    h->cluster_mode = env.cluster;
    h->user_cluster_mode = h->cluster_mode;  // what was asked for (environment or default); set_tuning / fault recovery go through apply_modes
    h->user_fuse_ln = L.fuse_ln;
#ifdef TDMPC2_TEST_HOOKS  // libtdmpc2_plan_hooks.so (built beside the product library, loaded by the GPU tests of the fault paths only)
    if (const char *cf = getenv("TDMPC2_CLUSTER_FAULT")) h->cl_fault = atoi(cf);
#endif
    if (h->cl_fault) L.mid = false;  // the hook mutes a workgroup of the WAITING paths: the handle runs them (the few-row path has no waits)
    // in-kernel phase timers exist in -DSPLIT_TIMING builds only (tools/ablate.sh)
    if (env.timing && dev_alloc(h, (void **)&h->timing, 16 * 8) == 0) (void)hipMemset(h->timing, 0, 16 * 8);
    undo.h = nullptr;
    *out = h;
    return TDMPC2_OK;
}

void tdmpc2_plan_destroy(tdmpc2_plan_t *h) {
    if (!h) return;
    DevGuard dev_(h->cfg.device);
    if (h->timing) {  // in-kernel phase timers of a -DSPLIT_TIMING build (tools/ablate.sh)
        unsigned long long t[16];
        if (hipMemcpy(t, h->timing, sizeof t, hipMemcpyDeviceToHost) == hipSuccess && t[15] > 0) {
            static const char *names[16] = {"kloop", "epi_post", "head", "actions", "park/unpark", "tile_from_global", "epi_stats", "epi_sync",
                                            "epi_bias", "epi_combine", "epi_math_store", "cluster_wait", "head_kloop", "head_stage", "total", "workgroups"};
            fprintf(stderr, "[tdmpc2_plan timing max_envs=%d] mean cycles per workgroup (one wave, SPLIT_TIMING_WAVE):", h->cfg.max_envs);
            for (int i = 0; i < 15; ++i)
                if (names[i][0]) fprintf(stderr, " %s=%.0f", names[i], (double)t[i] / (double)t[15]);
            fprintf(stderr, "\n");
        }
    }
    if (h->lay.gw_timing) {  // phase clocks of g_gemm_w (-DGW_TIMING build + TDMPC2_GW_TIMING=1)
        unsigned long long t[32];
        if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(t, h->lay.gw_timing, sizeof t, hipMemcpyDeviceToHost) == hipSuccess) {
            static const char *cls[4] = {"mish K<1024", "mish K>=1024", "simnorm K<1024", "simnorm K>=1024"};
            for (int c = 0; c < 4; ++c) {
                const unsigned long long *q = t + 8 * c;
                if (!q[6]) continue;
                const double n = (double)q[6];
                fprintf(stderr, "[g_gemm_w timing max_envs=%d, %s] workgroups=%llu mean cycles of wave 0: loop_end=%.0f stats_stored=%.0f "
                        "peers_arrived=%.0f row_stats=%.0f end=%.0f\n", h->cfg.max_envs, cls[c], q[6], q[1] / n, q[2] / n, q[3] / n, q[4] / n, q[5] / n);
            }
        }
    }
    if (h->lay.side) {  // back to the pool, never destroyed (see SidePool)
        SideRes sr;
        sr.stream = h->lay.side; sr.ev[0] = h->lay.ev_fork; sr.ev[1] = h->lay.ev_side; sr.ev[2] = h->lay.ev_xread;
        side_release(h->cfg.device, sr);
    }
    for (void *p : h->allocs) (void)hipFree(p);
    if (h->cl_err_host) (void)hipHostFree(h->cl_err_host);
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    if (h->turn_ev) (void)hipEventDestroy(h->turn_ev);
    delete h;
}

uint64_t tdmpc2_plan_device_bytes(const tdmpc2_plan_t *h) { return h ? h->bytes : 0; }
int tdmpc2_plan_path(const tdmpc2_plan_t *h) { return h ? h->cfg.path : -1; }
int tdmpc2_plan_precision(const tdmpc2_plan_t *h) { return h ? h->cfg.precision : -1; }

namespace {
// Shape of one nn.Linear of the world model as the planner stores it (tdmpc2/common/world_model.py:26-30).
struct LayerShape {
    int in, out;      // nn.Linear in_features / out_features
    int nz, nt, na;   // source columns: latent or hidden | task embedding | action
    int KB, CT;
    bool has_ln, mish;  // LayerNorm after the Linear; Mish (hidden layers) as opposed to SimNorm / none
    int heads;
    size_t wsz /* floats' worth of packed weights per head */, bsz, gsz, esz;
};
LayerShape layer_shape(const tdmpc2_plan *h, int net, int layer) {
    const tdmpc2_plan_cfg &c = h->cfg;
    LayerShape s{};
    const bool is_q = net == TDMPC2_NET_Q || net == TDMPC2_NET_TARGET_Q;
    const bool takes_action = (net == TDMPC2_NET_DYNAMICS || net == TDMPC2_NET_REWARD || is_q);
    s.heads = is_q ? c.num_q : 1;
    if (layer == 0) {
        s.in = c.latent_dim + c.task_dim + (takes_action ? c.action_dim : 0);
        s.out = c.mlp_dim;
    } else if (layer == 1) {
        s.in = c.mlp_dim;
        s.out = c.mlp_dim;
    } else {
        s.in = c.mlp_dim;
        s.out = net == TDMPC2_NET_DYNAMICS ? c.latent_dim : net == TDMPC2_NET_PI ? 2 * c.action_dim
                : net == TDMPC2_NET_TERMINATION ? 1 : (c.num_bins > 1 ? c.num_bins : 1);
    }
    s.has_ln = (layer < 2) || net == TDMPC2_NET_DYNAMICS;
    s.mish = layer < 2;
    s.nz = (layer == 0) ? c.latent_dim : c.mlp_dim;
    s.nt = (layer == 0) ? c.task_dim : 0;
    s.na = (layer == 0 && takes_action) ? c.action_dim : 0;
    // packed contraction length: the fused kernels pad the action columns to 16, the layered GEMMs the whole row to GBK
    const int Kp = h->lay.on ? (int)round_up((size_t)s.nz + s.na, GBK) : s.nz + (s.na + 15) / 16 * 16;
    s.KB = h->split ? Kp / 16 : Kp / 8;
    s.CT = (s.out + 31) / 32;
    s.wsz = h->split ? (size_t)s.CT * s.KB * 512 /* floats' worth of 1024 halfs */ : (size_t)s.CT * s.KB * 256;
    s.bsz = (size_t)s.CT * 32;
    s.gsz = round_up((size_t)s.out, 4);
    s.esz = (size_t)s.out * (s.nt > 0 ? s.nt : 0);
    return s;
}

// One slab per tensor kind holding all ensemble members at a constant stride (the layered GEMM selects a member per plan
// by stride); allocated on the first bind (or import) of a (net, layer).
int ensure_layer_alloc(tdmpc2_plan *h, int net, int layer, const LayerShape &sh) {
    HostLayer &L0 = net_of(h, net, 0)->l[layer];
    if (L0.alloc) return 0;
    int rc;
    if (h->split && !net_of(h, net, 0)->scal) {  // the net's [heads][3] scalar table, defaults: scales 2^5, kw 0
        LayerScal *tab = nullptr;
        if ((rc = dev_alloc(h, (void **)&tab, (size_t)sh.heads * 3 * sizeof(LayerScal)))) return rc;
        std::vector<LayerScal> init((size_t)sh.heads * 3, LayerScal{1.f, 1.f / ACT_SCALE, 0u, 0, ACT_SCALE, ACT_SCALE_LOG2, 0u, 0u});
        HIP_TRY(hipMemcpy(tab, init.data(), init.size() * sizeof(LayerScal), hipMemcpyHostToDevice));
        for (int hd = 0; hd < sh.heads; ++hd) net_of(h, net, hd)->scal = tab + (size_t)hd * 3;
    }
    float *wslab = nullptr, *bslab = nullptr, *gslab = nullptr, *betaslab = nullptr, *eslab = nullptr;
    if ((rc = dev_alloc(h, (void **)&wslab, sh.heads * sh.wsz * 4))) return rc;
    if ((rc = dev_alloc(h, (void **)&bslab, sh.heads * sh.bsz * 4))) return rc;
    if (sh.has_ln) {
        if ((rc = dev_alloc(h, (void **)&gslab, sh.heads * sh.gsz * 4))) return rc;
        if ((rc = dev_alloc(h, (void **)&betaslab, sh.heads * sh.gsz * 4))) return rc;
    }
    if (sh.nt > 0 && (rc = dev_alloc(h, (void **)&eslab, sh.heads * sh.esz * 4))) return rc;
    for (int hd = 0; hd < sh.heads; ++hd) {
        HostNet *N = net_of(h, net, hd);
        HostLayer &L = N->l[layer];
        L.alloc = true;
        L.KB = sh.KB; L.CT = sh.CT; L.out = sh.out;
        L.wbytes = sh.wsz * 4;
        if (h->split) {
            L.wps = reinterpret_cast<_Float16 *>(wslab + hd * sh.wsz);
            L.scal = N->scal + layer;
            L.oscale = &L.scal->oscale;
            L.ascale = &L.scal->ascale;
        } else {
            L.wp = wslab + hd * sh.wsz;
            L.oscale = h->one;  // the exact arithmetic has no scales
            L.ascale = h->one;
        }
        L.bias = bslab + hd * sh.bsz;
        L.g = sh.has_ln ? gslab + hd * sh.gsz : nullptr;
        L.b = sh.has_ln ? betaslab + hd * sh.gsz : nullptr;
        L.wemb = sh.nt > 0 ? eslab + hd * sh.esz : nullptr;
    }
    return 0;
}

int ensure_enc_alloc(tdmpc2_plan *h, int layer, int in_features, int out_features) {
    const tdmpc2_plan_cfg &c = h->cfg;
    tdmpc2_plan::Enc &L = h->enc[layer];
    if (in_features > ENC_MAX_IN)  // binds and packed blobs both come through here, before anything is allocated or enqueued
        return fail(TDMPC2_ERR_UNSUPPORTED, "encoder layer %d: %d inputs, at most %d (a layer's input row is held in %zu bytes of LDS)",
                    layer, in_features, ENC_MAX_IN, ENC_GEMV_LDS_MAX);
    if (L.wt && (L.in != in_features || L.out != out_features))
        return fail(TDMPC2_ERR_STATE, "encoder layer %d re-bound with a different shape", layer);
    int rc;
    if (!L.wt) {
        if ((rc = dev_alloc(h, (void **)&L.wt, (size_t)in_features * out_features * 4))) return rc;
        if ((rc = dev_alloc(h, (void **)&L.bias, (size_t)out_features * 4))) return rc;
        if ((rc = dev_alloc(h, (void **)&L.g, (size_t)out_features * 4))) return rc;
        if ((rc = dev_alloc(h, (void **)&L.b, (size_t)out_features * 4))) return rc;
        L.in = in_features;
        L.out = out_features;
    }
    if (!h->zenc && (rc = dev_alloc(h, (void **)&h->zenc, (size_t)c.max_envs * c.latent_dim * 4))) return rc;
    const int w = std::max(in_features, out_features);
    if (w > ENC_WIDE && w > h->enc_ws_width) {  // workspace of the layer-at-a-time encoder path (grows with the widest layer)
        if ((rc = dev_alloc(h, (void **)&h->enc_y, (size_t)c.max_envs * w * 4))) return rc;
        if ((rc = dev_alloc(h, (void **)&h->enc_x, (size_t)c.max_envs * w * 4))) return rc;
        h->enc_ws_width = w;
    }
    return 0;
}

// ================================================================ the weight packer's host side (k_refresh.hip: refresh_kernels.cuh, refresh_route.h)
// Every entry point that stores weights describes JOBS -- one per (net, layer) with every ensemble member inside it, one per
// transposed copy (a state-encoder layer, a layer of the policy prior's fp32 copy) -- and hands them to run_jobs.  The entry
// points differ only in how they collect jobs: the per-layer binds describe one, the table calls walk their table.  Each kind
// of job has ONE function that checks it, allocates its first-time storage and appends it; everything that can refuse,
// refuses before anything is enqueued.
struct RfJobs {
    RfParams p{};
    unsigned nets = 0;          // nets with a named layer
    unsigned enc = 0, pol = 0;  // state-encoder / policy-copy layers among p.tr
    int nenc = 0;               // the encoder depth its layers were checked against
    explicit RfJobs(const tdmpc2_plan *h) {
        p.split = h->split ? 1 : 0;
        p.lerp_net = -1;
    }
};

// one nn.Linear of a net (+ its LayerNorm), every ensemble member: `e` in the checkpoint's layout, stacked over heads
int add_net_layer(tdmpc2_plan *h, RfJobs &j, int net, int l, const tdmpc2_weight_entry &e) {
    if (net == TDMPC2_NET_TERMINATION && !h->cfg.episodic)
        return fail(TDMPC2_ERR_INVALID, "termination head bound on a non-episodic planner");
    const LayerShape sh = layer_shape(h, net, l);
    if (!e.W || !e.b) return fail(TDMPC2_ERR_INVALID, "net %d is named but layer %d lacks its weight or bias", net, l);
    if (sh.has_ln && (!e.ln_g || !e.ln_b)) return fail(TDMPC2_ERR_INVALID, "net %d layer %d needs LayerNorm parameters", net, l);
    if (int rc = ensure_layer_alloc(h, net, l, sh)) return rc;
    const HostLayer &L0 = net_of(h, net, 0)->l[l];
    RfNet &N = j.p.net[net];
    RfLayer &J = N.l[l];
    J.W = e.W; J.b = e.b; J.g = sh.has_ln ? e.ln_g : nullptr; J.beta = sh.has_ln ? e.ln_b : nullptr;
    J.wdst = h->split ? reinterpret_cast<float *>(L0.wps) : L0.wp;
    J.bias = L0.bias; J.gd = L0.g; J.bd = L0.b; J.wemb = L0.wemb;
    J.out = sh.out; J.in = sh.in; J.nz = sh.nz; J.nt = sh.nt; J.na = sh.na; J.CT = sh.CT; J.KB = sh.KB;
    J.has_ln = sh.has_ln ? 1 : 0; J.mish = sh.mish ? 1 : 0;
    J.scan_nbw = rf_scan_wblocks((long)sh.out * sh.in);
    N.heads = sh.heads;
    N.scal = h->split ? net_of(h, net, 0)->scal : nullptr;
    N.mask |= 1 << l;
    j.nets |= 1u << net;
    return 0;
}

// layer `l` of a state encoder of `nenc` layers
int add_enc_layer(tdmpc2_plan *h, RfJobs &j, int l, int nenc, const tdmpc2_weight_entry &e, int out_features, int in_features) {
    const tdmpc2_plan_cfg &c = h->cfg;
    if (nenc < 1 || nenc > ENC_MAX_LAYERS) return fail(TDMPC2_ERR_INVALID, "encoder depth %d outside [1, %d]", nenc, ENC_MAX_LAYERS);
    if (l < 0 || l >= nenc) return fail(TDMPC2_ERR_INVALID, "encoder layer %d outside [0, %d)", l, nenc);
    if (!e.W || !e.b || !e.ln_g || !e.ln_b) return fail(TDMPC2_ERR_INVALID, "encoder layer %d: null tensor", l);
    if (out_features < 1 || out_features > ENC_THREADS * ENC_MAX_PER_THREAD || in_features < 1)
        return fail(TDMPC2_ERR_UNSUPPORTED, "encoder layer %d: width %d outside [1, %d]", l, out_features, ENC_THREADS * ENC_MAX_PER_THREAD);
    if (l == nenc - 1 && out_features != c.latent_dim)
        return fail(TDMPC2_ERR_INVALID, "the last encoder layer has %d outputs, latent_dim is %d", out_features, c.latent_dim);
    if (l == nenc - 1 && (c.latent_dim % c.simnorm_dim || (c.simnorm_dim & (c.simnorm_dim - 1)) || c.simnorm_dim > 64))
        return fail(TDMPC2_ERR_UNSUPPORTED, "SimNorm groups of %d over %d latents", c.simnorm_dim, c.latent_dim);
    if (h->enc_layers && h->enc_layers != nenc) return fail(TDMPC2_ERR_STATE, "encoder depth changed from %d to %d", h->enc_layers, nenc);
    if (int rc = ensure_enc_alloc(h, l, in_features, out_features)) return rc;  // refuses a re-bind with another shape
    const tdmpc2_plan::Enc &E = h->enc[l];
    j.p.tr[j.p.ntrans++] = RfTrans{e.W, e.b, e.ln_g, e.ln_b, E.wt, E.bias, E.g, E.b, E.out, E.in};
    j.enc |= 1u << l;
    j.nenc = nenc;
    return 0;
}

// layer `l` of the policy prior's fp32 copy; its buffers exist (tdmpc2_plan_bind_policy) and `e` has passed that call's checks
// or add_net_layer(TDMPC2_NET_PI)'s, which ask the same of it
void add_pol_layer(tdmpc2_plan *h, RfJobs &j, int l, const tdmpc2_weight_entry &e) {
    const bool ln = l < 2;
    const tdmpc2_plan_cfg &c = h->cfg;
    const tdmpc2_plan::Pol &P = h->pol;
    j.p.tr[j.p.ntrans++] = RfTrans{e.W, e.b, ln ? e.ln_g : nullptr, ln ? e.ln_b : nullptr, P.wt[l], P.bias[l], ln ? P.g[l] : nullptr,
                                   ln ? P.b[l] : nullptr, l == 2 ? 2 * c.action_dim : c.mlp_dim, l == 0 ? c.latent_dim + c.task_dim : c.mlp_dim};
    j.pol |= 1u << l;
}

// The launches refresh_route lists over the jobs' workgroup ranges, then the bound flags of exactly the jobs that ran.
int run_jobs(tdmpc2_plan *h, RfJobs &j, hipStream_t st) {
    RfParams &p = j.p;
    const bool pi = j.nets >> TDMPC2_NET_PI & 1;
    const RefreshRoute route = refresh_route(RefreshIn{p.split, j.nets, __builtin_popcount(j.enc), j.pol && pi, p.lerp_net >= 0,
                                                       h->cfg.num_q, h->cfg.episodic, j.pol && !pi});
    long sb = 0, pb = 0;
    for (int net = 0; net < RF_NETS; ++net)
        for (int l = 0; l < 3; ++l) {
            const RfNet &N = p.net[net];
            const RfLayer &J = N.l[l];
            p.scan_blk0[net * 3 + l] = (int)sb;
            p.pack_blk0[net * 3 + l] = (int)pb;
            if (!(N.mask >> l & 1)) continue;
            sb += (long)N.heads * (J.scan_nbw + 1);
            pb += (long)N.heads * rf_pack_blocks(J.CT, J.KB * (p.split ? 16 : 8), J.nt);
        }
    p.scan_blk0[3 * RF_NETS] = (int)sb;
    for (int t = 0; t < RF_MAX_TRANS; ++t) {
        p.pack_blk0[3 * RF_NETS + t] = (int)pb;
        if (t < p.ntrans) pb += rf_transpose_blocks(p.tr[t].out, p.tr[t].in);
    }
    p.pack_blk0[RF_SEGS] = (int)pb;
    if (pb > 0x7fffffffL || sb > 0x7fffffffL) return fail(TDMPC2_ERR_UNSUPPORTED, "weight refresh: %ld workgroups", pb);
    for (int i = 0; i < route.nops; ++i)
        if (int rc = tdk::refresh_launch(route.op[i], p, st)) return rc;
    for (int net = 0; net < RF_NETS; ++net)
        for (int l = 0; l < 3; ++l)
            if (p.net[net].mask >> l & 1)
                for (int hd = 0; hd < p.net[net].heads; ++hd) net_of(h, net, hd)->l[l].bound = true;
    for (int l = 0; l < ENC_MAX_LAYERS; ++l)
        if (j.enc >> l & 1) h->enc[l].bound = true;
    if (j.enc) h->enc_layers = j.nenc;
    for (int l = 0; l < 3; ++l)
        if (j.pol >> l & 1) h->pol.bound[l] = true;
    return TDMPC2_OK;
}
}  // namespace

int tdmpc2_plan_bind_weights(tdmpc2_plan_t *h, int net, int layer, const float *W, const float *b, const float *ln_g,
                             const float *ln_b, int out_features, int in_features, void *stream) {
    if (!h || !W || !b) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (layer < 0 || layer > 2) return fail(TDMPC2_ERR_INVALID, "layer %d outside [0, 2]", layer);
    if (net < TDMPC2_NET_DYNAMICS || net > TDMPC2_NET_TARGET_Q) return fail(TDMPC2_ERR_INVALID, "unknown net %d", net);
    ENTER_ON(h, stream);
    const LayerShape sh = layer_shape(h, net, layer);  // the caller states the shape: it must be the handle's
    if (in_features != sh.in || out_features != sh.out)
        return fail(TDMPC2_ERR_INVALID, "net %d layer %d: got [%d, %d], expected [%d, %d]", net, layer, out_features,
                    in_features, sh.out, sh.in);
    RfJobs j(h);
    if (int rc = add_net_layer(h, j, net, layer, tdmpc2_weight_entry{W, b, ln_g, ln_b})) return rc;
    return run_jobs(h, j, (hipStream_t)stream);
}

int tdmpc2_plan_bind_encoder(tdmpc2_plan_t *h, int layer, int n_layers, const float *W, const float *b, const float *ln_g,
                             const float *ln_b, int out_features, int in_features, void *stream) {
    if (!h || !W || !b || !ln_g || !ln_b) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    RfJobs j(h);
    if (int rc = add_enc_layer(h, j, layer, n_layers, tdmpc2_weight_entry{W, b, ln_g, ln_b}, out_features, in_features)) return rc;
    return run_jobs(h, j, (hipStream_t)stream);
}

namespace {
int launch_encode(tdmpc2_plan *h, int E, const float *obs, int obs_dim, const float *task_emb, float *z, hipStream_t st) {
    const tdmpc2_plan_cfg &c = h->cfg;
    if (!h->enc_layers) return fail(TDMPC2_ERR_STATE, "no encoder bound (tdmpc2_plan_bind_encoder)");
    EncodeParams p{};
    int maxw = 0;
    for (int l = 0; l < h->enc_layers; ++l) {
        const tdmpc2_plan::Enc &L = h->enc[l];
        if (!L.bound) return fail(TDMPC2_ERR_STATE, "encoder layer %d of %d is not bound", l, h->enc_layers);
        const int exp_in = l == 0 ? obs_dim + c.task_dim : h->enc[l - 1].out;
        if (L.in != exp_in) return fail(TDMPC2_ERR_INVALID, "encoder layer %d takes %d inputs, the data brings %d", l, L.in, exp_in);
        if (L.in > ENC_MAX_IN)  // checked for every layer before the first launch
            return fail(TDMPC2_ERR_UNSUPPORTED, "encoder layer %d: %d inputs, at most %d (a layer's input row is held in %zu bytes of LDS)",
                        l, L.in, ENC_MAX_IN, ENC_GEMV_LDS_MAX);
        p.l[l] = EncLayerDev{L.wt, L.bias, L.g, L.b, L.in, L.out};
        maxw = std::max(maxw, std::max(L.in, L.out));
    }
    if (c.task_dim > 0 && !task_emb) return fail(TDMPC2_ERR_INVALID, "multitask encoder needs task_emb");
    if (maxw > ENC_WIDE) {  // layer-at-a-time across the chip (encoder_kernels.cuh)
        if (E > c.max_envs) return fail(TDMPC2_ERR_INVALID, "encoders wider than %d take at most max_envs = %d rows per call (got %d)", ENC_WIDE, c.max_envs, E);
        if (!h->enc_y || h->enc_ws_width < maxw) return fail(TDMPC2_ERR_STATE, "encoder workspace missing (bind every layer first)");
        for (int l = 0; l < h->enc_layers; ++l) {
            const tdmpc2_plan::Enc &L = h->enc[l];
            EncGemvParams g{};
            g.wt = L.wt; g.bias = L.bias; g.in = L.in; g.out = L.out; g.y = h->enc_y;
            if (l == 0) { g.obs = obs; g.emb = task_emb; g.obs_dim = obs_dim; g.T = c.task_dim; }
            else { g.x = h->enc_x; g.ldx = h->enc[l - 1].out; }
            hipLaunchKernelGGL(k_enc_gemv, dim3((L.out + 63) / 64, E), dim3(256), ((size_t)L.in + 256) * 4, st, g);
            EncNormParams n{};
            const bool last = l == h->enc_layers - 1;
            n.y = h->enc_y; n.g = L.g; n.b = L.b; n.out = last ? z : h->enc_x; n.width = L.out; n.last = last; n.simnorm_dim = c.simnorm_dim;
            hipLaunchKernelGGL(k_enc_norm, dim3(E), dim3(ENC_THREADS), 0, st, n);
        }
        HIP_TRY(hipGetLastError());
        return 0;
    }
    p.nl = h->enc_layers; p.obs_dim = obs_dim; p.T = c.task_dim; p.maxw = maxw; p.simnorm_dim = c.simnorm_dim;
    p.obs = obs; p.task_emb = task_emb; p.z = z;
    const size_t lds = ((size_t)2 * maxw + ENC_THREADS / 64) * 4;
    hipLaunchKernelGGL(k_encode, dim3(E), dim3(ENC_THREADS), lds, st, p);
    HIP_TRY(hipGetLastError());
    return 0;
}
}  // namespace

int tdmpc2_plan_encode(tdmpc2_plan_t *h, int n_envs, const float *obs, int obs_dim, const float *task_emb, float *z_out,
                       void *stream) {
    if (!h || !obs || !z_out) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n_envs < 1) return fail(TDMPC2_ERR_INVALID, "n_envs %d < 1", n_envs);
    ENTER_ON(h, stream);
    return launch_encode(h, n_envs, obs, obs_dim, task_emb, z_out, (hipStream_t)stream);
}

int tdmpc2_plan_run_obs(tdmpc2_plan_t *h, int n_envs, const float *obs, int obs_dim, const float *task_emb,
                        const float *act_mask, const float *discount_pow, float *prev_mean, const uint8_t *t0, int eval_mode,
                        const tdmpc2_noise *tape, uint64_t seed, float *action, void *stream) {
    if (!h || !obs) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n_envs < 1 || n_envs > h->cfg.max_envs) return fail(TDMPC2_ERR_INVALID, "n_envs %d outside [1, %d]", n_envs, h->cfg.max_envs);
    ENTER_ON(h, stream);
    int rc = launch_encode(h, n_envs, obs, obs_dim, task_emb, h->zenc, (hipStream_t)stream);
    if (rc) return rc;
    return run_impl(h, n_envs, h->zenc, task_emb, act_mask, discount_pow, prev_mean, t0, eval_mode, tape, seed, action, nullptr,
                    stream);
}

// ================================================================ pixel-observation encoder (pixel_kernels.cuh, pixel_route.h)
int tdmpc2_plan_bind_pixel_encoder(tdmpc2_plan_t *h, int layer, const float *W, const float *b, int out_channels, int in_channels,
                                   int kernel, void *stream) {
    if (!h || !W || !b) return fail(TDMPC2_ERR_INVALID, "null argument");
    const tdmpc2_plan_cfg &c = h->cfg;
    if (c.multitask)  // the reference cannot concatenate task_emb onto an image either (world_model.py:88-112)
        return fail(TDMPC2_ERR_UNSUPPORTED, "the pixel encoder is single-task only (multitask handle)");
    if (layer < 0 || layer >= PIX_LAYERS) return fail(TDMPC2_ERR_INVALID, "pixel encoder layer %d outside [0, %d)", layer, PIX_LAYERS);
    if (kernel != pix_kernel(layer))
        return fail(TDMPC2_ERR_INVALID, "pixel encoder layer %d has a %dx%d kernel, not %dx%d", layer, pix_kernel(layer), pix_kernel(layer),
                    kernel, kernel);
    if (out_channels < PIX_MIN_C || out_channels > PIX_MAX_C || out_channels % 8)
        return fail(TDMPC2_ERR_UNSUPPORTED, "pixel encoder: %d channels (a multiple of 8 in [%d, %d])", out_channels, PIX_MIN_C, PIX_MAX_C);
    if (16 * out_channels != c.latent_dim)
        return fail(TDMPC2_ERR_INVALID, "pixel encoder: 16 x %d channels is not latent_dim %d", out_channels, c.latent_dim);
    if (c.simnorm_dim != 8) return fail(TDMPC2_ERR_UNSUPPORTED, "pixel encoder: SimNorm groups of %d (8 only)", c.simnorm_dim);
    if (layer == 0 && (in_channels < 1 || in_channels > PIX_MAX_CIN))
        return fail(TDMPC2_ERR_INVALID, "pixel encoder: %d input channels outside [1, %d]", in_channels, PIX_MAX_CIN);
    if (layer > 0 && in_channels != out_channels)
        return fail(TDMPC2_ERR_INVALID, "pixel encoder layer %d takes %d channels, not %d", layer, out_channels, in_channels);
    ENTER_ON(h, stream);
    tdmpc2_plan::Pix &P = h->pix;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (!P.tab) {  // every buffer of the encoder, once: encode / run never allocate
        static PixTap host_tab[PIX_SHIFTS * PIX_IN];
        static std::once_flag once;
        std::call_once(once, [] { pix_shift_table(host_tab); });
        for (int l = 0; l < PIX_LAYERS; ++l) {
            const int cin = l == 0 ? PIX_MAX_CIN : out_channels;
            if ((rc = dev_alloc(h, (void **)&P.wp[l], (size_t)cin * pix_kernel(l) * pix_kernel(l) * out_channels * 4))) return rc;
            if ((rc = dev_alloc(h, (void **)&P.bias[l], (size_t)out_channels * 4))) return rc;
        }
        if ((rc = dev_alloc(h, &P.tab, sizeof(host_tab)))) return rc;
        if ((rc = dev_alloc(h, (void **)&P.ws, pix_ws_bytes(c.max_envs, out_channels)))) return rc;
        if (!h->zenc && (rc = dev_alloc(h, (void **)&h->zenc, (size_t)c.max_envs * c.latent_dim * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(P.tab, host_tab, sizeof(host_tab), hipMemcpyHostToDevice, st));
        P.C = out_channels;
    }
    const int kk = kernel * kernel;
    const int n = out_channels * in_channels * kk;
    hipLaunchKernelGGL(k_pix_pack, dim3((n + 255) / 256), dim3(256), 0, st, W, P.wp[layer], out_channels, in_channels, kk);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(P.bias[layer], b, (size_t)out_channels * 4, hipMemcpyDeviceToDevice, st));
    if (layer == 0) P.cin = in_channels;
    P.bound[layer] = true;
    return TDMPC2_OK;
}

namespace {
int check_pix_call(tdmpc2_plan *h, int n_envs, int obs_dtype, int in_channels) {
    const tdmpc2_plan::Pix &P = h->pix;
    if (n_envs < 1 || n_envs > h->cfg.max_envs) return fail(TDMPC2_ERR_INVALID, "n_envs %d outside [1, %d]", n_envs, h->cfg.max_envs);
    if (obs_dtype != 0 && obs_dtype != 1) return fail(TDMPC2_ERR_INVALID, "obs_dtype %d (0 = uint8, 1 = float32)", obs_dtype);
    for (int l = 0; l < PIX_LAYERS; ++l)
        if (!P.bound[l]) return fail(TDMPC2_ERR_STATE, "no pixel encoder bound (layer %d; tdmpc2_plan_bind_pixel_encoder)", l);
    if (in_channels < 1 || in_channels > PIX_MAX_CIN)
        return fail(TDMPC2_ERR_INVALID, "pixel encoder: %d input channels outside [1, %d]", in_channels, PIX_MAX_CIN);
    if (in_channels != P.cin)
        return fail(TDMPC2_ERR_INVALID, "pixel encoder: the observation has %d channels, layer 0 was bound with %d", in_channels, P.cin);
    return 0;
}

int launch_encode_pix(tdmpc2_plan *h, int E, const void *obs, int obs_dtype, const int32_t *shift, float *z, hipStream_t st) {
    const tdmpc2_plan::Pix &P = h->pix;
    PixParams p{};
    for (int l = 0; l < PIX_LAYERS; ++l) { p.wp[l] = P.wp[l]; p.bias[l] = P.bias[l]; }
    p.obs = obs; p.obs_u8 = obs_dtype == 0; p.cin = P.cin; p.C = P.C;
    p.shift = shift; p.tab = static_cast<const PixTap *>(P.tab); p.ws = P.ws; p.z = z;
    const PixRoute r = pix_route(E, P.C, h->num_cus);
    if (r.kind == PIX_PER_IMAGE) {
        hipLaunchKernelGGL(k_pix_image, dim3(r.g[0].x), dim3(r.g[0].threads), r.g[0].lds, st, p);
    } else {
        hipLaunchKernelGGL(k_pix_spread<0>, dim3(r.g[0].x, r.g[0].y, r.g[0].z), dim3(r.g[0].threads), 0, st, p);
        hipLaunchKernelGGL(k_pix_spread<1>, dim3(r.g[1].x, r.g[1].y, r.g[1].z), dim3(r.g[1].threads), 0, st, p);
        hipLaunchKernelGGL(k_pix_spread<2>, dim3(r.g[2].x, r.g[2].y, r.g[2].z), dim3(r.g[2].threads), 0, st, p);
        hipLaunchKernelGGL(k_pix_spread<3>, dim3(r.g[3].x, r.g[3].y, r.g[3].z), dim3(r.g[3].threads), 0, st, p);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
}  // namespace

int tdmpc2_plan_encode_pix(tdmpc2_plan_t *h, int n_envs, const void *obs, int obs_dtype, int in_channels, const int32_t *shift,
                           float *z_out, void *stream) {
    if (!h || !obs || !shift || !z_out) return fail(TDMPC2_ERR_INVALID, "null argument");
    int rc = check_pix_call(h, n_envs, obs_dtype, in_channels);
    if (rc) return rc;
    ENTER_ON(h, stream);
    return launch_encode_pix(h, n_envs, obs, obs_dtype, shift, z_out, (hipStream_t)stream);
}

int tdmpc2_plan_run_pix(tdmpc2_plan_t *h, int n_envs, const void *obs, int obs_dtype, int in_channels, const int32_t *shift,
                        const float *disc_pow, float *prev_mean, const uint8_t *t0, int eval_mode, const tdmpc2_noise *tape, uint64_t seed,
                        float *action, void *stream) {
    if (!h || !obs || !shift || !disc_pow || !prev_mean || !t0 || !action) return fail(TDMPC2_ERR_INVALID, "null argument");
    int rc = check_pix_call(h, n_envs, obs_dtype, in_channels);
    if (rc) return rc;
    ENTER_ON(h, stream);
    if ((rc = launch_encode_pix(h, n_envs, obs, obs_dtype, shift, h->zenc, (hipStream_t)stream))) return rc;
    return run_impl(h, n_envs, h->zenc, nullptr, nullptr, disc_pow, prev_mean, t0, eval_mode, tape, seed, action, nullptr, stream);
}

// ================================================================ policy prior (k_policy.hip: policy_kernels.cuh, policy_route.h)
int tdmpc2_plan_bind_policy(tdmpc2_plan_t *h, int layer, const float *W, const float *b, const float *ln_g, const float *ln_b,
                            int out_features, int in_features, void *stream) {
    if (!h || !W || !b) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (layer < 0 || layer > 2) return fail(TDMPC2_ERR_INVALID, "policy layer %d outside [0, 2]", layer);
    const tdmpc2_plan_cfg &c = h->cfg;
    const int in0 = c.latent_dim + c.task_dim, M = c.mlp_dim, A = c.action_dim;
    const int want_in = layer == 0 ? in0 : M, want_out = layer == 2 ? 2 * A : M;
    if (in_features != want_in || out_features != want_out)
        return fail(TDMPC2_ERR_INVALID, "policy layer %d: got [%d, %d], expected [%d, %d] (latent_dim + task_dim -> mlp_dim -> 2 action_dim)",
                    layer, out_features, in_features, want_out, want_in);
    if (layer < 2 && (!ln_g || !ln_b)) return fail(TDMPC2_ERR_INVALID, "policy layer %d needs its LayerNorm parameters", layer);
    if (M > POL_MAX_WIDTH || in0 > POL_MAX_WIDTH)
        return fail(TDMPC2_ERR_UNSUPPORTED, "policy prior: widths %d / %d beyond %d", in0, M, POL_MAX_WIDTH);
    ENTER_ON(h, stream);
    tdmpc2_plan::Pol &P = h->pol;
    int rc;
    if (!P.x) {  // every buffer of the policy prior, once: pi / act_pi never allocate
        for (int l = 0; l < 3; ++l) {
            const int li = l == 0 ? in0 : M, lo = l == 2 ? 2 * A : M;
            if ((rc = dev_alloc(h, (void **)&P.wt[l], (size_t)li * lo * 4))) return rc;
            if ((rc = dev_alloc(h, (void **)&P.bias[l], (size_t)lo * 4))) return rc;
            if (l < 2 && (rc = dev_alloc(h, (void **)&P.g[l], (size_t)lo * 4))) return rc;
            if (l < 2 && (rc = dev_alloc(h, (void **)&P.b[l], (size_t)lo * 4))) return rc;
        }
        if ((rc = dev_alloc(h, (void **)&P.y, pol_ws_y_floats(c.max_envs, M, A) * 4))) return rc;
        if (!h->zenc && (rc = dev_alloc(h, (void **)&h->zenc, (size_t)c.max_envs * c.latent_dim * 4))) return rc;
        if ((rc = tdk::pol_set_lds())) return rc;
        if ((rc = dev_alloc(h, (void **)&P.x, pol_ws_x_floats(c.max_envs, M) * 4))) return rc;  // last: marks the set complete
    }
    RfJobs j(h);
    add_pol_layer(h, j, layer, tdmpc2_weight_entry{W, b, ln_g, ln_b});
    return run_jobs(h, j, (hipStream_t)stream);
}

// ================================================================ weight tables: the packer's jobs, collected from a table
// Every net the table names (all three layers of it), the state encoder, and the policy prior's fp32 copy when its buffers
// exist and TDMPC2_NET_PI is named.
int tdmpc2_plan_refresh_weights(tdmpc2_plan_t *h, const tdmpc2_weight_table *tab, void *stream) {
    if (!h || !tab) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    RfJobs j(h);
    for (int net = TDMPC2_NET_DYNAMICS; net <= TDMPC2_NET_TARGET_Q; ++net) {
        int named = 0;
        for (const tdmpc2_weight_entry &e : tab->net[net]) named += (e.W != nullptr) + (e.b != nullptr) + (e.ln_g != nullptr) + (e.ln_b != nullptr);
        if (!named) continue;  // left as it is
        for (int l = 0; l < 3; ++l)
            if (int rc = add_net_layer(h, j, net, l, tab->net[net][l])) return rc;
    }
    if (tab->enc_layers < 0) return fail(TDMPC2_ERR_INVALID, "encoder depth %d outside [0, %d]", tab->enc_layers, ENC_MAX_LAYERS);
    for (int l = 0; l < tab->enc_layers; ++l)
        if (int rc = add_enc_layer(h, j, l, tab->enc_layers, tab->enc[l], tab->enc_out[l], tab->enc_in[l])) return rc;
    if (h->pol.x && (j.nets >> TDMPC2_NET_PI & 1))
        for (int l = 0; l < 3; ++l) add_pol_layer(h, j, l, tab->net[TDMPC2_NET_PI][l]);
    return run_jobs(h, j, (hipStream_t)stream);
}

// The jobs of TDMPC2_NET_TARGET_Q with the caller's target tensors as sources; RO_SCAN lerps them towards the online ensemble
// `online` names before it scans them.
int tdmpc2_plan_soft_update_target(tdmpc2_plan_t *h, const tdmpc2_weight_table *online, float *const target[3][4], float tau,
                                   void *stream) {
    if (!h || !online || !target) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (!(tau >= 0.f && tau <= 1.f)) return fail(TDMPC2_ERR_INVALID, "soft update: tau %g outside [0, 1]", (double)tau);
    ENTER_ON(h, stream);
    RfJobs j(h);
    for (int l = 0; l < 3; ++l) {
        const tdmpc2_weight_entry src{target[l][0], target[l][1], target[l][2], target[l][3]};
        const tdmpc2_weight_entry &on = online->net[TDMPC2_NET_Q][l];
        const bool ln = layer_shape(h, TDMPC2_NET_TARGET_Q, l).has_ln;
        if (!on.W || !on.b || (ln && (!on.ln_g || !on.ln_b)))
            return fail(TDMPC2_ERR_INVALID, "soft update: the table lacks the online Q ensemble (layer %d)", l);
        if (!src.W || !src.b || (ln && (!src.ln_g || !src.ln_b)))
            return fail(TDMPC2_ERR_INVALID, "soft update: null target tensor (layer %d)", l);
        if (int rc = add_net_layer(h, j, TDMPC2_NET_TARGET_Q, l, src)) return rc;
        j.p.online[l][0] = on.W; j.p.online[l][1] = on.b; j.p.online[l][2] = ln ? on.ln_g : nullptr; j.p.online[l][3] = ln ? on.ln_b : nullptr;
    }
    j.p.lerp_net = TDMPC2_NET_TARGET_Q;
    j.p.tau = tau;
    return run_jobs(h, j, (hipStream_t)stream);
}

namespace {
int check_pol_call(tdmpc2_plan *h, const float *task_emb, const float *act_mask, const tdmpc2_policy_out *out) {
    if (!out || !out->action) return fail(TDMPC2_ERR_INVALID, "null policy output (out / out->action)");
    for (int l = 0; l < 3; ++l)
        if (!h->pol.bound[l]) return fail(TDMPC2_ERR_STATE, "policy layer %d is not bound (tdmpc2_plan_bind_policy)", l);
    if (h->cfg.multitask && (!task_emb || !act_mask)) return fail(TDMPC2_ERR_INVALID, "a multitask policy prior needs task_emb and act_mask");
    return 0;
}

// the state encoder as row-route layers (acting), with launch_encode's checks; maxw = its widest layer
int pol_enc_chain(tdmpc2_plan *h, int obs_dim, PolRowParams &p, int &maxw) {
    if (!h->enc_layers) return fail(TDMPC2_ERR_STATE, "no encoder bound (tdmpc2_plan_bind_encoder)");
    maxw = 0;
    for (int l = 0; l < h->enc_layers; ++l) {
        const tdmpc2_plan::Enc &L = h->enc[l];
        if (!L.bound) return fail(TDMPC2_ERR_STATE, "encoder layer %d of %d is not bound", l, h->enc_layers);
        const int exp_in = l == 0 ? obs_dim + h->cfg.task_dim : h->enc[l - 1].out;
        if (L.in != exp_in) return fail(TDMPC2_ERR_INVALID, "encoder layer %d takes %d inputs, the data brings %d", l, L.in, exp_in);
        p.enc[l] = PolLayerDev{L.wt, L.bias, L.g, L.b, L.in, L.out};
        maxw = std::max(maxw, std::max(L.in, L.out));
    }
    p.enc_nl = h->enc_layers;
    p.obs_dim = obs_dim;
    return 0;
}

// WorldModel.pi of n rows.  obs != null: the rows are observations and the encoder runs first -- inside the row-route launch when
// it is narrow enough for k_encode's own one-launch route, else through launch_encode into h->zenc.
int launch_pi(tdmpc2_plan *h, int n, const float *z, const float *obs, int obs_dim, const float *emb, const float *mask,
              const float *eps, uint64_t seed, int eval_mode, const tdmpc2_policy_out *out, hipStream_t st) {
    const tdmpc2_plan_cfg &c = h->cfg;
    const tdmpc2_plan::Pol &P = h->pol;
    const int L = c.latent_dim, T = c.task_dim, M = c.mlp_dim, A = c.action_dim, in0 = L + T;
    PolRowParams rp{};
    int maxw = std::max(in0, std::max(M, 2 * A)), rc;
    if (obs) {
        int enc_w = 0;
        if ((rc = pol_enc_chain(h, obs_dim, rp, enc_w))) return rc;
        const PolRoute r = pol_route(n, in0, M, A, std::max(maxw, enc_w), P.mode);
        if (enc_w <= ENC_WIDE && r.kind == POL_ROW) {
            maxw = std::max(maxw, enc_w);
            rp.obs = obs;
        } else {  // the encoder's own route, unchanged, then the policy from its latents
            if ((rc = launch_encode(h, n, obs, obs_dim, emb, h->zenc, st))) return rc;
            rp.enc_nl = 0;
            z = h->zenc;
        }
    }
    PolHeadArgs hd{};
    hd.A = A; hd.eval_mode = eval_mode; hd.lmin = c.log_std_min; hd.ldif = c.log_std_dif;
    hd.seed = seed; hd.call = h->call++;  // exactly one per call
    auto at = [](float *p, size_t off) { return p ? p + off : nullptr; };
    auto cat = [](const float *p, size_t off) { return p ? p + off : nullptr; };
    const PolRoute r = pol_route(n, in0, M, A, maxw, P.mode);
    if (r.kind == POL_ROW) {
        rp.z = z; rp.task_emb = emb;
        rp.L = L; rp.T = T; rp.maxw = maxw; rp.simnorm_dim = c.simnorm_dim;
        for (int l = 0; l < 3; ++l) rp.pi[l] = PolLayerDev{P.wt[l], P.bias[l], l < 2 ? P.g[l] : nullptr, l < 2 ? P.b[l] : nullptr,
                                                            l == 0 ? in0 : M, l == 2 ? 2 * A : M};
        hd.row0 = 0; hd.mask = mask; hd.eps = eps;
        hd.action = out->action; hd.mean = out->mean; hd.log_std = out->log_std; hd.entropy = out->entropy;
        hd.scaled_entropy = out->scaled_entropy; hd.eps_out = out->eps_out;
        rp.head = hd;
        return tdk::pol_launch_row(rp, r.g[0], st);
    }
    for (int r0 = 0; r0 < n; r0 += c.max_envs) {  // the spread route: chunks of at most max_envs rows (the workspace)
        const int m = std::min(c.max_envs, n - r0);
        const PolRoute rc_ = pol_route(m, in0, M, A, maxw, POL_FORCE_SPREAD);
        const size_t ra = (size_t)r0 * A;
        for (int l = 0; l < 3; ++l) {
            PolGemvParams g{};
            g.wt = P.wt[l]; g.bias = P.bias[l]; g.in = l == 0 ? in0 : M; g.out = l == 2 ? 2 * A : M; g.n = m; g.y = P.y;
            if (l == 0) { g.z = z + (size_t)r0 * L; g.emb = cat(emb, (size_t)r0 * T); g.L = L; g.T = T; }
            else { g.x = P.x; g.ldx = M; }
            if ((rc = tdk::pol_launch_gemv(g, rc_.g[2 * l], st))) return rc;
            if (l == 2) break;
            EncNormParams nm{};
            nm.y = P.y; nm.g = P.g[l]; nm.b = P.b[l]; nm.out = P.x; nm.width = M; nm.last = 0; nm.simnorm_dim = c.simnorm_dim;
            const PolGrid &ng = rc_.g[2 * l + 1];
            hipLaunchKernelGGL(k_enc_norm, dim3(ng.x), dim3(ng.threads), 0, st, nm);
            HIP_TRY(hipGetLastError());
        }
        PolHeadParams hp{};
        hp.y = P.y;
        hp.head = hd;
        hp.head.row0 = r0; hp.head.mask = cat(mask, ra); hp.head.eps = cat(eps, ra);
        hp.head.action = at(out->action, ra); hp.head.mean = at(out->mean, ra); hp.head.log_std = at(out->log_std, ra);
        hp.head.entropy = at(out->entropy, r0); hp.head.scaled_entropy = at(out->scaled_entropy, r0); hp.head.eps_out = at(out->eps_out, ra);
        if ((rc = tdk::pol_launch_head(hp, rc_.g[5], st))) return rc;
    }
    return 0;
}
}  // namespace

int tdmpc2_plan_pi(tdmpc2_plan_t *h, int n_rows, const float *z, const float *task_emb, const float *act_mask, const float *eps,
                   uint64_t seed, const tdmpc2_policy_out *out, void *stream) {
    if (!h || !z) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n_rows < 1) return fail(TDMPC2_ERR_INVALID, "n_rows %d < 1", n_rows);
    int rc = check_pol_call(h, task_emb, act_mask, out);
    if (rc) return rc;
    ENTER_ON(h, stream);
    return launch_pi(h, n_rows, z, nullptr, 0, task_emb, act_mask, eps, seed, 0, out, (hipStream_t)stream);
}

int tdmpc2_plan_act_pi(tdmpc2_plan_t *h, int n_envs, const float *obs, int obs_dim, const float *task_emb, const float *act_mask,
                       const float *eps, int eval_mode, uint64_t seed, const tdmpc2_policy_out *out, void *stream) {
    if (!h || !obs) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n_envs < 1 || n_envs > h->cfg.max_envs) return fail(TDMPC2_ERR_INVALID, "n_envs %d outside [1, %d]", n_envs, h->cfg.max_envs);
    int rc = check_pol_call(h, task_emb, act_mask, out);
    if (rc) return rc;
    ENTER_ON(h, stream);
    return launch_pi(h, n_envs, nullptr, obs, obs_dim, task_emb, act_mask, eps, seed, eval_mode, out, (hipStream_t)stream);
}

int tdmpc2_plan_act_pi_pix(tdmpc2_plan_t *h, int n_envs, const void *obs, int obs_dtype, int in_channels, const int32_t *shift,
                           const float *eps, int eval_mode, uint64_t seed, const tdmpc2_policy_out *out, void *stream) {
    if (!h || !obs || !shift) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (h->cfg.multitask) return fail(TDMPC2_ERR_UNSUPPORTED, "the pixel encoder is single-task only (multitask handle)");
    int rc = check_pix_call(h, n_envs, obs_dtype, in_channels);
    if (rc) return rc;
    if ((rc = check_pol_call(h, nullptr, nullptr, out))) return rc;
    ENTER_ON(h, stream);
    if ((rc = launch_encode_pix(h, n_envs, obs, obs_dtype, shift, h->zenc, (hipStream_t)stream))) return rc;
    return launch_pi(h, n_envs, h->zenc, nullptr, 0, nullptr, nullptr, eps, seed, eval_mode, out, (hipStream_t)stream);
}

namespace {
// per-task tables of a multitask value call: effective first-layer biases of pi and of the chosen Q ensemble, action
// masks, discounts; (re)built on every call (the weights may have been re-bound), storage grown on demand
int build_task_tables(tdmpc2_plan *h, const tdmpc2_task_tables *tk, bool target, size_t rows_p, hipStream_t st, bool all_nets = false) {
    const tdmpc2_plan_cfg &c = h->cfg;
    const int nt = tk->n_tasks;
    const size_t width = h->lay.on ? (size_t)h->lay.Mp : (size_t)WIDTH;
    int rc;
    if (nt > h->tab_tasks) {  // grow: the old tables are released (stream-ordered: earlier calls on `st` are done with them)
        HIP_TRY(hipStreamSynchronize(st));
        dev_release(h, h->beff_tab); dev_release(h, h->mask_tab); dev_release(h, h->disc_tab);
        h->beff_tab = h->mask_tab = h->disc_tab = nullptr;
        h->tab_tasks = 0;
        if ((rc = dev_alloc(h, (void **)&h->beff_tab, (size_t)nt * h->nnets * width * 4))) return rc;
        if ((rc = dev_alloc(h, (void **)&h->mask_tab, (size_t)nt * c.action_dim * 4))) return rc;
        if ((rc = dev_alloc(h, (void **)&h->disc_tab, (size_t)nt * 4))) return rc;
        h->tab_tasks = nt;
    }
    if (rows_p > h->task_rows_cap) {
        HIP_TRY(hipStreamSynchronize(st));
        dev_release(h, h->task_rows);
        h->task_rows = nullptr;
        h->task_rows_cap = 0;
        if ((rc = dev_alloc(h, (void **)&h->task_rows, rows_p * 4))) return rc;
        h->task_rows_cap = rows_p;
    }
    HIP_TRY(hipMemcpyAsync(h->mask_tab, tk->act_mask, (size_t)nt * c.action_dim * 4, hipMemcpyDeviceToDevice, st));
    if (tk->discount) HIP_TRY(hipMemcpyAsync(h->disc_tab, tk->discount, (size_t)nt * 4, hipMemcpyDeviceToDevice, st));
    const HostNet *qarr = target ? h->tq : h->q;
    if (h->lay.on) return lay_setup(h, st, nt, tk->task_emb, nullptr, nullptr, false, h->beff_tab, qarr);
    TaskBiasParams p{};
    p.T = c.task_dim; p.nq = c.num_q; p.nnets = h->nnets; p.task_emb = tk->task_emb; p.beff_tab = h->beff_tab;
    p.wemb[BE_PI] = h->pi.l[0].wemb; p.bias[BE_PI] = h->pi.l[0].bias;
    if (all_nets) {  // model rollout: the dynamics and reward first layers take the row's task as well
        p.wemb[BE_DYN] = h->dyn.l[0].wemb; p.bias[BE_DYN] = h->dyn.l[0].bias;
        p.wemb[BE_REW] = h->rew.l[0].wemb; p.bias[BE_REW] = h->rew.l[0].bias;
    }
    for (int i = 0; i < c.num_q; ++i) { p.wemb[BE_Q0 + i] = qarr[i].l[0].wemb; p.bias[BE_Q0 + i] = qarr[i].l[0].bias; }
    hipLaunchKernelGGL(ks_task_bias, dim3(nt), dim3(WIDTH), 0, st, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_value(tdmpc2_plan *h, int rows, const float *z, bool target, bool reduce_min, const float *pi_eps, const int32_t *qidx,
                 uint64_t seed, const float *reward, const float *terminated, float discount, const tdmpc2_task_tables *tk,
                 float *action, float *out, hipStream_t st) {
    const tdmpc2_plan_cfg &c = h->cfg;
    unsigned call;
    int rc = begin_value_call(h, "policy_value / td_target need", tk, target, st, &call, [&] {
        return c.multitask && reward && !tk->discount ? fail(TDMPC2_ERR_INVALID, "multitask td_target needs the per-task discounts") : 0;
    });
    if (rc) return rc;
    if (h->lay.on) {
        const size_t rows_p = round_up((size_t)rows, GBM), cap = round_up((size_t)c.max_envs * c.num_samples, GBM);
        if (rows_p > cap)
            return fail(TDMPC2_ERR_INVALID, "the layered workspace holds %zu rows (max_envs x num_samples); got %d", cap, rows);
        if (c.multitask) {
            if ((rc = build_task_tables(h, tk, target, rows_p, st))) return rc;
            HIP_TRY(hipMemsetAsync(h->task_rows, 0, rows_p * 4, st));
            HIP_TRY(hipMemcpyAsync(h->task_rows, tk->task_ids, (size_t)rows * 4, hipMemcpyDeviceToDevice, st));
        }
        // the two heads: given, or randperm(num_q)[:2] once per call (world_model.py:212)
        if ((rc = lay_set_qidx(h, st, 1, qidx, 2L, c.num_q, 0, seed, call, h->lay.qidx))) return rc;
        return lay_value(h, st, rows, z, target, reduce_min, pi_eps, h->lay.qidx, seed, call, reward, terminated, discount,
                         c.multitask ? h->task_rows : nullptr, action, out);
    }
    if (c.multitask && (rc = build_task_tables(h, tk, target, 0, st))) return rc;
    ValueParams p{};
    p.rows = rows; p.A = c.action_dim; p.Apad = h->Apad; p.nq = c.num_q; p.num_bins = c.num_bins; p.reduce_min = reduce_min ? 1 : 0;
    p.log_std_min = c.log_std_min; p.log_std_dif = c.log_std_dif; p.discount = discount;
    p.pi = to_dev(h->pi);
    for (int i = 0; i < c.num_q; ++i) p.q[i] = to_dev(target ? h->tq[i] : h->q[i]);
    p.bins = h->bins; p.z = z; p.pi_eps = pi_eps; p.qidx = qidx; p.seed = seed; p.call = call;
    p.reward = reward; p.terminated = terminated; p.action = action; p.out = out;
    p.nnets = h->nnets;
    if (c.multitask) {
        p.task_ids = tk->task_ids; p.beff_tab = h->beff_tab; p.mask_tab = h->mask_tab;
        p.disc_tab = reward ? h->disc_tab : nullptr;
    }
    const int grid = (rows + ROWS - 1) / ROWS;
    const size_t lds = h->lds_bytes;
    const int ar = h->split ? 0 : 1;
    fused_ops(h->Apad).value(ar, p, grid, lds, st);
    HIP_TRY(hipGetLastError());
    return 0;
}
}  // namespace

int tdmpc2_plan_policy_value_mt(tdmpc2_plan_t *h, int n_rows, const float *z, const tdmpc2_task_tables *tasks, int use_target,
                                int reduce_min, const float *pi_eps, const int32_t *qidx, uint64_t seed, float *action, float *q,
                                void *stream) {
    if (!h || !z || !q) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n_rows < 1) return fail(TDMPC2_ERR_INVALID, "n_rows %d < 1", n_rows);
    ENTER_ON(h, stream);
    return launch_value(h, n_rows, z, use_target != 0, reduce_min != 0, pi_eps, qidx, seed, nullptr, nullptr, 0.f, tasks, action, q,
                        (hipStream_t)stream);
}

int tdmpc2_plan_policy_value(tdmpc2_plan_t *h, int n_rows, const float *z, int use_target, int reduce_min, const float *pi_eps,
                             const int32_t *qidx, uint64_t seed, float *action, float *q, void *stream) {
    return tdmpc2_plan_policy_value_mt(h, n_rows, z, nullptr, use_target, reduce_min, pi_eps, qidx, seed, action, q, stream);
}

int tdmpc2_plan_td_target_mt(tdmpc2_plan_t *h, int n_rows, const float *next_z, const float *reward, const float *terminated,
                             float discount, const tdmpc2_task_tables *tasks, const float *pi_eps, const int32_t *qidx,
                             uint64_t seed, float *td, void *stream) {
    if (!h || !next_z || !reward || !terminated || !td) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n_rows < 1) return fail(TDMPC2_ERR_INVALID, "n_rows %d < 1", n_rows);
    ENTER_ON(h, stream);
    return launch_value(h, n_rows, next_z, true, true, pi_eps, qidx, seed, reward, terminated, discount, tasks, nullptr, td,
                        (hipStream_t)stream);
}

int tdmpc2_plan_td_target(tdmpc2_plan_t *h, int n_rows, const float *next_z, const float *reward, const float *terminated,
                          float discount, const float *pi_eps, const int32_t *qidx, uint64_t seed, float *td, void *stream) {
    return tdmpc2_plan_td_target_mt(h, n_rows, next_z, reward, terminated, discount, nullptr, pi_eps, qidx, seed, td, stream);
}

// ---------------------------------------------------------------- model rollout + losses: the forward half of TDMPC2._update
// (tdmpc2/tdmpc2.py:259-304).  model_route.h decides the stages; the fused family launches ks_value_roll / ks_value_chain
// (k_model.hip), the layered family its GEMM chains (lay_model); the loss rows and the fixed-order tail are shared.
namespace {
int grow_ws(tdmpc2_plan *h, float **buf, size_t *cap, size_t floats, hipStream_t st) {
    if (floats <= *cap) return 0;
    HIP_TRY(hipStreamSynchronize(st));  // (first use or a larger call: outside a hipGraph capture, like the task tables)
    dev_release(h, *buf);
    *buf = nullptr;
    *cap = 0;
    int rc = dev_alloc(h, (void **)buf, floats * 4);
    if (rc) return rc;
    *cap = floats;
    return 0;
}

int launch_model(tdmpc2_plan *h, int B, int H, const float *z0, const float *actions, bool target, const tdmpc2_task_tables *tk,
                 const tdmpc2_model_targets *tg, const tdmpc2_model_out *out, float *losses, float *step_means, hipStream_t st) {
    const tdmpc2_plan_cfg &c = h->cfg;
    static const tdmpc2_model_out none{};
    if (!out) out = &none;
    unsigned want = 0;
    if (out->zs) want |= MW_ZS;
    if (out->reward_logits) want |= MW_REW_LOGITS;
    if (out->reward) want |= MW_REW;
    if (out->q_logits) want |= MW_Q_LOGITS;
    if (out->q) want |= MW_Q;
    if (out->term_logit) want |= MW_TERM;
    if (tg) want |= MW_LOSSES;
    if (tg && c.num_bins < 2) return fail(TDMPC2_ERR_UNSUPPORTED, "model_losses needs two-hot heads (num_bins %d: the reference's soft_ce is identically 0)", c.num_bins);
    if (tg && tg->terminated && !c.episodic) return fail(TDMPC2_ERR_INVALID, "`terminated` given to a non-episodic handle");
    const size_t cap = round_up((size_t)c.max_envs * c.num_samples, GBM);
    const ModelRoute r = model_route(ModelIn{h->lay.on ? MODEL_LAYERED : MODEL_FUSED, B, H, c.num_q, c.num_bins, c.episodic, want, (long)cap,
                                                 (h->split && h->lay.fuse_ln) ? 0 : 1});
    switch (r.refuse) {
        case MR_OK: break;
        case MR_BAD_H: return fail(TDMPC2_ERR_INVALID, "steps %d outside [0, %d]", H, MAXH);
        case MR_BAD_B: return fail(TDMPC2_ERR_INVALID, "batch %d < 1", B);
        case MR_LOSSES_H0: return fail(TDMPC2_ERR_INVALID, "model_losses needs at least one step");
        case MR_NOT_EPISODIC: return fail(TDMPC2_ERR_INVALID, "term_logit asked of a non-episodic handle");
        case MR_ROWS: return fail(TDMPC2_ERR_INVALID, "the layered workspace holds %zu rows (max_envs x num_samples); got batch x steps = %d x %d", cap, B, H);
        default: return fail(TDMPC2_ERR_UNSUPPORTED, "model_losses needs two-hot heads (num_bins %d)", c.num_bins);
    }
    if (H > 0 && !actions) return fail(TDMPC2_ERR_INVALID, "null actions");
    if (tg) {
        if (!tg->next_z || !tg->reward || !tg->td_target || !losses) return fail(TDMPC2_ERR_INVALID, "null target / losses argument");
        if (c.episodic && !tg->terminated) return fail(TDMPC2_ERR_INVALID, "episodic handle: `terminated` is required");
    }
    unsigned call;
    int rc = begin_value_call(h, "model_rollout / model_losses need", tk, target, st, &call, [] { return 0; });
    if (rc) return rc;
    const size_t Ld = (size_t)c.latent_dim, HB = (size_t)H * B;
    if (r.launches == 0) {  // H = 0 and no termination logit: zs[0] = z0 is all there is
        if (out->zs && out->zs != z0) HIP_TRY(hipMemcpyAsync(out->zs, z0, (size_t)B * Ld * 4, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    float *zs = out->zs;
    if (!zs) {
        if ((rc = grow_ws(h, &h->model_zs, &h->model_zs_cap, (size_t)(H + 1) * B * Ld, st))) return rc;
        zs = h->model_zs;
    }
    if (tg && (rc = grow_ws(h, &h->model_rowloss, &h->model_rowloss_cap, (size_t)model_rowloss_floats(B, H, c.num_q), st))) return rc;
    const size_t trows = (size_t)(H + 1) * B, trows_p = round_up(trows, GBM);
    if (c.multitask) {
        if ((rc = build_task_tables(h, tk, target, h->lay.on ? trows_p : 0, st, true))) return rc;
        if (h->lay.on && (rc = model_launch_tile_tasks(tk->task_ids, B, (int)trows, (int)trows_p, h->task_rows, st))) return rc;
    }
    if (zs != z0) HIP_TRY(hipMemcpyAsync(zs, z0, (size_t)B * Ld * 4, hipMemcpyDeviceToDevice, st));
    ModelLossArgs ls{};
    ls.num_bins = c.num_bins; ls.vmin = c.vmin; ls.vmax = c.vmax;
    ls.bin_size = c.num_bins > 1 ? (float)(((double)c.vmax - (double)c.vmin) / (c.num_bins - 1)) : 1.f;  // parser.py: cfg.bin_size
    ls.bins = h->bins; ls.HB = (long)HB;
    if (tg) { ls.t_reward = tg->reward; ls.t_td = tg->td_target; ls.t_term = tg->terminated; ls.rowloss = h->model_rowloss; }
    const ModelOutArgs oa{out->reward_logits, out->reward, out->q_logits, out->q, out->term_logit};
    if (h->lay.on) {
        if ((rc = lay_model(h, st, r, B, H, actions, zs, target, c.multitask ? h->task_rows : nullptr, oa, ls))) return rc;
    } else {
        ModelParams p{};
        p.B = B; p.H = H; p.A = c.action_dim; p.Apad = h->Apad; p.nq = c.num_q; p.nnets = h->nnets; p.steps = r.st[MS_DYN].steps;
        p.dyn = to_dev(h->dyn); p.rew = to_dev(h->rew);
        if (c.episodic) p.term = to_dev(h->term);
        for (int i = 0; i < c.num_q; ++i) p.q[i] = to_dev(target ? h->tq[i] : h->q[i]);
        p.z0 = z0; p.actions = actions; p.zs = zs; p.out = oa; p.ls = ls;
        if (c.multitask) { p.task_ids = tk->task_ids; p.beff_tab = h->beff_tab; }
        const int ar = h->split ? 0 : 1;
        const ModelOps &ops = model_ops(h->Apad);
        if (r.st[MS_DYN].run) {
            ops.dyn(ar, p, r.st[MS_DYN].gx, h->lds_bytes, st);
            HIP_TRY(hipGetLastError());
        }
        if (r.st[MS_HEADS].run) {
            for (int k = 0; k < r.nchain; ++k) p.chain[k] = r.chain[k];
            ops.chain(ar, p, r.st[MS_HEADS].gx, r.st[MS_HEADS].gy, r.st[MS_HEADS].gz, h->lds_bytes, st);
            HIP_TRY(hipGetLastError());
        }
        if (r.st[MS_TERM].run) {
            p.chain[0] = MC_TERM;
            ops.chain(ar, p, r.st[MS_TERM].gx, r.st[MS_TERM].gy, 1, h->lds_bytes, st);
            HIP_TRY(hipGetLastError());
        }
    }
    if (!tg) return 0;
    const unsigned int *err = (h->lay.on && h->split && h->lay.fuse_ln) ? h->cl_err_dev : nullptr;
    ModelConsParams cp{zs + (size_t)B * Ld, tg->next_z, (int)HB, c.latent_dim, h->model_rowloss};
    if ((rc = model_launch_cons(cp, r.st[MS_CONS].gx, st))) return rc;
    ModelTailParams tp{};
    tp.rowloss = h->model_rowloss; tp.B = B; tp.H = H; tp.L = c.latent_dim; tp.nq = c.num_q; tp.episodic = c.episodic;
    for (int t = 0; t < H; ++t) tp.rho_pow[t] = (float)std::pow((double)tg->rho, t);
    tp.coef[0] = tg->consistency_coef; tp.coef[1] = tg->reward_coef; tp.coef[2] = tg->value_coef; tp.coef[3] = tg->termination_coef;
    tp.losses = losses; tp.step_means = step_means; tp.err = err;
    return model_launch_tail(tp, st);
}
}  // namespace

int tdmpc2_plan_model_rollout_mt(tdmpc2_plan_t *h, int batch, int steps, const float *z0, const float *actions,
                                 const tdmpc2_task_tables *tasks, int use_target, const tdmpc2_model_out *out, void *stream) {
    if (!h || !z0 || !out) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    return launch_model(h, batch, steps, z0, actions, use_target != 0, tasks, nullptr, out, nullptr, nullptr, (hipStream_t)stream);
}
int tdmpc2_plan_model_rollout(tdmpc2_plan_t *h, int batch, int steps, const float *z0, const float *actions, int use_target,
                              const tdmpc2_model_out *out, void *stream) {
    return tdmpc2_plan_model_rollout_mt(h, batch, steps, z0, actions, nullptr, use_target, out, stream);
}
int tdmpc2_plan_model_losses_mt(tdmpc2_plan_t *h, int batch, int steps, const float *z0, const float *actions,
                                const tdmpc2_task_tables *tasks, int use_target, const tdmpc2_model_targets *targets,
                                const tdmpc2_model_out *out, float *losses, float *step_means, void *stream) {
    if (!h || !z0 || !targets || !losses) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    return launch_model(h, batch, steps, z0, actions, use_target != 0, tasks, targets, out, losses, step_means, (hipStream_t)stream);
}
int tdmpc2_plan_model_losses(tdmpc2_plan_t *h, int batch, int steps, const float *z0, const float *actions, int use_target,
                             const tdmpc2_model_targets *targets, const tdmpc2_model_out *out, float *losses, float *step_means,
                             void *stream) {
    return tdmpc2_plan_model_losses_mt(h, batch, steps, z0, actions, nullptr, use_target, targets, out, losses, step_means, stream);
}

// ---------------------------------------------------------------- policy loss: the forward of TDMPC2.update_pi (tdmpc2/tdmpc2.py:208-239)
// ks_value_ent (pi + two online Q heads + the entropy terms, per row into the handle's workspace), then one workgroup each for
// RunningScale.update on q[0] and for the fixed-order tail.
namespace {
int launch_policy_loss(tdmpc2_plan *h, int B, int steps, const float *zs, const tdmpc2_task_tables *tk, const float *pi_eps,
                       const int32_t *qidx, uint64_t seed, const tdmpc2_policy_loss_in *in, float *scale,
                       const tdmpc2_policy_loss_out *out, float *loss, hipStream_t st) {
    const tdmpc2_plan_cfg &c = h->cfg;
    static const tdmpc2_policy_loss_out none{};
    if (!out) out = &none;
    if (B < 1) return fail(TDMPC2_ERR_INVALID, "batch %d < 1", B);
    if (steps < 0 || steps > PL_MAX_STEPS) return fail(TDMPC2_ERR_INVALID, "steps %d outside [0, %d]", steps, (int)PL_MAX_STEPS);
    unsigned call;
    int rc = begin_value_call(h, "policy_loss needs", tk, false, st, &call, [&] {
        return in->update_scale && B > PL_SCALE_MAX_N
                   ? fail(TDMPC2_ERR_UNSUPPORTED, "the running scale takes at most %d values; got batch %d", (int)PL_SCALE_MAX_N, B) : 0;
    });
    if (rc) return rc;
    const int T = steps + 1;
    const size_t rows = (size_t)T * B;
    if ((rc = grow_ws(h, &h->ploss_rows, &h->ploss_rows_cap, 3 * rows, st))) return rc;
    float *wq = h->ploss_rows, *went = wq + rows, *wsent = went + rows;
    const unsigned int *err = nullptr;
    if (h->lay.on) {
        // LAYERED: pi, then the two heads, as lay_value runs them -- in pieces of the workspace's rows (max_envs x num_samples) when
        // the call has more; the two heads are drawn once, and a row's noise index is its row in the call, whatever the pieces
        const size_t cap = round_up((size_t)c.max_envs * c.num_samples, GBM), rows_p = round_up(rows, GBM);
        if (c.multitask) {
            if ((rc = build_task_tables(h, tk, false, rows_p, st))) return rc;
            if ((rc = model_launch_tile_tasks(tk->task_ids, B, (int)rows, (int)rows_p, h->task_rows, st))) return rc;
        }
        if ((rc = lay_set_qidx(h, st, 1, qidx, 2L, c.num_q, 0, seed, call, h->lay.qidx))) return rc;
        for (size_t r0 = 0; r0 < rows; r0 += cap) {
            const int n = (int)std::min(cap, rows - r0);
            if ((rc = lay_value(h, st, n, zs + r0 * c.latent_dim, false, false, pi_eps, h->lay.qidx, seed, call, nullptr, nullptr, 0.f,
                                c.multitask ? h->task_rows + r0 : nullptr, out->action ? out->action + r0 * c.action_dim : nullptr,
                                wq + r0, (int)r0, went + r0, wsent + r0))) return rc;
        }
        err = (h->split && h->lay.fuse_ln) ? h->cl_err_dev : nullptr;
    } else {
        if (c.multitask && (rc = build_task_tables(h, tk, false, 0, st))) return rc;
        ValueEntParams p{};
        p.rows = (int)rows; p.A = c.action_dim; p.Apad = h->Apad; p.nq = c.num_q; p.num_bins = c.num_bins; p.reduce_min = 0;
        p.log_std_min = c.log_std_min; p.log_std_dif = c.log_std_dif;
        p.pi = to_dev(h->pi);
        for (int i = 0; i < c.num_q; ++i) p.q[i] = to_dev(h->q[i]);
        p.bins = h->bins; p.z = zs; p.pi_eps = pi_eps; p.qidx = qidx; p.seed = seed; p.call = call;
        p.action = out->action; p.out = wq; p.entropy = went; p.scaled_entropy = wsent;
        p.nnets = h->nnets;
        if (c.multitask) { p.task_ids = tk->task_ids; p.beff_tab = h->beff_tab; p.mask_tab = h->mask_tab; p.task_mod = B; }
        policy_loss_ops(h->Apad).value_ent(h->split ? 0 : 1, p, (int)((rows + ROWS - 1) / ROWS), h->lds_bytes, st);
        HIP_TRY(hipGetLastError());
    }
    if (in->update_scale && (rc = pl_launch_scale(RunningScaleParams{wq, B, in->tau, scale, out->percentiles, err}, st))) return rc;
    PolicyLossTailParams tp{};
    tp.q = wq; tp.entropy = went; tp.scaled_entropy = wsent; tp.scale = scale; tp.B = B; tp.T = T; tp.entropy_coef = in->entropy_coef;
    for (int t = 0; t < T; ++t) tp.rho_pow[t] = std::pow(in->rho, (float)t);  // torch.pow(rho, arange) in fp32 (tdmpc2.py:227)
    tp.step_means = out->step_means; tp.loss = loss; tp.err = err;
    tp.action = out->action; tp.A = c.action_dim;
    if ((rc = pl_launch_tail(tp, st))) return rc;
    if (out->q) HIP_TRY(hipMemcpyAsync(out->q, wq, rows * 4, hipMemcpyDeviceToDevice, st));
    if (out->entropy) HIP_TRY(hipMemcpyAsync(out->entropy, went, rows * 4, hipMemcpyDeviceToDevice, st));
    if (out->scaled_entropy) HIP_TRY(hipMemcpyAsync(out->scaled_entropy, wsent, rows * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}
}  // namespace

int tdmpc2_plan_policy_loss_mt(tdmpc2_plan_t *h, int batch, int steps, const float *zs, const tdmpc2_task_tables *tasks,
                               const float *pi_eps, const int32_t *qidx, uint64_t seed, const tdmpc2_policy_loss_in *in,
                               float *scale, const tdmpc2_policy_loss_out *out, float *loss, void *stream) {
    if (!h || !zs || !in || !scale || !loss) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    return launch_policy_loss(h, batch, steps, zs, tasks, pi_eps, qidx, seed, in, scale, out, loss, (hipStream_t)stream);
}
int tdmpc2_plan_policy_loss(tdmpc2_plan_t *h, int batch, int steps, const float *zs, const float *pi_eps, const int32_t *qidx,
                            uint64_t seed, const tdmpc2_policy_loss_in *in, float *scale, const tdmpc2_policy_loss_out *out,
                            float *loss, void *stream) {
    return tdmpc2_plan_policy_loss_mt(h, batch, steps, zs, nullptr, pi_eps, qidx, seed, in, scale, out, loss, stream);
}
int tdmpc2_plan_running_scale(tdmpc2_plan_t *h, int n, const float *x, float tau, float *scale, float *percentiles, void *stream) {
    if (!h || !x || !scale) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n < 1) return fail(TDMPC2_ERR_INVALID, "n %d < 1", n);
    if (n > PL_SCALE_MAX_N) return fail(TDMPC2_ERR_UNSUPPORTED, "the running scale takes at most %d values; got %d", (int)PL_SCALE_MAX_N, n);
    ENTER_ON(h, stream);
    return pl_launch_scale(RunningScaleParams{x, n, tau, scale, percentiles, nullptr}, (hipStream_t)stream);
}
int tdmpc2_plan_termination_stats(tdmpc2_plan_t *h, int n, const float *term_logit, const float *terminated, float *stats,
                                  void *stream) {
    if (!h || !term_logit || !terminated || !stats) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n < 1) return fail(TDMPC2_ERR_INVALID, "n %d < 1", n);
    ENTER_ON(h, stream);
    return pl_launch_term_stats(TerminationStatsParams{term_logit, terminated, n, stats}, (hipStream_t)stream);
}

// ---------------------------------------------------------------- one plan sharded over several GPUs (last row)
// The sample rows of every plan are split over the ranks; everything else is replicated: every rank holds the weights, runs
// the identical set-up, draws the identical actions (same tape / same Philox seed) and performs the identical elite
// selection + refit on the all-gathered values.  Per CEM iteration a rank calls shard_values for ITS row range, the host
// all-gathers value[E, N / G] over RCCL (4 KB per plan), and every rank calls shard_refit.  tdmpc2_amd/dist.py drives it.
int tdmpc2_plan_shard_begin(tdmpc2_plan_t *h, int n_envs, const float *z0, const float *task_emb, const float *act_mask,
                            const float *prev_mean, const uint8_t *t0, const tdmpc2_noise *tape, uint64_t seed, void *stream) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    ENTER_ON(h, stream);
    int rc = validate_envs(h, n_envs);
    if (rc) return rc;
    if (!z0 || !prev_mean || !t0) return fail(TDMPC2_ERR_INVALID, "null argument");
    const tdmpc2_plan_cfg &c = h->cfg;
    if (c.multitask && (!task_emb || !act_mask)) return fail(TDMPC2_ERR_INVALID, "multitask plan needs task_emb and act_mask");
    if (!c.multitask) { task_emb = nullptr; act_mask = nullptr; }
    if (tape && c.num_pi_trajs > 0 && !tape->pi_traj_eps) return fail(TDMPC2_ERR_INVALID, "noise tape has null fields");
    hipStream_t st = (hipStream_t)stream;
    const unsigned call = h->call++;
    h->shard_call = call;
    // in_shard: no re-arm between the calls of this plan (fault_clean), word 0 of the error line kept until the final pick.  Set
    // only when the whole prologue has been enqueued: a shard_begin that fails leaves the handle as an ordinary call would.
    struct ShardGuard {
        tdmpc2_plan *h; bool ok;
        ~ShardGuard() { h->in_shard = ok; }
    } guard{h, false};
    const int E = n_envs, P = c.num_pi_trajs;
    if (h->lay.on) {
        if ((rc = fault_fresh(h, st))) return rc;
        if ((rc = lay_setup(h, st, E, task_emb, prev_mean, t0, true))) return rc;
        if ((rc = lay_cvec(h, st, E, z0))) return rc;
        if (P > 0 && (rc = lay_pitraj(h, st, E, z0, act_mask, tape ? tape->pi_traj_eps : nullptr, seed, call))) return rc;
        guard.ok = true;
        return TDMPC2_OK;
    }
    const FusedRoute r = fused_route_shard(fused_in(h, E), 0, c.num_samples);
    if ((rc = launch_setup(h, r, E, z0, task_emb, prev_mean, t0, st))) return rc;
    if (r.pitraj && (rc = launch_pitraj(h, r, E, z0, act_mask, tape, seed, call, st))) return rc;
    guard.ok = true;
    return TDMPC2_OK;
}

int tdmpc2_plan_shard_values(tdmpc2_plan_t *h, int n_envs, int iter, int row_begin, int row_end, const float *z0,
                             const float *act_mask, const float *disc_pow, const tdmpc2_noise *tape, uint64_t seed,
                             float *value, void *stream) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    ENTER_ON(h, stream);
    int rc = validate_envs(h, n_envs);
    if (rc) return rc;
    if (!z0 || !disc_pow || !value) return fail(TDMPC2_ERR_INVALID, "null argument");
    const tdmpc2_plan_cfg &c = h->cfg;
    const int E = n_envs, N = c.num_samples, A = c.action_dim, I = c.iterations;
    if (iter < 0 || iter >= I) return fail(TDMPC2_ERR_INVALID, "iteration %d outside [0, %d)", iter, I);
    const int gran = h->lay.on ? GBM : ROWS;
    if (row_begin < 0 || row_end > N || row_begin >= row_end || row_begin % gran || row_end % gran)
        return fail(TDMPC2_ERR_INVALID, "row range [%d, %d) must be non-empty, inside [0, %d) and aligned to %d rows", row_begin, row_end, N, gran);
    if (c.multitask && !act_mask) return fail(TDMPC2_ERR_INVALID, "multitask plan needs act_mask");
    if (!c.multitask) act_mask = nullptr;
    if (tape && (!tape->sample_eps || !tape->pi_eps || !tape->qidx)) return fail(TDMPC2_ERR_INVALID, "noise tape has null fields");
    hipStream_t st = (hipStream_t)stream;
    const unsigned call = h->shard_call;
    // (1) the actions of ALL rows of this iteration (replicated: the refit needs every elite's actions)
    int *qbuf = h->lay.on ? h->lay.qidx : h->qidx_buf;
    if ((rc = lay_sample_iteration(h, st, E, iter, act_mask, tape, seed, call, qbuf))) return rc;
    const float *pi_eps = tape ? tape->pi_eps + (size_t)iter * N * A : nullptr;
    // (2) this rank's rows
    if (h->lay.on)
        return lay_estimate_value(h, st, E, z0, act_mask, disc_pow, h->actions, pi_eps, (long)I * N * A, qbuf, seed, call, iter, value,
                                  nullptr, row_begin, row_end - row_begin);
    const FusedRoute r = fused_route_shard(fused_in(h, E), row_begin, row_end);
    RolloutParams rp{};
    fill_rollout(h, r, rp, E);
    rp.z0 = z0; rp.act_mask = act_mask; rp.disc_pow = disc_pow; rp.seed = seed; rp.call = call; rp.given_actions = 1; rp.iter = iter;
    rp.value = value; rp.pi_eps = pi_eps; rp.pi_eps_estride = (long)I * N * A; rp.qidx = qbuf; rp.qidx_estride = 2;
    return launch_rollout(h, r, rp, st);
}

int tdmpc2_plan_shard_refit(tdmpc2_plan_t *h, int n_envs, int iter, float *value, const float *act_mask, float *prev_mean,
                            int eval_mode, const tdmpc2_noise *tape, uint64_t seed, float *action, const tdmpc2_debug *dbg,
                            void *stream) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    ENTER_ON(h, stream);
    if (n_envs < 1 || n_envs > h->cfg.max_envs) return fail(TDMPC2_ERR_INVALID, "n_envs=%d outside [1, %d]", n_envs, h->cfg.max_envs);
    if (!value || !prev_mean || !action) return fail(TDMPC2_ERR_INVALID, "null argument");
    const tdmpc2_plan_cfg &c = h->cfg;
    if (iter < 0 || iter >= c.iterations) return fail(TDMPC2_ERR_INVALID, "iteration %d outside [0, %d)", iter, c.iterations);
    if (tape && (!tape->gumbel_exp || (!eval_mode && !tape->final_eps))) return fail(TDMPC2_ERR_INVALID, "noise tape has null fields");
    hipStream_t st = (hipStream_t)stream;
    int stage = 0, rc;
    const size_t lds = refit_lds_bytes(c.num_samples, c.num_elites, c.horizon, c.action_dim, &stage);
    RefitParams fp;
    // err: a bounded inter-workgroup wait (fused NormedLinear epilogue) that gave up in ANY iteration of this sharded plan: NaN
    // action, prev_mean kept -- word 0 is cleared by shard_begin only (in stream order), not by the calls in between
    fill_refit(h, fp, n_envs, iter, eval_mode, value, c.multitask ? act_mask : nullptr, tape, seed, h->shard_call, prev_mean, action, dbg,
               stage, h->cl_err_dev);
    if ((rc = launch_refit(fp, n_envs, c.num_samples, lds, st))) return rc;
    if (fp.last) {
        h->in_shard = false;
        if (h->safe_once) { h->safe_once = false; apply_modes(h); }
    }
    return dump_actions(h, dbg, n_envs, iter, st);
}

// ---------------------------------------------------------------- packed weight file
// Everything a bind produces -- fragment-ordered (and, for the split arithmetic, hi/lo-split and scaled) weights, padded
// biases, LayerNorm parameters, task-embedding columns, the per-layer scale records, the transposed encoder -- as one
// host blob: [PackHdr][segment sizes][segment data].  Importing it is a sequence of plain host-to-device copies: no
// packing kernels, no fp32 checkpoint on the device (reference load path: tdmpc2/tdmpc2.py:81-95).
namespace {
struct PackHdr {
    char magic[8];
    uint32_t version, abi;
    tdmpc2_plan_cfg cfg;  // as resolved by create (path and precision are concrete); max_envs / device are not compared
    uint32_t has_target, enc_layers;
    int32_t enc_in[ENC_MAX_LAYERS], enc_out[ENC_MAX_LAYERS];
    uint64_t nseg, data_bytes;
};
struct Seg {
    void *p;
    size_t bytes;
};
const int kPackNets[] = {TDMPC2_NET_DYNAMICS, TDMPC2_NET_REWARD, TDMPC2_NET_PI, TDMPC2_NET_TERMINATION, TDMPC2_NET_Q, TDMPC2_NET_TARGET_Q};

bool net_in_pack(const tdmpc2_plan *h, int net, bool has_target) {
    if (net == TDMPC2_NET_TERMINATION) return h->cfg.episodic != 0;
    if (net == TDMPC2_NET_TARGET_Q) return has_target;
    return true;
}
// canonical walk; every visited layer must be allocated
void collect_segments(tdmpc2_plan *h, bool has_target, int enc_layers, std::vector<Seg> &out) {
    for (int net : kPackNets) {
        if (!net_in_pack(h, net, has_target)) continue;
        const int heads = layer_shape(h, net, 0).heads;
        for (int hd = 0; hd < heads; ++hd) {
            HostNet *N = net_of(h, net, hd);
            for (int l = 0; l < 3; ++l) {
                const LayerShape sh = layer_shape(h, net, l);
                HostLayer &L = N->l[l];
                out.push_back({h->split ? (void *)L.wps : (void *)L.wp, sh.wsz * 4});
                out.push_back({L.bias, sh.bsz * 4});
                if (sh.has_ln) {
                    out.push_back({L.g, sh.gsz * 4});
                    out.push_back({L.b, sh.gsz * 4});
                }
                if (sh.nt > 0) out.push_back({L.wemb, sh.esz * 4});
            }
            if (h->split) out.push_back({N->scal, 3 * sizeof(LayerScal)});
        }
    }
    for (int l = 0; l < enc_layers; ++l) {
        tdmpc2_plan::Enc &E = h->enc[l];
        out.push_back({E.wt, (size_t)E.in * E.out * 4});
        out.push_back({E.bias, (size_t)E.out * 4});
        out.push_back({E.g, (size_t)E.out * 4});
        out.push_back({E.b, (size_t)E.out * 4});
    }
}
bool target_bound(const tdmpc2_plan *h) {
    for (int i = 0; i < 3; ++i)
        for (int q = 0; q < h->cfg.num_q; ++q)
            if (!h->tq[q].l[i].bound) return false;
    return true;
}
bool same_model(const tdmpc2_plan_cfg &a, const tdmpc2_plan_cfg &b) {
    return a.horizon == b.horizon && a.num_samples == b.num_samples && a.action_dim == b.action_dim && a.latent_dim == b.latent_dim &&
           a.mlp_dim == b.mlp_dim && a.task_dim == b.task_dim && a.num_bins == b.num_bins && a.num_q == b.num_q &&
           a.simnorm_dim == b.simnorm_dim && a.multitask == b.multitask && a.episodic == b.episodic && a.path == b.path &&
           a.precision == b.precision;
}
}  // namespace

int tdmpc2_plan_packed_size(tdmpc2_plan_t *h, uint64_t *bytes) {
    if (!h || !bytes) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER(h);
    int rc = check_ready(h);
    if (rc) return rc;
    std::vector<Seg> segs;
    collect_segments(h, target_bound(h), h->enc_layers, segs);
    uint64_t total = sizeof(PackHdr) + segs.size() * sizeof(uint64_t);
    for (const Seg &sg : segs) total += sg.bytes;
    *bytes = total;
    return TDMPC2_OK;
}

int tdmpc2_plan_export_packed(tdmpc2_plan_t *h, void *host_buf, uint64_t bytes, void *stream) {
    if (!h || !host_buf) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    int rc = check_ready(h);
    if (rc) return rc;
    for (int l = 0; l < h->enc_layers; ++l)
        if (!h->enc[l].bound) return fail(TDMPC2_ERR_STATE, "encoder layer %d of %d is not bound", l, h->enc_layers);
    const bool has_target = target_bound(h);
    std::vector<Seg> segs;
    collect_segments(h, has_target, h->enc_layers, segs);
    PackHdr hdr{};
    memcpy(hdr.magic, "TDMPC2PK", 8);
    hdr.version = 1; hdr.abi = TDMPC2_PLAN_ABI_VERSION; hdr.cfg = h->cfg; hdr.has_target = has_target ? 1 : 0;
    hdr.enc_layers = (uint32_t)h->enc_layers;
    for (int l = 0; l < h->enc_layers; ++l) { hdr.enc_in[l] = h->enc[l].in; hdr.enc_out[l] = h->enc[l].out; }
    hdr.nseg = segs.size();
    for (const Seg &sg : segs) hdr.data_bytes += sg.bytes;
    const uint64_t need = sizeof(PackHdr) + segs.size() * sizeof(uint64_t) + hdr.data_bytes;
    if (bytes < need) return fail(TDMPC2_ERR_INVALID, "buffer of %llu bytes, the packed weights need %llu", (unsigned long long)bytes, (unsigned long long)need);
    char *dst = static_cast<char *>(host_buf);
    memcpy(dst, &hdr, sizeof hdr);
    uint64_t *sizes = reinterpret_cast<uint64_t *>(dst + sizeof hdr);
    char *data = dst + sizeof hdr + segs.size() * sizeof(uint64_t);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // binds on this stream have landed
    for (size_t i = 0; i < segs.size(); ++i) {
        sizes[i] = segs[i].bytes;
        HIP_TRY(hipMemcpy(data, segs[i].p, segs[i].bytes, hipMemcpyDeviceToHost));
        data += segs[i].bytes;
    }
    return TDMPC2_OK;
}

int tdmpc2_plan_import_packed(tdmpc2_plan_t *h, const void *host_buf, uint64_t bytes, void *stream) {
    if (!h || !host_buf) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    if (bytes < sizeof(PackHdr)) return fail(TDMPC2_ERR_INVALID, "packed weights: truncated header");
    PackHdr hdr;
    memcpy(&hdr, host_buf, sizeof hdr);
    if (memcmp(hdr.magic, "TDMPC2PK", 8) != 0 || hdr.version != 1) return fail(TDMPC2_ERR_INVALID, "not a packed weight blob (magic / version)");
    if (!same_model(hdr.cfg, h->cfg))
        return fail(TDMPC2_ERR_INVALID, "packed weights were exported for another model / kernel family / arithmetic "
                    "(latent %d mlp %d A %d path %d precision %d; this handle: %d %d %d %d %d)", hdr.cfg.latent_dim, hdr.cfg.mlp_dim,
                    hdr.cfg.action_dim, hdr.cfg.path, hdr.cfg.precision, h->cfg.latent_dim, h->cfg.mlp_dim, h->cfg.action_dim,
                    h->cfg.path, h->cfg.precision);
    if (hdr.enc_layers > (uint32_t)ENC_MAX_LAYERS) return fail(TDMPC2_ERR_INVALID, "packed weights: bad encoder depth");
    if (h->enc_layers && hdr.enc_layers && h->enc_layers != (int)hdr.enc_layers)
        return fail(TDMPC2_ERR_STATE, "encoder depth changed from %d to %u", h->enc_layers, hdr.enc_layers);
    int rc;
    for (int net : kPackNets) {
        if (!net_in_pack(h, net, hdr.has_target != 0)) continue;
        for (int l = 0; l < 3; ++l)
            if ((rc = ensure_layer_alloc(h, net, l, layer_shape(h, net, l)))) return rc;
    }
    for (uint32_t l = 0; l < hdr.enc_layers; ++l) {  // untrusted header fields: range-check before anything is allocated
        const int wmax = ENC_THREADS * ENC_MAX_PER_THREAD;
        if (hdr.enc_in[l] < 1 || hdr.enc_in[l] > 1 << 20 || hdr.enc_out[l] < 1 || hdr.enc_out[l] > wmax)
            return fail(TDMPC2_ERR_INVALID, "packed weights: encoder layer %u has shape [%d, %d]", l, hdr.enc_out[l], hdr.enc_in[l]);
    }
    for (uint32_t l = 0; l < hdr.enc_layers; ++l)
        if ((rc = ensure_enc_alloc(h, (int)l, hdr.enc_in[l], hdr.enc_out[l]))) return rc;
    std::vector<Seg> segs;
    collect_segments(h, hdr.has_target != 0, (int)hdr.enc_layers, segs);
    // the blob must hold exactly what this handle expects: header + size table + the sum of the EXPECTED segment sizes (the
    // header's own data_bytes is only compared, never trusted; no addition can wrap)
    uint64_t expect = 0;
    for (const Seg &sg : segs) {
        if (sg.bytes > (uint64_t)1 << 40 || expect > (uint64_t)1 << 41) return fail(TDMPC2_ERR_INVALID, "packed weights: implausible segment size");
        expect += sg.bytes;
    }
    const uint64_t need = sizeof(PackHdr) + (uint64_t)segs.size() * sizeof(uint64_t) + expect;
    if (segs.size() != hdr.nseg || hdr.data_bytes != expect || bytes < need)
        return fail(TDMPC2_ERR_INVALID, "packed weights: %llu segments / %llu data bytes in a buffer of %llu bytes; this handle expects %zu segments / "
                    "%llu data bytes (%llu in all)", (unsigned long long)hdr.nseg, (unsigned long long)hdr.data_bytes, (unsigned long long)bytes,
                    segs.size(), (unsigned long long)expect, (unsigned long long)need);
    const char *src = static_cast<const char *>(host_buf);
    const uint64_t *sizes = reinterpret_cast<const uint64_t *>(src + sizeof hdr);
    for (size_t i = 0; i < segs.size(); ++i)
        if (sizes[i] != segs[i].bytes) return fail(TDMPC2_ERR_INVALID, "packed weights: segment %zu has %llu bytes, expected %zu", i, (unsigned long long)sizes[i], segs[i].bytes);
    const char *data = src + sizeof hdr + segs.size() * sizeof(uint64_t);
    hipStream_t st = (hipStream_t)stream;
    for (size_t i = 0; i < segs.size(); ++i) {
        HIP_TRY(hipMemcpyAsync(segs[i].p, data, segs[i].bytes, hipMemcpyHostToDevice, st));
        data += segs[i].bytes;
    }
    HIP_TRY(hipStreamSynchronize(st));  // the host blob may be released on return
    for (int net : kPackNets) {
        if (!net_in_pack(h, net, hdr.has_target != 0)) continue;
        const int heads = layer_shape(h, net, 0).heads;
        for (int hd = 0; hd < heads; ++hd)
            for (int l = 0; l < 3; ++l) net_of(h, net, hd)->l[l].bound = true;
    }
    for (uint32_t l = 0; l < hdr.enc_layers; ++l) h->enc[l].bound = true;
    if (hdr.enc_layers) h->enc_layers = (int)hdr.enc_layers;
    return TDMPC2_OK;
}

int tdmpc2_plan_export_noise(tdmpc2_plan_t *h, int env_first, int n_envs, uint64_t seed, uint32_t call,
                             const tdmpc2_noise_out *out, void *stream) {
    if (!h || !out) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (env_first < 0 || n_envs < 1) return fail(TDMPC2_ERR_INVALID, "environment range [%d, +%d)", env_first, n_envs);
    ENTER_ON(h, stream);
    const tdmpc2_plan_cfg &c = h->cfg;
    NoiseExportParams p{};
    p.e0 = env_first; p.n = n_envs; p.H = c.horizon; p.N = c.num_samples; p.P = c.num_pi_trajs; p.A = c.action_dim;
    p.K = c.num_elites; p.I = c.iterations; p.nq = c.num_q; p.hp = (c.action_dim + 15) / 16 * 8;
    p.seed = seed; p.call = call; p.o = *out;
    hipLaunchKernelGGL(k_export_noise, dim3(2048), dim3(256), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return TDMPC2_OK;
}

int tdmpc2_plan_call_counter(const tdmpc2_plan_t *h, uint32_t *next_call) {
    if (!h || !next_call) return fail(TDMPC2_ERR_INVALID, "null argument");
    *next_call = h->call;
    return TDMPC2_OK;
}

int tdmpc2_plan_set_call_counter(tdmpc2_plan_t *h, uint32_t next_call) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    ENTER(h);
    h->call = next_call;
    return TDMPC2_OK;
}

int tdmpc2_plan_fault_word(tdmpc2_plan_t *h, uint32_t *dst_dev, void *stream) {
    if (!h || !dst_dev) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    hipStream_t st = (hipStream_t)stream;
    // word 0 of the host-mapped error line, copied IN STREAM ORDER: what the kernels enqueued so far have raised when the copy runs
    if (h->cl_err_dev) HIP_TRY(hipMemcpyAsync(dst_dev, h->cl_err_dev, 4, hipMemcpyDefault, st));
    else HIP_TRY(hipMemsetAsync(dst_dev, 0, 4, st));
    return TDMPC2_OK;
}

int tdmpc2_plan_take_fault(tdmpc2_plan_t *h, int *faults) {
    if (!h || !faults) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER(h);
    (void)fault_poll(h);
    *faults = h->faults;
    h->faults = 0;
    return TDMPC2_OK;
}

int tdmpc2_plan_fault_info(tdmpc2_plan_t *h, tdmpc2_fault_info *info) {
    if (!h || !info) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER(h);
    info->faults_total = h->faults_total;
    info->rearms = h->rearms;
    info->degraded = h->degraded ? 1 : 0;
    info->clean_calls = h->clean_calls;
    info->rearm_after = h->rearm_after;
    info->seconds_since_fault = h->faults_total
        ? std::chrono::duration<double>(std::chrono::steady_clock::now() - h->last_fault).count() : -1.0;
    return TDMPC2_OK;
}

int tdmpc2_plan_set_tuning(tdmpc2_plan_t *h, int key, int value) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    if (key == TDMPC2_TUNE_ROWS_PER_WORKGROUP) {
        if (value != 0 && value != 32 && value != 64) return fail(TDMPC2_ERR_INVALID, "rows per workgroup must be 0, 32 or 64");
        h->force_rows = value;
        return TDMPC2_OK;
    }
    if (key == TDMPC2_TUNE_CLUSTER) {
        if (value < 0 || value > 2) return fail(TDMPC2_ERR_INVALID, "cluster must be 0 (never), 1 (whenever the call fits) or 2 (auto)");
        h->user_cluster_mode = value;  // an explicit setting also re-arms the handle at once
        h->degraded = false;
        apply_modes(h);
        return TDMPC2_OK;
    }
    if (key == TDMPC2_TUNE_FUSE_LN) {
        if (value < 0 || value > 1) return fail(TDMPC2_ERR_INVALID, "fuse_ln must be 0 or 1");
        h->user_fuse_ln = value != 0 && h->lay.stats != nullptr;
        h->degraded = false;
        apply_modes(h);
        return TDMPC2_OK;
    }
    if (key == TDMPC2_TUNE_REARM_AFTER) {
        if (value < 0) return fail(TDMPC2_ERR_INVALID, "rearm_after must be >= 0 (0: never)");
        h->rearm_after = h->rearm_base = value;
        return TDMPC2_OK;
    }
    if (key == TDMPC2_TUNE_SAFE_ONCE) {
        // the next whole plan (tdmpc2_plan_run*, or shard_begin .. the last shard_refit) runs on the paths without inter-workgroup
        // waits; the caller's settings, the downgrade state and the re-arm counter are not touched (dist.sharded_plan's re-plan)
        if (value < 0 || value > 1) return fail(TDMPC2_ERR_INVALID, "safe_once must be 0 or 1");
        h->safe_once = value != 0;
        apply_modes(h);
        return TDMPC2_OK;
    }
    if (key == TDMPC2_TUNE_KSPLIT) {
        if (value < 0 || value > 2) return fail(TDMPC2_ERR_INVALID, "ksplit must be 0 (never), 1 (always) or 2 (few-tile launches)");
        {
            DevGuard dev_(h->cfg.device);
            const int rc = ksws_ensure(h, value);  // (a bigger workspace when the mode needs one)
            if (rc) return rc;
        }
        h->lay.ksplit = value;
        return TDMPC2_OK;
    }
    if (key >= TDMPC2_TUNE_EXPERT && key < TDMPC2_TUNE_EXPERT + LK_COUNT) {
        // measurement knobs of the layered family's tile choice (layer_route.h: LayKnob, LAY_KNOBS; include/tdmpc2_plan.h: tdmpc2_expert_knob).
        // INT32_MIN restores the default.  They move work between kernels that compute the same values to fp32 round-off.
        const LayKnobSpec &k = LAY_KNOBS[key - TDMPC2_TUNE_EXPERT];
        if (value != INT32_MIN && (value < k.lo || value > k.hi))
            return fail(TDMPC2_ERR_INVALID, "expert knob %d: %d is outside %d .. %d", key - TDMPC2_TUNE_EXPERT, value, k.lo, k.hi);
        h->lay.knob[key - TDMPC2_TUNE_EXPERT] = value == INT32_MIN ? k.def : value;
        return TDMPC2_OK;
    }
    if (key == TDMPC2_TUNE_WAIT_US) {
        if (value < 100 || value > 10000000) return fail(TDMPC2_ERR_INVALID, "wait_us must be 100 .. 10 000 000");
        if (!h->cl_err_host) return fail(TDMPC2_ERR_STATE, "this handle has no path with inter-workgroup waits");
        // 100 MHz constant clock (s_memrealtime): 100 ticks per microsecond; word 12 of the host-mapped error line (WaitClock)
        __atomic_store_n(h->cl_err_host + ERR_WAIT_TICKS, (unsigned int)std::min<long long>(100LL * value, 0xffffffffLL), __ATOMIC_RELAXED);
        return TDMPC2_OK;
    }
    if (key == TDMPC2_TUNE_FEWROW) {
        if (value < 0 || value > 1) return fail(TDMPC2_ERR_INVALID, "fewrow must be 0 or 1");
        h->lay.mid = value != 0;
        return TDMPC2_OK;
    }
    if (key == TDMPC2_TUNE_POLICY_ROUTE) {
        if (value == INT32_MIN) value = POL_AUTO;
        if (value < POL_AUTO || value > POL_FORCE_SPREAD) return fail(TDMPC2_ERR_INVALID, "policy route must be 0 (auto), 1 (row) or 2 (spread)");
        h->pol.mode = value;
        return TDMPC2_OK;
    }
    if (key == TDMPC2_TUNE_FOLD_REFIT) {
        if (value < 0 || value > 2) return fail(TDMPC2_ERR_INVALID, "fold_refit must be 0 (never), 1 (always) or 2 (auto)");
        h->fold_refit = value;
        return TDMPC2_OK;
    }
    return fail(TDMPC2_ERR_INVALID, "unknown tuning key %d", key);
}

int tdmpc2_plan_set_profiling(tdmpc2_plan_t *h, int max_launches) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    ENTER(h);
    h->profiling = max_launches > 0;
    if ((int)h->ev.size() < 2 * max_launches) {
        const size_t old = h->ev.size();
        h->ev.resize(2 * (size_t)max_launches);
        for (size_t i = old; i < h->ev.size(); ++i) HIP_TRY(hipEventCreate(&h->ev[i]));
    }
    h->ev_used = 0;
    return TDMPC2_OK;
}

int tdmpc2_plan_profile_read(tdmpc2_plan_t *h, float *rollout_ms_total, int *rollout_launches) {
    if (!h || !rollout_ms_total || !rollout_launches) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER(h);
    float total = 0.f;
    for (int i = 0; i + 1 < h->ev_used; i += 2) {
        HIP_TRY(hipEventSynchronize(h->ev[i + 1]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
        total += ms;
    }
    *rollout_ms_total = total;
    *rollout_launches = h->ev_used / 2;
    h->ev_used = 0;
    return TDMPC2_OK;
}

int tdmpc2_plan_run(tdmpc2_plan_t *h, int n_envs, const float *z0, const float *task_emb, const float *act_mask,
                    const float *disc_pow, float *prev_mean, const uint8_t *t0, int eval_mode, const tdmpc2_noise *tape,
                    uint64_t seed, float *action, const tdmpc2_debug *dbg, void *stream) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    ENTER_ON(h, stream);
    return run_impl(h, n_envs, z0, task_emb, act_mask, disc_pow, prev_mean, t0, eval_mode, tape, seed, action, dbg, stream);
}

}  // extern "C"
namespace {
int run_impl(tdmpc2_plan *h, int n_envs, const float *z0, const float *task_emb, const float *act_mask, const float *disc_pow,
             float *prev_mean, const uint8_t *t0, int eval_mode, const tdmpc2_noise *tape, uint64_t seed, float *action,
             const tdmpc2_debug *dbg, void *stream) {
    if (h) h->in_shard = false;  // a whole plan on this handle abandons whatever sharded plan was left open (an exception in the caller)
    int rc = validate_envs(h, n_envs);
    if (rc) return rc;
    if (!z0 || !disc_pow || !prev_mean || !t0 || !action) return fail(TDMPC2_ERR_INVALID, "null argument");
    const tdmpc2_plan_cfg &c = h->cfg;
    if (c.multitask && (!task_emb || !act_mask)) return fail(TDMPC2_ERR_INVALID, "multitask plan needs task_emb and act_mask");
    if (!c.multitask) { task_emb = nullptr; act_mask = nullptr; }
    if (tape && (!tape->sample_eps || !tape->pi_eps || !tape->qidx || !tape->gumbel_exp ||
                 (c.num_pi_trajs > 0 && !tape->pi_traj_eps) || (!eval_mode && !tape->final_eps)))
        return fail(TDMPC2_ERR_INVALID, "noise tape has null fields");
    hipStream_t st = (hipStream_t)stream;
    struct SafeOnce {  // TDMPC2_TUNE_SAFE_ONCE covers exactly this plan
        tdmpc2_plan *h;
        ~SafeOnce() { if (h->safe_once) { h->safe_once = false; apply_modes(h); } }
    } once{h};
    if (h->lay.on) {
        if ((rc = fault_fresh(h, st))) return rc;
        return lay_run(h, st, n_envs, z0, task_emb, act_mask, disc_pow, prev_mean, t0, eval_mode, tape, seed, action, dbg);
    }
    return fused_run(h, st, n_envs, z0, task_emb, act_mask, disc_pow, prev_mean, t0, eval_mode, tape, seed, action, dbg);
}
}  // namespace
extern "C" {

int tdmpc2_plan_estimate_value(tdmpc2_plan_t *h, int n_envs, const float *z0, const float *task_emb,
                               const float *act_mask, const float *disc_pow, const float *actions, const float *pi_eps,
                               const int32_t *qidx, float *value, void *stream) {
    return tdmpc2_plan_estimate_value_trace(h, n_envs, z0, task_emb, act_mask, disc_pow, actions, pi_eps, qidx, value,
                                            nullptr, nullptr, stream);
}

int tdmpc2_plan_estimate_value_trace(tdmpc2_plan_t *h, int n_envs, const float *z0, const float *task_emb,
                                     const float *act_mask, const float *disc_pow, const float *actions,
                                     const float *pi_eps, const int32_t *qidx, float *value, float *trace_tiles,
                                     float *trace_scalars, void *stream) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    ENTER_ON(h, stream);
    int rc = validate_envs(h, n_envs);
    if (rc) return rc;
    if (!z0 || !disc_pow || !actions || !pi_eps || !qidx || !value) return fail(TDMPC2_ERR_INVALID, "null argument");
    const tdmpc2_plan_cfg &c = h->cfg;
    if (c.multitask && (!task_emb || !act_mask)) return fail(TDMPC2_ERR_INVALID, "multitask needs task_emb and act_mask");
    if (!c.multitask) { task_emb = nullptr; act_mask = nullptr; }
    hipStream_t st = (hipStream_t)stream;
    const int E = n_envs, N = c.num_samples, A = c.action_dim;
    if ((rc = fault_fresh(h, st))) return rc;
    if (h->lay.on) {
        if (trace_tiles) return fail(TDMPC2_ERR_UNSUPPORTED, "the layered path dumps trace_scalars only");
        if ((rc = lay_setup(h, st, E, task_emb, nullptr, nullptr, false))) return rc;
        if ((rc = lay_cvec(h, st, E, z0))) return rc;
        if ((rc = lay_set_qidx(h, st, E, qidx, 2L, c.num_q, 0, 0, 0, h->lay.qidx))) return rc;
        return lay_estimate_value(h, st, E, z0, act_mask, disc_pow, actions, pi_eps, (long)N * A, h->lay.qidx, 0, 0, 0, value,
                                  trace_scalars);
    }
    return fused_estimate_value(h, st, E, z0, task_emb, act_mask, disc_pow, actions, pi_eps, qidx, value, trace_tiles,
                                      trace_scalars);
}

int tdmpc2_plan_refit(tdmpc2_plan_t *h, int n_envs, float *value, const float *actions, const float *act_mask,
                      float *mean, float *std, float *score, int32_t *elite_idx, void *stream) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    if (n_envs < 1 || n_envs > h->cfg.max_envs) return fail(TDMPC2_ERR_INVALID, "n_envs=%d outside [1, %d]", n_envs, h->cfg.max_envs);
    if (!value || !actions) return fail(TDMPC2_ERR_INVALID, "null argument");
    ENTER_ON(h, stream);
    const tdmpc2_plan_cfg &c = h->cfg;
    hipStream_t st = (hipStream_t)stream;
    int refit_stage = 0;
    const size_t refit_lds = refit_lds_bytes(c.num_samples, c.num_elites, c.horizon, c.action_dim, &refit_stage);
    RefitParams fp{};
    fp.Nvalid = c.num_valid_samples; fp.E = n_envs; fp.N = c.num_samples; fp.H = c.horizon; fp.A = c.action_dim; fp.K = c.num_elites; fp.last = 0; fp.stage = refit_stage;
    fp.temperature = c.temperature; fp.min_std = c.min_std; fp.max_std = c.max_std;
    fp.value = value; fp.actions = actions; fp.act_mask = c.multitask ? act_mask : nullptr;
    fp.mean = mean ? mean : h->mean; fp.std = std ? std : h->std; fp.score = score; fp.elite_idx = elite_idx;
    return launch_refit(fp, n_envs, c.num_samples, refit_lds, st);
}

// ================================================================ pixel encoder, batch route (k_pixel_batch.hip, pixel_batch_route.h)
// Training batches of frame stacks: any number of images, in passes over a workspace that tdmpc2_plan_pix_batch_reserve sized.
// The weights, biases and ShiftAug table are the ones tdmpc2_plan_bind_pixel_encoder keeps for the planning routes.
namespace {
int check_pixb_handle(tdmpc2_plan *h) {
    if (h->cfg.multitask) return fail(TDMPC2_ERR_UNSUPPORTED, "the pixel encoder is single-task only (multitask handle)");
    for (int l = 0; l < PIX_LAYERS; ++l)
        if (!h->pix.bound[l]) return fail(TDMPC2_ERR_STATE, "no pixel encoder bound (layer %d; tdmpc2_plan_bind_pixel_encoder)", l);
    return 0;
}
}  // namespace

int tdmpc2_plan_pix_batch_reserve(tdmpc2_plan_t *h, int chunk_images, void *stream) {
    if (!h) return fail(TDMPC2_ERR_INVALID, "null handle");
    if (chunk_images < 1) return fail(TDMPC2_ERR_INVALID, "chunk_images %d < 1", chunk_images);
    int rc = check_pixb_handle(h);
    if (rc) return rc;
    ENTER_ON(h, stream);
    tdmpc2_plan::Pix &P = h->pix;
    if (chunk_images <= P.bchunk) return TDMPC2_OK;  // grows, never shrinks
    if (!P.bchunk && (rc = tdk::pixb_set_lds(pixb_lds(0, PIX_MAX_C, PIX_MAX_CIN)))) return rc;
    if ((rc = grow_ws(h, &P.bws, &P.bws_cap, (size_t)chunk_images * pix_ws_floats(P.C), (hipStream_t)stream))) return rc;
    P.bchunk = chunk_images;
    return TDMPC2_OK;
}

int tdmpc2_plan_encode_pix_batch(tdmpc2_plan_t *h, int n_images, const void *obs, int obs_dtype, int in_channels,
                                 const int32_t *shift, float *z_out, void *stream) {
    if (!h || !obs || !shift || !z_out) return fail(TDMPC2_ERR_INVALID, "null argument");
    if (n_images < 1) return fail(TDMPC2_ERR_INVALID, "n_images %d < 1", n_images);
    if (obs_dtype != 0 && obs_dtype != 1) return fail(TDMPC2_ERR_INVALID, "obs_dtype %d (0 = uint8, 1 = float32)", obs_dtype);
    if (in_channels < 1 || in_channels > PIX_MAX_CIN)
        return fail(TDMPC2_ERR_INVALID, "pixel encoder: %d input channels outside [1, %d]", in_channels, PIX_MAX_CIN);
    int rc = check_pixb_handle(h);
    if (rc) return rc;
    const tdmpc2_plan::Pix &P = h->pix;
    if (in_channels != P.cin)
        return fail(TDMPC2_ERR_INVALID, "pixel encoder: the observation has %d channels, layer 0 was bound with %d", in_channels, P.cin);
    if (!P.bchunk) return fail(TDMPC2_ERR_STATE, "no batch workspace reserved (tdmpc2_plan_pix_batch_reserve)");
    ENTER_ON(h, stream);
    PixbParams p{};
    for (int l = 0; l < PIX_LAYERS; ++l) { p.wp[l] = P.wp[l]; p.bias[l] = P.bias[l]; }
    p.cin = P.cin; p.C = P.C; p.tab = static_cast<const PixTap *>(P.tab); p.ws = P.bws;
    const size_t img_bytes = (size_t)P.cin * PIX_IN * PIX_IN * (obs_dtype == 0 ? 1 : 4);
    for (int i = 0; i < pixb_chunks(n_images, P.bchunk); ++i) {
        const int e0 = pixb_chunk_begin(i, P.bchunk);
        p.n = pixb_chunk_count(n_images, P.bchunk, i);
        p.obs = static_cast<const char *>(obs) + (size_t)e0 * img_bytes;
        p.shift = shift + 2 * (size_t)e0;
        p.z = z_out + (size_t)e0 * 16 * P.C;
        for (int l = 0; l < PIX_LAYERS; ++l)
            if ((rc = tdk::pixb_launch(l, obs_dtype == 0, p, pixb_grid(l, p.n, P.C, P.cin), (hipStream_t)stream))) return rc;
    }
    return TDMPC2_OK;
}

}  // extern "C"
