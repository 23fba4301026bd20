// MI355X (gfx950 / CDNA4) native TD-MPC2 planner: the core of the C ABI (include/tdmpc2_plan.h).
//
// This unit: error reporting (tdmpc2_last_error), the handle's create and destroy (every size is plan_layout.h's; the
// reference builds the same state in TDMPC2.__init__, tdmpc2/tdmpc2.py:17-44, and WorldModel.__init__,
// tdmpc2/common/world_model.py:17-36), the pool of side streams, the stream hand-over guard, the handle's allocations,
// the recovery from a bounded inter-workgroup wait that gave up, tuning, profiling, the call counter and the fault queries.
// What the other host units share of it is declared in plan_host.h:
//   plan_weights.hip   binds, the weight packer's job tables, the packed blob
//   plan_run.hip       planning (TDMPC2._plan, _estimate_value), the refit, sharded plans, the noise export
//   plan_obs.hip       observations to latents and the policy prior (WorldModel.encode, WorldModel.pi, act())
//   plan_train.hip     the forward halves of TDMPC2._update and update_pi
// Every kernel is instantiated in a k_*.hip unit and reached through launch.h; DESIGN.md has the full account.
// The test hooks (-DTDMPC2_TEST_HOOKS: TDMPC2_CLUSTER_FAULT, TDMPC2_DEBUG_NO_TURN, TDMPC2_POISON) are all in this unit:
// libtdmpc2_plan_hooks.so is the product's objects with the hooks build of this one in place of the plain one.
#include <cstdarg>
#include <cstring>
#include <new>

#include "plan_host.h"

namespace {
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

namespace tdk {

StreamTurn::StreamTurn(tdmpc2_plan *hh, hipStream_t s) : h(hh), st(s), live(false), err(hipSuccess) {
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
StreamTurn::~StreamTurn() {
    if (!live) return;
    if (hipEventRecord(h->turn_ev, st) == hipSuccess) {
        h->turn_stream = st;
        h->turn_valid = true;
    }
}

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

static void dev_release(tdmpc2_plan *h, void *p) {  // free one allocation made with dev_alloc (tables that are re-grown)
    if (!p) return;
    for (size_t i = 0; i < h->allocs.size(); ++i)
        if (h->allocs[i] == p) {
            h->allocs.erase(h->allocs.begin() + (long)i);
            break;
        }
    (void)hipFree(p);
}

int grow_ws(tdmpc2_plan *h, size_t *cap, size_t want, std::initializer_list<WsBuf> bufs, hipStream_t st) {
    if (want <= *cap) return 0;
    HIP_TRY(hipStreamSynchronize(st));
    for (const WsBuf &b : bufs) {
        dev_release(h, *b.p);
        *b.p = nullptr;
    }
    *cap = 0;
    for (const WsBuf &b : bufs)
        if (int rc = dev_alloc(h, b.p, b.bytes)) return rc;
    *cap = want;
    return 0;
}

// g_gemm_w's K-split workspaces, one per chain, of ksws_slots(..., mode) slots (plan_layout.h).  Called at create and when
// tdmpc2_plan_set_tuning raises the mode (grows, never shrinks; the smaller buffers stay with the handle until destroy).  `mode`: the
// K-split mode the workspaces are for -- the caller stores it only once they are there; a failed second allocation releases the first.
static int ksws_ensure(tdmpc2_plan *h, int mode) {
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
static void fault_note(tdmpc2_plan *h) {
    if (h->degraded && h->rearm_after > 0 && h->rearm_after < 4096)
        h->rearm_after *= 2;  // (a fault on the downgraded paths cannot happen; this branch is a fault right after a re-arm raced in)
    h->degraded = true;
    apply_modes(h);
    h->clean_calls = 0;
    h->faults++;
    h->faults_total++;
    h->last_fault = std::chrono::steady_clock::now();
}
static void fault_clean(tdmpc2_plan *h) {  // a call is about to be enqueued and no fault is pending
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

}  // namespace tdk

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

}  // extern "C"
