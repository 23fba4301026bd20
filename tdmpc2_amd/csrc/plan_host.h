// What the host units of the planner's C ABI share (plan_core.hip, plan_weights.hip, plan_run.hip, plan_obs.hip,
// plan_train.hip), on top of the handle (handle.h) and the kernel launchers (launch.h): the guards every entry point opens with,
// the handle's allocations, and the few helpers that more than one unit calls.  All of it is defined in plan_core.hip except
// run_impl (plan_run.hip).  Host code only: no kernels and no launches here or in the units that include this.
#pragma once
#include <initializer_list>

#include "dev_guard.h"
#include "launch.h"

namespace tdk {
#pragma GCC visibility push(hidden)  // calls between the host units, not more exports of the library

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
// Every entry point that allocates or launches runs on the handle's device and restores the caller's (DevGuard).
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
// (Out of line, in plan_core.hip: the test-hooks build of that unit gives it a negative control.)
struct StreamTurn {
    tdmpc2_plan *h;
    hipStream_t st;
    bool live;
    hipError_t err;
    StreamTurn(tdmpc2_plan *hh, hipStream_t s);
    ~StreamTurn();
    StreamTurn(const StreamTurn &) = delete;
    StreamTurn &operator=(const StreamTurn &) = delete;
};
#define ENTER_ON(h, stream)                                \
    ENTER(h);                                              \
    StreamTurn turn_((h), (hipStream_t)(stream));          \
    if (turn_.err != hipSuccess) return fail(TDMPC2_ERR_HIP, "hipStreamWaitEvent (stream hand-over of the handle) failed: %s", hipGetErrorString(turn_.err))

// ---- the handle's device memory: everything goes through dev_alloc (freed at destroy; grow_ws releases what it re-grows)
int dev_alloc(tdmpc2_plan *h, void **p, size_t bytes);
// Buffers that share one capacity (`*cap`, in the caller's unit): nothing when want <= *cap; else the stream is drained (earlier
// calls on it are done with the old buffers; first use or a larger call -- outside a hipGraph capture), the old buffers are
// released and the new ones allocated.  *cap is 0 while the set is incomplete.
struct WsBuf {
    void **p;
    size_t bytes;
};
int grow_ws(tdmpc2_plan *h, size_t *cap, size_t want, std::initializer_list<WsBuf> bufs, hipStream_t st);
inline int grow_ws(tdmpc2_plan *h, float **buf, size_t *cap, size_t floats, hipStream_t st) {  // one buffer of floats
    return grow_ws(h, cap, floats, {{(void **)buf, floats * 4}}, st);
}

// ---- the handle's nets
NetS to_dev(const HostNet &n);
HostNet *net_of(tdmpc2_plan *h, int net, int head);
int check_ready(tdmpc2_plan *h);
// the per-padding tables of launch.h by the handle's action padding
const FusedOps &fused_ops(int apad);
const ClusterOps &cluster_ops(int apad);
const ModelOps &model_ops(int apad);
const PolicyLossOps &policy_loss_ops(int apad);

// ---- recovery from a bounded wait that gave up (the state machine is plan_core.hip's)
void apply_modes(tdmpc2_plan *h);
bool fault_poll(tdmpc2_plan *h);
int fault_fresh(tdmpc2_plan *h, hipStream_t st);
int validate_envs(tdmpc2_plan *h, int E);

// ---- a whole plan on a handle that the caller has entered (plan_run.hip; tdmpc2_plan_run, run_obs, run_pix)
int run_impl(tdmpc2_plan *h, int n_envs, const float *z0, const float *task_emb, const float *act_mask, const float *disc_pow,
             float *prev_mean, const uint8_t *t0, int eval_mode, const tdmpc2_noise *tape, uint64_t seed, float *action,
             const tdmpc2_debug *dbg, void *stream);

#pragma GCC visibility pop
}  // namespace tdk
