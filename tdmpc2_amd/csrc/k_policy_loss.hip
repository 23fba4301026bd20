// Translation unit of tdmpc2_plan_policy_loss / running_scale / termination_stats (TDMPC2.update_pi's forward, tdmpc2/tdmpc2.py:208-239).
// Like k_model.hip it is compiled once per action padding (-DTU_APAD=16|32|48|64: ks_value_ent of policy_loss_fused.cuh -- ks_value with
// the policy head's entropy terms -- in both arithmetics) and once without TU_APAD: the one-workgroup kernels of
// policy_loss_kernels.cuh (running scale, loss tail, termination statistics).
#include "launch.h"

#ifdef TU_APAD
namespace {
#include "fused_kernels.cuh"
#include "policy_loss_fused.cuh"

constexpr int AP = TU_APAD;

void value_ent_(int ar, const ValueEntParams &p, int grid, size_t lds, hipStream_t st) {
    if (ar) hipLaunchKernelGGL((ks_value_ent<AP, 1>), dim3(grid), dim3(NTHREADS), lds, st, p);
    else hipLaunchKernelGGL((ks_value_ent<AP, 0>), dim3(grid), dim3(NTHREADS), lds, st, p);
}
int set_lds_(int ar, size_t b) { return ar ? set_lds(ks_value_ent<AP, 1>, b) : set_lds(ks_value_ent<AP, 0>, b); }
}  // namespace

#define TDK_CAT_(a, b) a##b
#define TDK_CAT(a, b) TDK_CAT_(a, b)
namespace tdk {
const PolicyLossOps &TDK_CAT(policy_loss_ops_ap, TU_APAD)() {
    static const PolicyLossOps ops = {value_ent_, set_lds_};
    return ops;
}
}

#else  // the generic unit

namespace {
#include "policy_loss_kernels.cuh"
}  // namespace

namespace tdk {
int pl_set_lds() {  // the key array of k_running_scale: up to 64 KB of dynamic LDS (once per handle, on its device, at creation)
    return set_lds(k_running_scale, (size_t)PL_SCALE_MAX_N * 4);
}
int pl_launch_scale(const RunningScaleParams &p, hipStream_t st) {
    hipLaunchKernelGGL(k_running_scale, dim3(1), dim3(PL_THREADS), (size_t)p.n * 4, st, p);
    LAUNCH_CHECK();
    return 0;
}
int pl_launch_tail(const PolicyLossTailParams &p, hipStream_t st) {
    hipLaunchKernelGGL(k_policy_loss_tail, dim3(1), dim3(256), 0, st, p);
    LAUNCH_CHECK();
    return 0;
}
int pl_launch_term_stats(const TerminationStatsParams &p, hipStream_t st) {
    hipLaunchKernelGGL(k_termination_stats, dim3(1), dim3(256), 0, st, p);
    LAUNCH_CHECK();
    return 0;
}
}  // namespace tdk
#endif
