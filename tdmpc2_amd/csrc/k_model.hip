// Translation unit of the model rollout / loss entry points (tdmpc2_plan_model_rollout / model_losses: the forward half of
// TDMPC2._update, tdmpc2/tdmpc2.py:259-304).  Like k_fused.hip it is compiled once per action padding (-DTU_APAD=16|32|48|64:
// ks_value_roll / ks_value_chain of model_kernels.cuh in both arithmetics, behind the ModelOps table of launch.h) and once
// without TU_APAD: the family-independent row kernels of model_rows.cuh (consistency rows, the fixed-order loss tail, the
// row -> task map).  The layered family's side lives with its GEMMs in k_layered.hip (model_layered.cuh).
#include "launch.h"

#ifdef TU_APAD
namespace {
#include "fused_kernels.cuh"
#include "model_rows.cuh"
#include "model_kernels.cuh"

constexpr int AP = TU_APAD;

void dyn_(int ar, const ModelParams &p, int gx, size_t lds, hipStream_t st) {
    if (ar) hipLaunchKernelGGL((ks_value_roll<AP, 1>), dim3(gx), dim3(NTHREADS), lds, st, p);
    else hipLaunchKernelGGL((ks_value_roll<AP, 0>), dim3(gx), dim3(NTHREADS), lds, st, p);
}
void chain_(int ar, const ModelParams &p, int gx, int gy, int gz, size_t lds, hipStream_t st) {
    if (ar) hipLaunchKernelGGL((ks_value_chain<AP, 1>), dim3(gx, gy, gz), dim3(NTHREADS), lds, st, p);
    else hipLaunchKernelGGL((ks_value_chain<AP, 0>), dim3(gx, gy, gz), dim3(NTHREADS), lds, st, p);
}
int set_lds_(int ar, size_t b) {
    return ar ? (set_lds(ks_value_roll<AP, 1>, b) || set_lds(ks_value_chain<AP, 1>, b))
              : (set_lds(ks_value_roll<AP, 0>, b) || set_lds(ks_value_chain<AP, 0>, b));
}
}  // namespace

#define TDK_CAT_(a, b) a##b
#define TDK_CAT(a, b) TDK_CAT_(a, b)
namespace tdk {
const ModelOps &TDK_CAT(model_ops_ap, TU_APAD)() {
    static const ModelOps ops = {dyn_, chain_, set_lds_};
    return ops;
}
}

#else  // the generic unit

namespace {
#define MODEL_GENERIC_KERNELS
#include "model_rows.cuh"
}  // namespace

namespace tdk {
int model_launch_cons(const ModelConsParams &p, int gx, hipStream_t st) {
    hipLaunchKernelGGL(k_model_cons_rows, dim3(gx), dim3(RW_THREADS), 0, st, p);
    LAUNCH_CHECK();
    return 0;
}
int model_launch_tail(const ModelTailParams &p, hipStream_t st) {
    hipLaunchKernelGGL(k_model_tail, dim3(1), dim3(256), 0, st, p);
    LAUNCH_CHECK();
    return 0;
}
int model_launch_tile_tasks(const int *task_ids, int B, int rows, int rows_p, int *out, hipStream_t st) {
    hipLaunchKernelGGL(k_model_tile_tasks, dim3((rows_p + 255) / 256), dim3(256), 0, st, task_ids, B, rows, rows_p, out);
    LAUNCH_CHECK();
    return 0;
}
}  // namespace tdk
#endif
