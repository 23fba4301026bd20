// Translation unit of the weight packer (tdmpc2_plan_bind_weights / bind_encoder / bind_policy / refresh_weights /
// soft_update_target): the kernels of refresh_kernels.cuh behind refresh_launch of launch.h.  The host side (job checks, job
// table, the C ABI) is in plan_weights.hip.
#include "launch.h"

namespace {
#include "refresh_kernels.cuh"
}  // namespace

int tdk::refresh_launch(int op, const RfParams &p, hipStream_t st) {
    switch (op) {
        case RO_RESET: hipLaunchKernelGGL(k_rf_reset, dim3(1), dim3(RF_THREADS), 0, st, p); break;
        case RO_SCAN: hipLaunchKernelGGL(k_rf_scan, dim3(p.scan_blk0[3 * RF_NETS]), dim3(RF_THREADS), 0, st, p); break;
        case RO_SCALES: hipLaunchKernelGGL(k_rf_scales, dim3(1), dim3(RF_THREADS), 0, st, p); break;
        case RO_PACK: hipLaunchKernelGGL(k_rf_pack, dim3(p.pack_blk0[RF_SEGS]), dim3(RF_THREADS), 0, st, p); break;
        default: return fail(TDMPC2_ERR_INVALID, "weight refresh: unknown operation %d", op);
    }
    LAUNCH_CHECK();
    return 0;
}
