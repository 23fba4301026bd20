// Translation unit of the pixel encoder's batch route (tdmpc2_plan_encode_pix_batch): the MFMA kernels of
// pixel_batch_kernels.cuh behind pixb_launch of launch.h.  The host side (checks, passes, the C ABI) is in plan_obs.hip.
#include "launch.h"

namespace {
#include "pixel_batch_kernels.cuh"
}  // namespace

int tdk::pixb_set_lds(size_t bytes) {
    if (int rc = set_lds(k_pixb<0, true>, bytes)) return rc;
    return set_lds(k_pixb<0, false>, bytes);
}

int tdk::pixb_launch(int layer, bool obs_u8, const PixbParams &p, const PixGrid &g, hipStream_t st) {
    const dim3 grid(g.x, g.y, g.z), block(g.threads);
    switch (layer) {
        case 0:
            if (obs_u8) hipLaunchKernelGGL((k_pixb<0, true>), grid, block, g.lds, st, p);
            else hipLaunchKernelGGL((k_pixb<0, false>), grid, block, g.lds, st, p);
            break;
        case 1: hipLaunchKernelGGL((k_pixb<1, false>), grid, block, g.lds, st, p); break;
        case 2: hipLaunchKernelGGL((k_pixb<2, false>), grid, block, g.lds, st, p); break;
        case 3: hipLaunchKernelGGL((k_pixb<3, false>), grid, block, g.lds, st, p); break;
        default: return fail(TDMPC2_ERR_INVALID, "pixel encoder batch route: layer %d", layer);
    }
    LAUNCH_CHECK();
    return 0;
}
