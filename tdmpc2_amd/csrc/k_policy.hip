// Translation unit of the policy prior (WorldModel.pi and act() with mpc = False): the row-route, GEMV and head kernels of
// policy_kernels.cuh behind the pol_* launchers of launch.h.  The host side is in plan_obs.hip (routes, the C ABI) and
// plan_weights.hip (bind).
#include "launch.h"

namespace {
#include "policy_kernels.cuh"
}  // namespace

int tdk::pol_set_lds() {
    if (int rc = set_lds(k_pol_gemv<1>, POL_LDS_MAX)) return rc;
    if (int rc = set_lds(k_pol_gemv<2>, POL_LDS_MAX)) return rc;
    if (int rc = set_lds(k_pol_gemv<4>, POL_LDS_MAX)) return rc;
    return set_lds(k_pol_gemv<8>, POL_LDS_MAX);
}

int tdk::pol_launch_row(const PolRowParams &p, const PolGrid &g, hipStream_t st) {
    hipLaunchKernelGGL(k_pol_row, dim3(g.x), dim3(g.threads), g.lds, st, p);
    LAUNCH_CHECK();
    return 0;
}

int tdk::pol_launch_gemv(const PolGemvParams &p, const PolGrid &g, hipStream_t st) {
    const dim3 grid(g.x, g.y), block(g.threads);
    switch (g.R) {
        case 1: hipLaunchKernelGGL(k_pol_gemv<1>, grid, block, g.lds, st, p); break;
        case 2: hipLaunchKernelGGL(k_pol_gemv<2>, grid, block, g.lds, st, p); break;
        case 4: hipLaunchKernelGGL(k_pol_gemv<4>, grid, block, g.lds, st, p); break;
        case 8: hipLaunchKernelGGL(k_pol_gemv<8>, grid, block, g.lds, st, p); break;
        default: return fail(TDMPC2_ERR_INVALID, "policy GEMV: %d rows per workgroup is not built", g.R);
    }
    LAUNCH_CHECK();
    return 0;
}

int tdk::pol_launch_head(const PolHeadParams &p, const PolGrid &g, hipStream_t st) {
    hipLaunchKernelGGL(k_pol_head, dim3(g.x), dim3(g.threads), 0, st, p);
    LAUNCH_CHECK();
    return 0;
}
