// Translation unit of the dropout-mask unit (tdmpc2_dropout_mask, include/tdmpc2_dropout.h): the kernels of dropout_kernels.cuh and
// their host side.  It shares nothing with a planner handle and keeps no state of its own: a call is its descriptor and its
// pointers.  Every decision (threshold, kept value, grid, decode, refusals on the descriptor) is dropout_route.h's; this file
// checks arguments, then launches.  Nothing is allocated, nothing synchronises the host: the call can be captured in a hipGraph.
#include "../../include/tdmpc2_dropout.h"
#include "launch.h"
#include "dropout_route.h"

namespace {
using namespace tdk;
#include "dropout_kernels.cuh"

static_assert(sizeof(DropDesc) == sizeof(tdmpc2_dropout_desc) && sizeof(DropDesc) == 32, "tdmpc2_dropout_desc is 32 bytes");
}  // namespace

extern "C" {

int tdmpc2_dropout_mask(const tdmpc2_dropout_desc *desc, uint32_t *state, float *mask, void *stream) {
    if (!desc) return fail(TDMPC2_ERR_INVALID, "dropout_mask: null descriptor");
    const DropDesc d{desc->n, desc->p, desc->seed_lo, desc->seed_hi, desc->call_lo, desc->call_hi, 0u};
    switch (drop_check(d)) {
    case DROP_OK: break;
    case DROP_BAD_N: return fail(TDMPC2_ERR_INVALID, "dropout_mask: n %lld: must be at least 1", (long long)d.n);
    case DROP_BAD_P: return fail(TDMPC2_ERR_INVALID, "dropout_mask: p %g outside [0, 1)", (double)d.p);
    default: return fail(TDMPC2_ERR_UNSUPPORTED, "dropout_mask: n %lld: 2^62 elements or more", (long long)d.n);
    }
    if (!mask) return fail(TDMPC2_ERR_INVALID, "dropout_mask: null mask");
    if ((uintptr_t)mask & 15u) return fail(TDMPC2_ERR_INVALID, "dropout_mask: mask %p is not 16-byte aligned", (void *)mask);
    DropParams p{};
    p.n = (uint64_t)d.n;
    p.thr = drop_thr(d.p);
    p.keep = drop_keep(d.p);
    p.seed_lo = d.seed_lo; p.seed_hi = d.seed_hi; p.call_lo = d.call_lo; p.call_hi = d.call_hi;
    p.state = state;
    p.mask = mask;
    hipLaunchKernelGGL(k_drop_mask, dim3((uint32_t)drop_grid(p.n)), dim3(DROP_THREADS), 0, (hipStream_t)stream, p);
    LAUNCH_CHECK();
    if (state) {
        hipLaunchKernelGGL(k_drop_bump, dim3(1), dim3(64), 0, (hipStream_t)stream, state);
        LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
