// Translation unit of the draw unit (tdmpc2_draw_noise, include/tdmpc2_draw.h): the kernels of draw_kernels.cuh and their host side.
// It shares nothing with a planner handle and keeps no state of its own: a call is its descriptor and its pointers.  Every decision
// (the refusals, the grid, the decode, the pair) is draw_route.h's; this file checks arguments, then launches.  Nothing is allocated,
// nothing synchronises the host: the call can be captured in a hipGraph.
#include "../../include/tdmpc2_draw.h"
#include "launch.h"
#include "draw_route.h"

namespace {
using namespace tdk;
#include "draw_kernels.cuh"

static_assert(sizeof(DrawDesc) == sizeof(tdmpc2_draw_desc) && sizeof(DrawDesc) == 32, "tdmpc2_draw_desc is 32 bytes");
static_assert(DRAW_MAXQ == MAXQ, "the pair is drawn from at most MAXQ heads");
}  // namespace

extern "C" {

int tdmpc2_draw_noise(const tdmpc2_draw_desc *desc, uint32_t *state, float *normal, int32_t *pair, void *stream) {
    if (!desc) return fail(TDMPC2_ERR_INVALID, "draw_noise: null descriptor");
    const DrawDesc d{desc->n, desc->num_q, desc->seed_lo, desc->seed_hi, desc->call_lo, desc->call_hi, 0u};
    switch (draw_check(d, normal != nullptr, pair != nullptr, (uint64_t)(uintptr_t)normal)) {
    case DRAW_OK: break;
    case DRAW_NO_OUTPUT: return fail(TDMPC2_ERR_INVALID, "draw_noise: both outputs are null");
    case DRAW_NEG_N: return fail(TDMPC2_ERR_INVALID, "draw_noise: n %lld is negative", (long long)d.n);
    case DRAW_ZERO_N: return fail(TDMPC2_ERR_INVALID, "draw_noise: n 0 with a normal buffer: pass a null normal to draw the pair alone");
    case DRAW_NULL_NORMAL: return fail(TDMPC2_ERR_INVALID, "draw_noise: null normal with n %lld", (long long)d.n);
    case DRAW_MISALIGNED: return fail(TDMPC2_ERR_INVALID, "draw_noise: normal %p is not 16-byte aligned", (void *)normal);
    case DRAW_BAD_Q: return fail(TDMPC2_ERR_INVALID, "draw_noise: num_q %d outside [2, %d]", (int)d.num_q, (int)DRAW_MAXQ);
    default: return fail(TDMPC2_ERR_UNSUPPORTED, "draw_noise: n %lld: 2^62 elements or more", (long long)d.n);
    }
    DrawParams p{};
    p.n = (uint64_t)d.n;
    p.num_q = d.num_q;
    p.seed_lo = d.seed_lo; p.seed_hi = d.seed_hi; p.call_lo = d.call_lo; p.call_hi = d.call_hi;
    p.state = state;
    p.normal = normal;
    p.pair = pair;
    hipLaunchKernelGGL(k_draw, dim3((uint32_t)draw_grid(p.n)), dim3(DRAW_THREADS), 0, (hipStream_t)stream, p);
    LAUNCH_CHECK();
    if (state) {
        hipLaunchKernelGGL(k_draw_bump, dim3(1), dim3(64), 0, (hipStream_t)stream, state);
        LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
