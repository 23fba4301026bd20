// Translation unit of the optimiser step (tdmpc2_optim_*): the kernels of optim_kernels.cuh and the whole host side of the handle.
// It shares nothing with a planner handle: the re-pack of the planner's weights stays tdmpc2_plan_refresh_weights, issued after
// the step.  Every decision (layout, chunks, the order of the norm, grids, the device block) is optim_route.h's; this file checks
// arguments, then launches.  A step allocates nothing, copies nothing from the host and never synchronises: it can be captured.
#include "launch.h"  // handle.h + grid_fits
#include "dev_guard.h"
#include "optim_route.h"

namespace {
using namespace tdk;
#include "optim_kernels.cuh"

static_assert(sizeof(OptSeg) == 32 && sizeof(OptState) == 40, "device records of optim_route.h");

// the refusals of layout and create, in one place: nothing here touches a device
int opt_validate(const tdmpc2_optim_cfg *cfg, const char *what) {
    if (!cfg) return fail(TDMPC2_ERR_INVALID, "%s: null cfg", what);
    if (cfg->n_segs < 1 || cfg->n_groups < 1)
        return fail(TDMPC2_ERR_INVALID, "%s: n_segs %d, n_groups %d: each must be at least 1", what, cfg->n_segs, cfg->n_groups);
    if (!cfg->lr || !cfg->segs) return fail(TDMPC2_ERR_INVALID, "%s: null lr or segs", what);
    if (opt_check_hyper(cfg->beta1, cfg->beta2, cfg->eps, cfg->max_norm))
        return fail(TDMPC2_ERR_INVALID, "%s: beta1 %g, beta2 %g must lie in [0, 1), eps %g and max_norm %g must be positive (and none NaN)",
                    what, (double)cfg->beta1, (double)cfg->beta2, (double)cfg->eps, (double)cfg->max_norm);
    for (int32_t i = 0; i < cfg->n_segs; ++i) {
        const tdmpc2_optim_seg &s = cfg->segs[i];
        switch (opt_check_seg(s.count, s.group, cfg->n_groups, s.param)) {
        case OPT_OK: break;
        case OPT_BAD_SEG: return fail(TDMPC2_ERR_INVALID, "%s: segment %d has count %lld (at least 1, at most 2^48)", what, i, (long long)s.count);
        case OPT_BAD_GROUP: return fail(TDMPC2_ERR_INVALID, "%s: segment %d names group %d of %d", what, i, s.group, cfg->n_groups);
        default: return fail(TDMPC2_ERR_INVALID, "%s: segment %d has a null param pointer", what, i);
        }
    }
    return 0;
}

uint64_t opt_arena(const tdmpc2_optim_cfg *cfg, int64_t *offsets) {
    return opt_layout(cfg->n_segs, &cfg->segs[0].count, sizeof(tdmpc2_optim_seg), offsets);
}
}  // namespace

struct tdmpc2_optim {
    int device = 0;
    int32_t n_groups = 0;
    uint64_t arena_floats = 0, chunks = 0;
    OptHyper hyper{};
    double beta1 = 0, beta2 = 0;
    OptBlock lay{};
    unsigned char *dev = nullptr;  // the one allocation (optim_route.h: opt_block)
    OptState staged{};             // host source of set_step's copy
};

extern "C" {

int tdmpc2_optim_layout(const tdmpc2_optim_cfg *cfg, int64_t *offsets, int64_t *arena_floats) {
    if (int rc = opt_validate(cfg, "optim_layout")) return rc;
    if (!offsets || !arena_floats) return fail(TDMPC2_ERR_INVALID, "optim_layout: null offsets or arena_floats");
    *arena_floats = (int64_t)opt_arena(cfg, offsets);
    return 0;
}

int tdmpc2_optim_create(const tdmpc2_optim_cfg *cfg, tdmpc2_optim_t **out) {
    if (!out) return fail(TDMPC2_ERR_INVALID, "optim_create: null out");
    *out = nullptr;
    if (int rc = opt_validate(cfg, "optim_create")) return rc;
    const uint64_t arena = opt_arena(cfg, nullptr), chunks = opt_chunks(arena);
    if (int rc = grid_fits(chunks, "optim_create")) return rc;
    tdmpc2_optim *o = new (std::nothrow) tdmpc2_optim();
    if (!o) return fail(TDMPC2_ERR_HIP, "optim_create: out of host memory");
    o->device = cfg->device;
    o->n_groups = cfg->n_groups;
    o->arena_floats = arena;
    o->chunks = chunks;
    o->beta1 = (double)cfg->beta1;
    o->beta2 = (double)cfg->beta2;
    o->hyper = OptHyper{cfg->beta1, cfg->beta2, cfg->eps, cfg->max_norm, (float)(1.0 - o->beta1), (float)(1.0 - o->beta2)};
    o->lay = opt_block((uint64_t)cfg->n_segs, (uint64_t)cfg->n_groups, chunks);
    // host image of everything in front of the partials: segment records, chunk_seg, lr, the scalars of step 0
    std::vector<unsigned char> img;
    try {
        img.assign(o->lay.partial_off, 0);
    } catch (...) {
        delete o;
        return fail(TDMPC2_ERR_HIP, "optim_create: out of host memory for the segment table");
    }
    OptSeg *segs = (OptSeg *)(img.data() + o->lay.segs_off);
    uint64_t at = 0;
    for (int32_t i = 0; i < cfg->n_segs; ++i) {
        segs[i] = OptSeg{cfg->segs[i].param, at / OPT_QUAD, (uint64_t)cfg->segs[i].count, cfg->segs[i].group, 0};
        at += opt_pad((uint64_t)cfg->segs[i].count);
    }
    int32_t *chunk_seg = (int32_t *)(img.data() + o->lay.chunk_seg_off);
    int32_t s = 0;
    for (uint64_t c = 0; c < chunks; ++c) {
        s = opt_seg_of_quad(&segs[0].quad0, sizeof(OptSeg), s, cfg->n_segs - 1, c * OPT_CHUNK_QUADS);
        chunk_seg[c] = s;
    }
    chunk_seg[chunks] = cfg->n_segs - 1;
    memcpy(img.data() + o->lay.lr_off, cfg->lr, (size_t)cfg->n_groups * sizeof(float));
    OptState st{};
    st.b1p = st.b2p = 1.0;
    memcpy(img.data() + o->lay.state_off, &st, sizeof st);

    DevGuard dg(o->device);
    if (!dg.ok) {
        delete o;
        return fail(TDMPC2_ERR_HIP, "optim_create: cannot select device %d", cfg->device);
    }
    hipError_t e = hipMalloc((void **)&o->dev, o->lay.bytes);
    if (e == hipSuccess) e = hipMemcpy(o->dev, img.data(), img.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (o->dev) (void)hipFree(o->dev);
        (void)hipGetLastError();
        delete o;
        return fail(TDMPC2_ERR_HIP, "optim_create: %llu bytes of device memory: %s", (unsigned long long)o->lay.bytes, hipGetErrorString(e));
    }
    *out = o;
    return 0;
}

void tdmpc2_optim_destroy(tdmpc2_optim_t *o) {
    if (!o) return;
    {
        DevGuard dg(o->device);
        if (o->dev) (void)hipFree(o->dev);
    }
    delete o;
}

int tdmpc2_optim_step(tdmpc2_optim_t *o, float *grad, float *exp_avg, float *exp_avg_sq, int zero_grad, float *norm_out, void *stream) {
    if (!o) return fail(TDMPC2_ERR_INVALID, "optim_step: null handle");
    if (!grad || !exp_avg || !exp_avg_sq) return fail(TDMPC2_ERR_INVALID, "optim_step: null arena (grad, exp_avg, exp_avg_sq)");
    DevGuard dg(o->device);
    if (!dg.ok) return fail(TDMPC2_ERR_HIP, "optim_step: cannot select device %d", o->device);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((uint32_t)o->chunks), block(OPT_THREADS);
    OptState *state = (OptState *)(o->dev + o->lay.state_off);
    float *partial = (float *)(o->dev + o->lay.partial_off), *ss = (float *)(o->dev + o->lay.ss_off);

    OptNormParams np{};
    np.grad = grad; np.partial = partial; np.arena_quads = o->arena_floats / OPT_QUAD;
    hipLaunchKernelGGL(k_opt_norm, grid, block, 0, st, np);
    LAUNCH_CHECK();

    OptTotalParams tp{};
    tp.partial = partial; tp.chunks = o->chunks; tp.state = state; tp.ss = ss;
    tp.lr = (const float *)(o->dev + o->lay.lr_off); tp.n_groups = o->n_groups; tp.h = o->hyper; tp.norm_out = norm_out;
    hipLaunchKernelGGL(k_opt_total, dim3(1), block, 0, st, tp);
    LAUNCH_CHECK();

    OptUpdateParams up{};
    up.grad = grad; up.exp_avg = exp_avg; up.exp_avg_sq = exp_avg_sq;
    up.segs = (const OptSeg *)(o->dev + o->lay.segs_off); up.chunk_seg = (const int32_t *)(o->dev + o->lay.chunk_seg_off);
    up.state = state; up.ss = ss; up.arena_quads = np.arena_quads; up.h = o->hyper; up.zero_grad = zero_grad != 0;
    hipLaunchKernelGGL(k_opt_update, grid, block, 0, st, up);
    LAUNCH_CHECK();
    return 0;
}

int tdmpc2_optim_get_step(tdmpc2_optim_t *o, int64_t *step, void *stream) {
    if (!o || !step) return fail(TDMPC2_ERR_INVALID, "optim_get_step: null argument");
    DevGuard dg(o->device);
    if (!dg.ok) return fail(TDMPC2_ERR_HIP, "optim_get_step: cannot select device %d", o->device);
    OptState s{};
    HIP_TRY(hipMemcpyAsync(&s, o->dev + o->lay.state_off, sizeof s, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    *step = s.step;
    return 0;
}

int tdmpc2_optim_set_step(tdmpc2_optim_t *o, int64_t step, void *stream) {
    if (!o) return fail(TDMPC2_ERR_INVALID, "optim_set_step: null handle");
    if (step < 0) return fail(TDMPC2_ERR_INVALID, "optim_set_step: step %lld < 0", (long long)step);
    DevGuard dg(o->device);
    if (!dg.ok) return fail(TDMPC2_ERR_HIP, "optim_set_step: cannot select device %d", o->device);
    // the products a run of `step` steps would have made on the device: IEEE fp64 multiplications in the same order
    OptState &s = o->staged;
    s = OptState{};
    s.step = step;
    s.b1p = s.b2p = 1.0;
    for (int64_t k = 0; k < step; ++k) {
        s.b1p *= o->beta1;
        s.b2p *= o->beta2;
    }
    HIP_TRY(hipMemcpyAsync(o->dev + o->lay.state_off, &s, sizeof s, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

}  // extern "C"
