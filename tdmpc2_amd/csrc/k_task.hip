// Translation unit of the task unit (tdmpc2_task_*, include/tdmpc2_task.h): the kernels of task_kernels.cuh and their host side.
// It shares nothing with a planner handle and keeps no state of its own: a call is its descriptor and its pointers.  Every decision
// (the refusals, the grids, the path) is task_route.h's; this file checks arguments, then launches.  Nothing is allocated, nothing
// synchronises the host: the calls can be captured in a hipGraph.
#include <initializer_list>

#include "../../include/tdmpc2_task.h"
#include "launch.h"
#include "task_route.h"

namespace {
using namespace tdk;
#include "task_kernels.cuh"

static_assert(sizeof(TaskDesc) == sizeof(tdmpc2_task_desc) && sizeof(TaskDesc) == 40, "tdmpc2_task_desc is 40 bytes");

TaskDesc desc_of(const tdmpc2_task_desc *s) {
    return TaskDesc{s->steps, s->batch, s->ids_len, s->id_bytes, s->num_tasks, s->x_dim, s->task_dim, s->a_dim, s->max_norm, 0u};
}

// the message of a refusal of task_check
int refuse(const char *what, int why, const TaskDesc &d) {
    switch (why) {
    case TASK_BAD_STEPS: return fail(TDMPC2_ERR_INVALID, "%s: steps %d < 1", what, (int)d.steps);
    case TASK_BAD_BATCH: return fail(TDMPC2_ERR_INVALID, "%s: batch %d < 1", what, (int)d.batch);
    case TASK_BAD_X: return fail(TDMPC2_ERR_INVALID, "%s: x_dim %d < 1", what, (int)d.x_dim);
    case TASK_BAD_T: return fail(TDMPC2_ERR_INVALID, "%s: task_dim %d < 1", what, (int)d.task_dim);
    case TASK_BAD_A: return fail(TDMPC2_ERR_INVALID, "%s: a_dim %d is negative", what, (int)d.a_dim);
    case TASK_BAD_TASKS: return fail(TDMPC2_ERR_INVALID, "%s: num_tasks %d < 1", what, (int)d.num_tasks);
    case TASK_BAD_IDS_LEN: return fail(TDMPC2_ERR_INVALID, "%s: ids_len %d is neither 1 nor batch %d", what, (int)d.ids_len, (int)d.batch);
    case TASK_BAD_ID_BYTES: return fail(TDMPC2_ERR_INVALID, "%s: id_bytes %d is neither 4 nor 8", what, (int)d.id_bytes);
    case TASK_NULL_PTR: return fail(TDMPC2_ERR_INVALID, "%s: a required pointer is null", what);
    case TASK_A_GIVEN: return fail(TDMPC2_ERR_INVALID, "%s: an action pointer with a_dim 0", what);
    case TASK_A_ABSENT: return fail(TDMPC2_ERR_INVALID, "%s: null a with a_dim %d", what, (int)d.a_dim);
    case TASK_NO_OUTPUT: return fail(TDMPC2_ERR_INVALID, "%s: all three outputs are null", what);
    case TASK_HUGE: return fail(TDMPC2_ERR_UNSUPPORTED, "%s: %llu rows of %llu columns: 2^62 elements or more", what,
                                (unsigned long long)task_rows(d), (unsigned long long)task_width(d));
    default: return fail(TDMPC2_ERR_UNSUPPORTED, "%s: more than 2^31 workgroups in one launch", what);
    }
}

bool aligned16(std::initializer_list<const void *> ptrs) {
    uintptr_t all = 0;
    for (const void *q : ptrs) all |= (uintptr_t)q;
    return (all & 15u) == 0;
}

int launch_renorm(const TaskDesc &d, float *table, const void *ids, hipStream_t st) {
    TaskParams p{};
    p.d = d;
    p.table = table;
    p.ids = ids;
    hipLaunchKernelGGL(k_task_renorm, dim3((uint32_t)task_renorm_grid(d)), dim3(TASK_THREADS), 0, st, p);
    LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" {

int tdmpc2_task_renorm(const tdmpc2_task_desc *desc, float *table, const void *ids, void *stream) {
    if (!desc) return fail(TDMPC2_ERR_INVALID, "task_renorm: null descriptor");
    const TaskDesc d = desc_of(desc);
    const int why = task_check(d, TASK_RENORM, (table ? TASK_HAS_TABLE : 0) | (ids ? TASK_HAS_IDS : 0));
    if (why) return refuse("task_renorm", why, d);
    if (!(d.max_norm > 0.0f)) return 0;
    return launch_renorm(d, table, ids, (hipStream_t)stream);
}

int tdmpc2_task_forward(const tdmpc2_task_desc *desc, float *table, const void *ids, const float *x, const float *a, float *out,
                        void *stream) {
    if (!desc) return fail(TDMPC2_ERR_INVALID, "task_forward: null descriptor");
    const TaskDesc d = desc_of(desc);
    const int why = task_check(d, TASK_FORWARD, (table ? TASK_HAS_TABLE : 0) | (ids ? TASK_HAS_IDS : 0) | (x ? TASK_HAS_X : 0) |
                                                    (a ? TASK_HAS_A : 0) | (out ? TASK_HAS_OUT : 0));
    if (why) return refuse("task_forward", why, d);
    if (d.max_norm > 0.0f) {  // a row is final before any workgroup gathers it: a launch of its own
        const int rc = launch_renorm(d, table, ids, (hipStream_t)stream);
        if (rc) return rc;
    }
    TaskParams p{};
    p.d = d;
    p.vec = task_vec(d, aligned16({table, x, a, out})) ? 1 : 0;
    p.table = table;
    p.ids = ids;
    p.x = x;
    p.a = a;
    p.out = out;
    hipLaunchKernelGGL(k_task_gather, dim3((uint32_t)task_gather_grid(d)), dim3(TASK_THREADS), 0, (hipStream_t)stream, p);
    LAUNCH_CHECK();
    return 0;
}

int tdmpc2_task_backward(const tdmpc2_task_desc *desc, const void *ids, const float *dout, float *dx, float *da, float *dtable,
                         void *stream) {
    if (!desc) return fail(TDMPC2_ERR_INVALID, "task_backward: null descriptor");
    const TaskDesc d = desc_of(desc);
    const int why = task_check(d, TASK_BACKWARD, (ids ? TASK_HAS_IDS : 0) | (dout ? TASK_HAS_DOUT : 0) | (dx ? TASK_HAS_DX : 0) |
                                                     (da ? TASK_HAS_DA : 0) | (dtable ? TASK_HAS_DTABLE : 0));
    if (why) return refuse("task_backward", why, d);
    TaskParams p{};
    p.d = d;
    p.vec = task_vec(d, aligned16({dout, dx, da})) ? 1 : 0;
    p.staged = task_staged(d) ? 1 : 0;
    p.grid = task_backward_grid(d, dx || da, dtable != nullptr);
    p.ids = ids;
    p.dout = dout;
    p.dx = dx;
    p.da = da;
    p.dtable = dtable;
    hipLaunchKernelGGL(k_task_backward, dim3((uint32_t)p.grid.first[2]), dim3(TASK_THREADS), 0, (hipStream_t)stream, p);
    LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
