/* Task conditioning of a multitask model (tdmpc2_task_*): the embedding lookup with max_norm, the first-layer input
 * [ x | task_emb | a ] of encode / next / reward / Q / pi (reference world_model.py:88-101 and the torch.cat of its callers) and their
 * backward.  A stateless unit beside the planner's ABI (tdmpc2_plan.h, whose version and symbols it leaves as they are), linked into
 * the same libtdmpc2_plan.so: no handle, no allocation, no host synchronisation, no atomics, no wait between workgroups, no
 * environment variable.  A call is its descriptor and its pointers, ordered by `stream`, and can be captured in a hipGraph.
 *
 *   R = steps * batch rows, W = x_dim + task_dim + a_dim columns (D, T, A below).  Every buffer is contiguous.
 *   table   fp32 [num_tasks, T]           ids    ids_len words of id_bytes (4: int32, 8: int64)
 *   x       fp32 [R, D]                   a      fp32 [R, A], NULL iff A == 0
 *   out     fp32 [R, W]                   dout   fp32 [R, W]
 *   dx      fp32 [R, D]                   da     fp32 [R, A]            dtable  fp32 [num_tasks, T]
 * Row r = t * batch + b uses ids[0] (ids_len == 1) or ids[b] (ids_len == batch): a [steps, batch, D] input with one id per batch
 * column, a [batch, D] input with one id, and a [batch, D] input with an id per row (steps = 1).
 *
 * Renorm (max_norm > 0; what F.embedding(max_norm=...) does at every lookup).  Every table row k that some id of the call names is
 * renormalised in place exactly once, before any row is gathered; no other row is written.  With x = table[k, :]:
 *   lane l (0 <= l < 64) forms s_l = 0, then s_l = s_l + x[c] * x[c] for c = l, l + 64, l + 128, ... < T in rising order
 *   (the product and the sum are two fp32 roundings); then the in-place tree s_l = s_l + s_{l + w}, w = 32, 16, .. 1, for l < w;
 *   norm = sqrt(s_0); if norm > max_norm: scale = max_norm / (norm + 1e-7f) and x[c] = x[c] * scale.
 * sqrt, the division and the products are correctly rounded fp32 operations (no contraction), so the same statements in numpy
 * fp32 give the same bits.
 *
 * Forward.  out[r, :] = [ x[r, :D] | table[id(r), :T] | a[r, :A] ].  Two launches when it renorms, one otherwise.
 *
 * Backward.  dx = dout[:, :D] and da = dout[:, D+T:], exact copies.  dtable[k, c] = sum of dout[r, D + c] over the rows r with
 * id(r) == k, and 0 for a task no row names: the whole [num_tasks, T] is written.  The order of the sum is fixed: the rows of task k
 * are listed by rising r and the list is cut into consecutive chunks of TASK_CHUNK = 64 rows (tdmpc2_amd/csrc/task_route.h); a
 * chunk's sum starts at 0 and adds its rows one after the other; the total starts at 0 and adds the chunk sums in chunk order.  All
 * additions are fp32.  One launch: copy workgroups and sum workgroups share the grid.
 *
 * An id outside [0, num_tasks) never leads to an access outside the table: the renorm ignores it, the forward writes NaN into the T
 * embedding columns of its rows, and in the backward its rows add to no table row.
 *
 * tdmpc2_task_renorm is the renorm alone (one launch; nothing happens, and nothing is launched, when max_norm <= 0).
 *
 * Return codes are tdmpc2_plan.h's (the message: tdmpc2_last_error).  TDMPC2_ERR_INVALID before the device is touched: a NULL
 * descriptor or a NULL required pointer; steps, batch, x_dim or task_dim < 1; a_dim < 0; num_tasks < 1; ids_len not 1 or batch;
 * id_bytes not 4 or 8; `a` (forward) or `da` (backward) given with a_dim == 0, `a` absent with a_dim > 0; all three backward outputs
 * NULL.  TDMPC2_ERR_UNSUPPORTED, also before the device is touched: R * W >= 2^62, or a grid of 2^31 workgroups or more. */
#ifndef TDMPC2_TASK_H
#define TDMPC2_TASK_H
#include <stdint.h>

#include "tdmpc2_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tdmpc2_task_desc {
    int32_t  steps;      /* >= 1 */
    int32_t  batch;      /* >= 1; R = steps * batch */
    int32_t  ids_len;    /* 1 or batch */
    int32_t  id_bytes;   /* 4 (int32) or 8 (int64) */
    int32_t  num_tasks;  /* rows of the table, >= 1 */
    int32_t  x_dim;      /* D >= 1 */
    int32_t  task_dim;   /* T >= 1 */
    int32_t  a_dim;      /* A >= 0; 0: no action block */
    float    max_norm;   /* <= 0: the forward does not renorm */
    uint32_t reserved;   /* the tail that rounds the size up to 8 bytes, named; ignored */
} tdmpc2_task_desc;   /* 40 bytes */

int tdmpc2_task_forward(const tdmpc2_task_desc *d, float *table, const void *ids, const float *x, const float *a, float *out,
                        void *stream);
int tdmpc2_task_backward(const tdmpc2_task_desc *d, const void *ids, const float *dout, float *dx, float *da, float *dtable,
                         void *stream);
int tdmpc2_task_renorm(const tdmpc2_task_desc *d, float *table, const void *ids, void *stream);

#ifdef __cplusplus
}
#endif
#endif
