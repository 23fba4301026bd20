/* Dropout masks (tdmpc2_dropout_*): the multipliers of the Q ensemble's first-layer dropout (reference common/layers.py:107-111),
 * drawn on the device from Philox4x32-10.  A stateless unit beside the planner's ABI (tdmpc2_plan.h, whose version and symbols it
 * leaves as they are), linked into the same libtdmpc2_plan.so: no handle, no allocation, no host synchronisation, no atomics, no
 * wait between workgroups, no environment variable.  A call is its descriptor and its pointers, ordered by `stream`, and can be
 * captured in a hipGraph.  The mask is what tdmpc2_layer_forward / tdmpc2_layer_backward take as `mask` [G, R, N].
 *
 *   mask    n fp32 elements, flat; the caller gives them meaning.  16-byte aligned.
 *   state   NULL, or two device words (lo, hi) holding the call counter.
 *
 * Element e (0 <= e < n) belongs to quad q = e >> 2, lane j = e & 3.  The quad's four words are
 *   philox4x32_10(counter = (q_lo, q_hi, call_lo, call_hi), key = (seed_lo, seed_hi)),
 * and the element is dropped iff word_j < thr, thr = (uint32_t)floor((double)p * 2^32), computed once on the host: P(drop) is
 * exactly thr / 2^32.  A dropped element is written as +0.0f, a kept one as keep = 1.0f / (float)(1.0 - (double)p), the value
 * torch.nn.functional.dropout gives kept elements.  p == 0: thr = 0, every element is exactly 1.0f.
 *
 * The counter.  state == NULL: the call counter is the descriptor's (call_lo, call_hi); one launch.  state != NULL: the mask
 * kernel reads the counter from state (the descriptor's is ignored), and a second, one-thread launch in the same stream then adds
 * 1 with carry: two launches, and a captured call draws a fresh mask on every replay.  No workgroup of the first launch writes
 * state.
 *
 * Launch shape: one thread per quad, one 16-byte store per full quad, single-element stores for the last partial quad, a
 * grid-stride loop under a workgroup cap (tdmpc2_amd/csrc/dropout_route.h: drop_grid), so no grid passes 2^31.
 *
 * Return codes are tdmpc2_plan.h's (the message: tdmpc2_last_error).  TDMPC2_ERR_INVALID before the device is touched: NULL
 * descriptor or mask; n < 1; p NaN, < 0 or >= 1; a mask that is not 16-byte aligned.  TDMPC2_ERR_UNSUPPORTED, also before the device
 * is touched: n >= 2^62. */
#ifndef TDMPC2_DROPOUT_H
#define TDMPC2_DROPOUT_H
#include <stdint.h>

#include "tdmpc2_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tdmpc2_dropout_desc {
    int64_t  n;                  /* elements of the mask, flat */
    float    p;                  /* drop probability, 0 <= p < 1 */
    uint32_t seed_lo, seed_hi;   /* Philox key */
    uint32_t call_lo, call_hi;   /* call counter, used only when `state` is NULL */
    uint32_t reserved;           /* the tail padding of the 8-byte alignment, named; ignored */
} tdmpc2_dropout_desc;   /* 32 bytes */

int tdmpc2_dropout_mask(const tdmpc2_dropout_desc *d, uint32_t *state, float *mask, void *stream);

#ifdef __cplusplus
}
#endif
#endif
