/* Draws of a training step (tdmpc2_draw_*): standard normals (the policy noise of the TD target and of update_pi, reference
 * tdmpc2.py:208-254) and an ordered pair of distinct Q heads (reference world_model.py:212, torch.randperm(num_q)[:2]), drawn on the
 * device from Philox4x32-10.  A stateless unit beside the planner's ABI (tdmpc2_plan.h, whose version and symbols it leaves as they
 * are), linked into the same libtdmpc2_plan.so: no handle, no allocation, no host synchronisation, no atomics, no wait between
 * workgroups, no environment variable.  A call is its descriptor and its pointers, ordered by `stream`, and can be captured in a
 * hipGraph.
 *
 *   normal  n fp32 elements, flat; the caller gives them meaning.  16-byte aligned.  NULL iff n == 0.
 *   pair    NULL, or two int32 words: (i, j), i != j, both in [0, num_q).
 *   state   NULL, or two device words (lo, hi) holding the call counter.
 *
 * Normals.  Element e (0 <= e < n) belongs to quad q = e >> 2, lane j = e & 3.  The quad's four words are
 *   w = philox4x32_10(counter = (q_lo, q_hi, call_lo, call_hi), key = (seed_lo, seed_hi)).
 * u(x) is the fp32 value of ((float)(x >> 8) + 0.5f) * 2^-24, in (0, 1].  Lanes 0 / 1 are r cos(2 pi u(w1)) / r sin(2 pi u(w1)) with
 * r = sqrt(-2 ln u(w0)); lanes 2 / 3 are the same from (w2, w3).  The kernel evaluates this with the precise fp32 logf, sqrtf and
 * sincospif; against the same expression in fp64 on the same fp32 uniforms it stays within 8 * 2^-24 * max(|x|, 1).
 *
 * Pair.  w = philox4x32_10((0xFFFFFFFF, 0xFFFFFFFF, call_lo, call_hi), key), a counter no quad reaches (n < 2^62);
 * i = (uint64(w0) * num_q) >> 32, k = (uint64(w1) * (num_q - 1)) >> 32, j = k + (k >= i): pure integer arithmetic, uniform over the
 * ordered pairs up to num_q / 2^32.
 *
 * The counter.  state == NULL: the call counter is the descriptor's (call_lo, call_hi); one launch.  state != NULL: the kernel reads
 * the counter from state (the descriptor's is ignored), and a second, one-thread launch in the same stream then adds 1 with carry:
 * two launches, and a captured call draws afresh on every replay.  No workgroup of the first launch writes state.
 *
 * Launch shape: one thread per quad, one 16-byte store per full quad, single-element stores for the last partial quad, a
 * grid-stride loop under a workgroup cap (tdmpc2_amd/csrc/draw_route.h: draw_grid); thread 0 of workgroup 0 writes the pair.
 *
 * Return codes are tdmpc2_plan.h's (the message: tdmpc2_last_error).  TDMPC2_ERR_INVALID before the device is touched: NULL
 * descriptor; both outputs NULL; n < 0; n == 0 with a normal buffer; n > 0 without one; a normal buffer that is not 16-byte aligned;
 * a pair with num_q < 2 or num_q > 8.  TDMPC2_ERR_UNSUPPORTED, also before the device is touched: n >= 2^62. */
#ifndef TDMPC2_DRAW_H
#define TDMPC2_DRAW_H
#include <stdint.h>

#include "tdmpc2_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tdmpc2_draw_desc {
    int64_t  n;                  /* normals to write (flat fp32); 0 allowed iff normal == NULL */
    int32_t  num_q;              /* ensemble size the pair is drawn from; read iff pair != NULL */
    uint32_t seed_lo, seed_hi;   /* Philox key */
    uint32_t call_lo, call_hi;   /* call counter, used only when `state` is NULL */
    uint32_t reserved;           /* the tail padding of the 8-byte alignment, named; ignored */
} tdmpc2_draw_desc;   /* 32 bytes */

int tdmpc2_draw_noise(const tdmpc2_draw_desc *d, uint32_t *state, float *normal, int32_t *pair, void *stream);

#ifdef __cplusplus
}
#endif
#endif
