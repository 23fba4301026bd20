/* The pixel encoder in training (tdmpc2_pixgrad_*): a forward that keeps its activations and the backward of the four
 * convolutions, for autograd over rgb observations (reference layers.py:136-150: ShiftAug, x / 255 - 0.5, Conv 7/2, 5/2, 3/2, 3/1 with
 * ReLU between, Flatten, SimNorm(8); 64 x 64 frames).  A stateless unit beside the planner's ABI (tdmpc2_plan.h, whose version and
 * symbols it leaves as they are), linked into the same libtdmpc2_plan.so: no handle, no allocation, no host synchronisation, no
 * atomics, no wait between workgroups, no environment variable.  A call is its descriptor, its pointers and caller-owned workspaces,
 * ordered by `stream`, and can be captured in a hipGraph.
 *
 *   n images, cin input channels (1..16), C channels (8..64, a multiple of 4).  hw = 841, 169, 36, 16 output pixels of layers 0..3.
 *   obs     [n, cin, 64, 64] uint8 (obs_dtype 0) or fp32 (1) pixel levels          shift  int32 [n, 2] = (dx, dy), clamped to [0, 6]
 *   tab     the 7 x 64 ShiftAug tap table (16 bytes per entry) on the device: tdmpc2_pixgrad_shift_table fills it on the host,
 *           the caller uploads it once; the unit never computes it on the device
 *   W[l]    the Conv2d weight [C, cin_l, k, k] (cin_0 = cin, else C; k = 7, 5, 3, 3), read where it is         b[l]  [C]
 *   acts    n * 1046 C floats: for every image the post-ReLU outputs of layers 0..2, [C][841] | [C][169] | [C][36]; then z [n, 16 C]
 *   dz      [n, 16 C]: the gradient of z (seed_is_preact 0), or of layer 3's pre-activation (1: the SimNorm backward is skipped)
 *   dW[l]   as W[l]     db[l]  [C]     given or NULL as a pair; a NULL pair drops the two launches that only it needs
 * The observation gets no gradient.
 *
 * Forward.  One launch re-packs the weights as [cin_l][k][k][C] into fwd_ws, then the four launches of the batch route
 * (tdmpc2_plan_encode_pix_batch) run on them with their outputs in acts: z has that call's bits.
 *
 * Backward (fp32; every product-sum is an fmaf chain on the 32x32x2 MFMA).  With a_l the saved output of layer l, in_l its input
 * (in_0 = the ShiftAug-resampled, preprocessed frame, recomputed with the forward's expression, never stored) and S the stride:
 *   dy_3 = z (dz - sum over the group of dz z)       groups of 8 features c 16 + 4 y + x; the sum adds j = 0 .. 7 in order
 *   dy_l = da_l (a_l > 0)                            l = 0..2: zero where the saved output is zero
 *   db_l [co] = sum over images and pixels of dy_l
 *   dW_l [co, ci, ky, kx] = sum_{image, oy, ox} dy_l [image, co, oy, ox] in_l [image, ci, S oy + ky, S ox + kx]
 *   da_{l-1} [image, ci, y, x] = sum_{co, ky, kx} dy_l [image, co, (y - ky) / S, (x - kx) / S] W_l [co, ci, ky, kx]
 *                                                    over the taps whose quotients are whole and inside the map
 * Order of dW_l and db_l: the rows (image, oy, ox) in rising order are cut into chunks of 256 and a chunk into sub-chains of 32; a
 * sub-chain is one chain from zero, a chunk's partial adds its sub-chains from zero in rising order; groups of 32 consecutive
 * partials are added from zero in rising order, then the group sums likewise.  db_l is the same sum
 * with in_l = 1.  Order of da: (co, ky, kx) in rising order with co outermost, as chains of 256 terms from zero, each added to the
 * total in order.  Nothing depends on the device or on the other elements of the call: equal inputs give equal bits.
 * One backward is 12 launches whatever n is: the seed, three transposed convolutions, and per layer the partials and their fold.
 * bwd_ws holds dy_0 .. dy_3 ([n][C][hw_l], at the offsets of pixel_grad_route.h) and the partials of the layer in flight.
 *
 * Return codes are tdmpc2_plan.h's (the message: tdmpc2_last_error), before the device is touched: TDMPC2_ERR_INVALID for a NULL
 * descriptor or required pointer, n < 1, obs_dtype or seed_is_preact outside {0, 1}, dW[l] without db[l] or the reverse, no output at
 * all; TDMPC2_ERR_UNSUPPORTED for cin outside [1, 16], C outside [8, 64] or no multiple of 4, n above 2^20. */
#ifndef TDMPC2_PIXEL_GRAD_H
#define TDMPC2_PIXEL_GRAD_H
#include <stddef.h>
#include <stdint.h>

#include "tdmpc2_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tdmpc2_pixgrad_desc {
    int32_t  n;               /* images, 1 .. 2^20 */
    int32_t  cin;             /* input channels of layer 0, 1 .. 16 */
    int32_t  C;               /* channels, 8 .. 64, a multiple of 4 */
    int32_t  obs_dtype;       /* 0 uint8, 1 fp32 */
    int32_t  seed_is_preact;  /* backward: 0 dz is the gradient of z, 1 of layer 3's pre-activation */
    uint32_t reserved;        /* the tail that rounds the size up to 8 bytes, named; ignored */
} tdmpc2_pixgrad_desc;     /* 24 bytes */

int tdmpc2_pixgrad_workspace_bytes(const tdmpc2_pixgrad_desc *d, size_t *acts_bytes, size_t *fwd_ws_bytes, size_t *bwd_ws_bytes);
int tdmpc2_pixgrad_shift_table(void *host_out /* 7 * 64 * 16 bytes */);
int tdmpc2_pixgrad_forward(const tdmpc2_pixgrad_desc *d, const void *obs, const int32_t *shift, const void *tab,
                           const float *const W[4], const float *const b[4], float *fwd_ws, float *acts, void *stream);
int tdmpc2_pixgrad_backward(const tdmpc2_pixgrad_desc *d, const void *obs, const int32_t *shift, const void *tab,
                            const float *const W[4], const float *acts, const float *dz, float *bwd_ws, float *const dW[4],
                            float *const db[4], void *stream);

#ifdef __cplusplus
}
#endif
#endif
