// Kernel arguments of the weight packer (refresh_kernels.cuh; routes in refresh_route.h).  Included by launch.h inside
// namespace tdk.  ONE record, passed by value to every launch of a call: the caller's pointers reach the kernels as kernel
// arguments (no host-to-device copy is enqueued; a captured call replays on the same tensors).
#pragma once
#include "refresh_route.h"

// one (net, layer), every ensemble member: sources in the checkpoint's layout (stacked over heads), destinations are the
// handle's slabs (member stride = the slab's per-head size)
struct RfLayer {
    const float *W, *b, *g, *beta;  // [heads][out][in], [heads][out] x 3 (g / beta null without LayerNorm).  Soft update: the TARGET tensors
    float *wdst, *bias, *gd, *bd, *wemb;  // packed operands (halfs when split), padded bias, LayerNorm vectors, task-embedding columns
    int out, in, nz, nt, na, CT, KB;
    int has_ln, mish;
    int scan_nbw;    // RO_SCAN workgroups per member over W (+ 1 for the vectors)
};
struct RfNet {
    RfLayer l[3];
    LayerScal *scal;  // [heads][3] (split) or null
    int heads, mask;  // bit l: layer l is named (0: the net is left as it is).  Absent layers are empty workgroup ranges
};
// nn.Linear [out][in] -> [in][out] plus its vectors (state encoder, policy prior's fp32 copy)
struct RfTrans {
    const float *W, *b, *g, *beta;
    float *wt, *bias, *gd, *bd;
    int out, in;
};
enum { RF_MAX_TRANS = RF_MAX_ENC + 3, RF_SEGS = 3 * RF_NETS + RF_MAX_TRANS };
struct RfParams {
    RfNet net[RF_NETS];
    RfTrans tr[RF_MAX_TRANS];
    int ntrans, split;
    int scan_blk0[3 * RF_NETS + 1];  // first workgroup of job (net, layer) in RO_SCAN
    int pack_blk0[RF_SEGS + 1];      // first workgroup of job (net, layer) / transpose in RO_PACK
    // soft update: net[lerp_net] is lerped towards these before it is scanned (torch.lerp's two forms)
    int lerp_net;                    // -1: no lerp
    float tau;
    const float *online[3][4];
};
static_assert(sizeof(RfParams) <= 4096, "RfParams travels as a kernel argument");
