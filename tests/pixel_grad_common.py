"""The pixel encoder's backward (include/tdmpc2_pixel_grad.h) on the CPU: an fp64 closed form on top of pixel_common.reference,
a numpy fp32 emulation of the documented summation orders (tdmpc2_amd/csrc/pixel_grad_route.h: PG_CHUNK, PG_FOLD, PG_DA_SEG), the
torch fp32 yardstick built from torch.nn.grad, and the cases the tests share.

All three take the SAVED activations (layer 0's input, the post-ReLU outputs of layers 0..2, z) and dz as inputs, so the ReLU masks
are shared with the side under test and a sign flip of a pre-activation near zero cannot enter a comparison."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import pixel_common as pc

KERNEL, STRIDE, OUT, SIDE = pc.KERNEL, pc.STRIDE, pc.OUT, (64, 29, 13, 6)
HW = tuple(o * o for o in OUT)
PG_CHUNK, PG_SUB, PG_FOLD, PG_DA_SEG = 256, 32, 32, 128
U = 2.0 ** -24


def seed_grad(z, dz, preact):
    """dy_3 [n, C, 4, 4] from dz [n, 16 C] in the dtype of its inputs: the SimNorm backward, or dz itself."""
    n = z.shape[0]
    if preact:
        return dz.reshape(n, -1, 4, 4)
    zz, dd = z.reshape(n, -1, 8), dz.reshape(n, -1, 8)
    return (zz * (dd - (dd * zz).sum(-1, keepdim=True))).reshape(n, -1, 4, 4)


def stage_dw(x_in, dy, l):
    """One stage on its own inputs, in their dtype: (dW_l [C, cin k k], db_l [C]) from in_l and dy_l [n, C, o, o]."""
    g = dy.flatten(2)
    cols = F.unfold(x_in, KERNEL[l], stride=STRIDE[l])
    return torch.einsum("nch,nkh->ck", g, cols), g.sum((0, 2))


def stage_da(dy, W, l):
    """One stage on its own inputs: da_{l-1} [n, cin_l, side, side], the transposed convolution of dy_l with W_l (no mask)."""
    return F.fold(torch.einsum("ck,nch->nkh", W.reshape(W.shape[0], -1), dy.flatten(2)), SIDE[l], KERNEL[l], stride=STRIDE[l])


def x0_fp32(obs, shifts):
    """Layer 0's input with the forward's bits: pixb_stage0's expression in numpy fp32 (the four-neighbour blend as one fmaf chain
    nw, ne, sw, se from zero with fp32 weight products, then / 255 - 0.5) on the tap table of pixel_route.h.  -> fp32 [n, cin, 64, 64]."""
    lo, hi, w0, w1 = pc.table()
    out = []
    for img, (dx, dy) in zip(np.asarray(obs), shifts):
        q = img.astype(np.float32)
        rl, rh, cl, ch = lo[dy], hi[dy], lo[dx], hi[dx]
        rw0, rw1 = w0[dy].astype(np.float32)[:, None], w1[dy].astype(np.float32)[:, None]
        cw0, cw1 = w0[dx].astype(np.float32)[None, :], w1[dx].astype(np.float32)[None, :]
        v = np.zeros(q.shape, np.float32)
        for rows, cols, w in ((rl, cl, cw0 * rw0), (rl, ch, cw1 * rw0), (rh, cl, cw0 * rw1), (rh, ch, cw1 * rw1)):
            v = _fma(q[:, rows][:, :, cols], np.broadcast_to(w.astype(np.float32), q.shape[1:])[None], v)
        out.append(v / np.float32(255.0) - np.float32(0.5))
    return torch.as_tensor(np.stack(out))


def closed_form(x0, acts, z, dz, Ws, preact=False):
    """The backward of the header in the dtype of its inputs (fp64 for the reference): x0 [n, cin, 64, 64] layer 0's input, acts the
    post-ReLU outputs of layers 0..2, z / dz [n, 16 C].  -> dict dW, db (lists of four), dy (the four pre-activation gradients)."""
    ins = [x0, acts[0], acts[1], acts[2]]
    dy = seed_grad(z, dz, preact)
    dW, db, dys = [None] * 4, [None] * 4, [None] * 4
    for l in (3, 2, 1, 0):
        C = Ws[l].shape[0]
        dys[l] = dy
        g = dy.flatten(2)                                           # [n, C, hw]
        db[l] = g.sum((0, 2))
        cols = F.unfold(ins[l], KERNEL[l], stride=STRIDE[l])        # [n, cin k k, hw]
        dW[l] = torch.einsum("nch,nkh->ck", g, cols).reshape(Ws[l].shape)
        if l > 0:
            da = F.fold(torch.einsum("ck,nch->nkh", Ws[l].reshape(C, -1), g), SIDE[l], KERNEL[l], stride=STRIDE[l])
            dy = da * (ins[l] > 0)
    return dict(dW=dW, db=db, dy=dys)


def torch32(x0, acts, z, dz, Ws, preact=False):
    """The yardstick: the same backward in torch CPU fp32 from torch.nn.grad.conv2d_weight / conv2d_input."""
    f = lambda t: t.float()  # noqa: E731
    ins = [f(x0), f(acts[0]), f(acts[1]), f(acts[2])]
    dy = seed_grad(f(z), f(dz), preact)
    dW, db, dys = [None] * 4, [None] * 4, [None] * 4
    for l in (3, 2, 1, 0):
        dys[l] = dy
        db[l] = dy.sum((0, 2, 3))
        dW[l] = torch.nn.grad.conv2d_weight(ins[l], Ws[l].shape, dy, stride=STRIDE[l])
        if l > 0:
            dy = torch.nn.grad.conv2d_input(ins[l].shape, f(Ws[l]), dy, stride=STRIDE[l]) * (ins[l] > 0)
    return dict(dW=dW, db=db, dy=dys)


# ------------------------------------------------------------------------------------------------- fp32 emulation of the orders
def _fma(a, b, c):
    """fmaf on fp32 arrays: the product is exact in fp64; the sum rounds to fp64 and then to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _fold(p, f):
    """Groups of f consecutive entries of the last axis (f = 0: all of them), each added from zero in rising order."""
    m = p.shape[-1]
    f = f or m
    g = -(-m // f)
    p = np.pad(p, [(0, 0)] * (p.ndim - 1) + [(0, g * f - m)]).reshape(*p.shape[:-1], g, f)   # (adding the padding's zeros is exact)
    s = np.zeros(p.shape[:-1], np.float32)
    for j in range(f):
        s = s + p[..., j]
    return s


def chunked_sum(a, b, chunk=PG_CHUNK, sub=PG_SUB, fold=PG_FOLD):
    """sum_r a[..., r] b[..., r] in the order of dW / db: sub-chains of `sub` consecutive rows, each one fmaf chain from zero; a chunk's
    partial adds its chunk / sub sub-chains from zero in rising order; groups of `fold` consecutive partials likewise; then the group
    sums likewise.  fp32 in, fp32 out."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    R = a.shape[-1]
    ns = -(-R // sub)
    pad = [(0, 0)] * (a.ndim - 1) + [(0, ns * sub - R)]
    a = np.pad(a, pad).reshape(*a.shape[:-1], ns, sub)
    b = np.pad(b, pad).reshape(*b.shape[:-1], ns, sub)
    part = np.zeros(a.shape[:-1], np.float32)
    for i in range(sub):
        part = _fma(a[..., i], b[..., i], part)   # (the padding's fmaf(0, 0, acc) is exact)
    return _fold(_fold(_fold(part, chunk // sub), fold), 0)[..., 0]


def dw_rows(x_in, l, ci, ky, kx):
    """in_l [n, cin, side, side] -> the rows (image, oy, ox) of tap (ci, ky, kx): [n hw]."""
    S, o = STRIDE[l], OUT[l]
    return np.asarray(x_in)[:, ci, ky:ky + S * (o - 1) + 1:S, kx:kx + S * (o - 1) + 1:S].reshape(-1)


def emulate_dw(x_in, dy, l, elems, **kw):
    """dW_l at the elements [(co, ci, ky, kx)] and db_l at the channels those name, in the documented order (fp32)."""
    x_in, dy = np.asarray(x_in, np.float32), np.asarray(dy, np.float32)
    a = np.stack([dw_rows(x_in, l, ci, ky, kx) for _, ci, ky, kx in elems])
    b = np.stack([dy[:, co].reshape(-1) for co, _, _, _ in elems])
    return chunked_sum(a, b, **kw), chunked_sum(np.ones_like(b), b, **kw)


def emulate_dw_full(x_in, dy, l, **kw):
    """All of dW_l [C, cin, k, k] and db_l [C] in the documented order (fp32): small shapes only."""
    x_in, dy = np.asarray(x_in, np.float32), np.asarray(dy, np.float32)
    n, cin = x_in.shape[:2]
    C, k = dy.shape[1], KERNEL[l]
    cols = np.stack([dw_rows(x_in, l, ci, ky, kx) for ci in range(cin) for ky in range(k) for kx in range(k)])  # [K, R]
    g = dy.transpose(1, 0, 2, 3).reshape(C, -1)                                                                # [C, R]
    dW = chunked_sum(cols[None, :, :], g[:, None, :], **kw).reshape(C, cin, k, k)
    return dW, chunked_sum(np.ones_like(g), g, **kw)


def emulate_da(dy, W, l, seg=PG_DA_SEG):
    """da_{l-1} [n, C, side, side] = the transposed convolution of dy_l with W_l in the documented order (fp32): kk = (co, ky, kx)
    in rising order, chains of 2 seg terms from zero, each added to the total."""
    dy, W = np.asarray(dy, np.float32), np.asarray(W, np.float32)
    n, C = dy.shape[:2]
    cin, k, S, o, side = W.shape[1], KERNEL[l], STRIDE[l], OUT[l], SIDE[l]
    acc = np.zeros((n, cin, side, side), np.float32)
    tot = np.zeros_like(acc)
    kk = 0
    for co in range(C):
        for ky in range(k):
            for kx in range(k):
                up = np.zeros((n, 1, side, side), np.float32)
                up[:, 0, ky:ky + S * (o - 1) + 1:S, kx:kx + S * (o - 1) + 1:S] = dy[:, co]
                acc = _fma(up, W[co, :, ky, kx][None, :, None, None], acc)
                kk += 1
                if kk % (2 * seg) == 0:
                    tot, acc = tot + acc, np.zeros_like(acc)
    return tot + acc if kk % (2 * seg) else tot


def roundings_dw(rows):
    """Roundings of the documented order for one dW / db element over `rows` rows: a sub-chain, a chunk, a group, the group sums."""
    nch = -(-rows // PG_CHUNK)
    return min(rows, PG_SUB) + PG_CHUNK // PG_SUB + min(nch, PG_FOLD) + -(-nch // PG_FOLD)


def roundings_da(l, C):
    K = C * KERNEL[l] ** 2
    return K + -(-K // (2 * PG_DA_SEG))


# -------------------------------------------------------------------------------------------------------------------- cases
SHIFTS = [(0, 6), (6, 0), (3, 5), (1, 4), (6, 6), (0, 0), (3, 3), (2, 5), (5, 1), (4, 4), (0, 3), (6, 2), (1, 1), (5, 5), (2, 0),
          (4, 6), (3, 0)]
EDGE_SHAPES = [(8, 1), (32, 9), (40, 16)]


@functools.lru_cache(maxsize=None)
def grad_case(C, cin, n=3, seed=0, fp32=False, trained=True):
    """n images, default-init weights (trained: gains calibrated as pixel_common.stack_case makes them), a fixed upstream gradient G."""
    obs = pc._images(n, cin, 2000 + 64 * cin + C + seed, fp32)
    shifts = SHIFTS[:n]
    Ws, Bs = pc.default_weights(cin, C, 17 * C + cin + seed)
    if trained:
        Ws, Bs = pc.calibrate(obs, shifts, Ws, Bs, pc.STACK_TARGETS)
    g = torch.Generator().manual_seed(5 + seed)
    G = torch.randn(n, 16 * C, generator=g, dtype=torch.float64)
    return dict(obs=obs, shifts=shifts, Ws=Ws, Bs=Bs, C=C, cin=cin, stack=True, G=G)


def saved_of(case):
    """fp64 reference forward of a case -> (x0, [a0, a1, a2], z) as the closed form takes them."""
    ref = pc.reference(case["obs"], case["shifts"], case["Ws"], case["Bs"])
    return ref["x"], ref["act"][:3], ref["z"]


def rel_err(got, ref):
    ref = np.asarray(ref, np.float64)
    den = float(np.abs(ref).max())
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / (den if den > 0 else 1.0)
