"""PyTorch autograd over the library's trainable layer (tdmpc2_layer_forward / tdmpc2_layer_backward, include/tdmpc2_plan.h).

`LayerFn` is one NormedLinear (Linear -> dropout mask -> LayerNorm -> Mish or SimNorm) or one plain Linear, forward and backward in
HIP; `mlp_apply` and `ensemble_apply` walk the modules of tdmpc2_amd/layers.py through it, so that `loss.backward()` over
`WorldModel.next / reward / pi / Q` computes every MLP gradient in the library.  `ModelLossFn` / `model_loss` are the four losses of
`TDMPC2._update` and the gradient seeds of their total (tdmpc2_loss_forward / tdmpc2_loss_backward).  `PiHeadFn`, `PiLossFn` / `pi_loss`
are `update_pi` between its layers (tdmpc2_pigrad_*, include/tdmpc2_pi_grad.h): the Gaussian head after `_pi`'s MLP, and two_hot_inv of
the two drawn Q heads, the running scale and the rho-weighted loss.  `TaskConcatFn` / `task_concat` are the task conditioning of a
multitask model (tdmpc2_task_*, include/tdmpc2_task.h): the embedding lookup with max_norm and the concatenation [x | emb | a] that
feeds a network's first layer, with their backward.  `PixelEncoderFn` / `pixel_encode` are the rgb encoder of `layers.conv`
(tdmpc2_pixgrad_*, include/tdmpc2_pixel_grad.h): the batch route's forward with its activations kept, and the backward of the four
convolutions.  There is no fallback: a CPU tensor is an error.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import layers, native


class LayerFn(torch.autograd.Function):
    """y = layer(x).  x [..., K] (leading dimensions are flattened to rows); ungrouped parameters w [N, K], b / ln_w / ln_b [N]
    give y [..., N]; stacked parameters w [G, N, K], ... take x [G, ..., K], or with `shared_x` one x [..., K] for all groups,
    and give y [G, ..., N].  mask: None or dropout's multipliers, shaped as y.  Saves x, pre, stat and mask."""

    @staticmethod
    def forward(ctx, x, w, b, ln_w, ln_b, mask, kind, shared_x, simnorm_dim, eps):
        grouped = w.dim() == 3
        G = w.shape[0] if grouped else 1
        N, K = w.shape[-2], w.shape[-1]
        lead = x.shape[1:-1] if grouped and not shared_x else x.shape[:-1]
        if x.shape[-1] != K or (grouped and not shared_x and x.shape[0] != G):
            raise native.NativeError(f"LayerFn: x {tuple(x.shape)} does not fit w {tuple(w.shape)} (shared_x={bool(shared_x)})")
        R = 1
        for s in lead:
            R *= int(s)
        desc = native.layer_desc(kind, G, R, K, N, shared_x, simnorm_dim, eps)
        xc, wc, bc = x.detach().contiguous(), w.detach().contiguous(), b.detach().contiguous()
        ln = kind != native.LAYER_LINEAR
        lwc = ln_w.detach().contiguous() if ln else None
        lbc = ln_b.detach().contiguous() if ln else None
        mc = mask.detach().contiguous() if mask is not None else None
        y = torch.empty((G, R, N), dtype=torch.float32, device=x.device)
        pre = torch.empty_like(y) if ln else None
        stat = torch.empty((G, R, 2), dtype=torch.float32, device=x.device) if ln else None
        native.layer_forward(desc, xc, wc, bc, lwc, lbc, mc, y, pre, stat)
        ctx.desc, ctx.ln, ctx.x_shape, ctx.w_shape = desc, ln, x.shape, w.shape
        ctx.save_for_backward(xc, wc, lwc, lbc, pre, stat, mc)
        return y.view(*((G,) if grouped else ()), *lead, N)

    @staticmethod
    def backward(ctx, dy):
        xc, wc, lwc, lbc, pre, stat, mc = ctx.saved_tensors
        desc, ln = ctx.desc, ctx.ln
        need_x = ctx.needs_input_grad[0]
        need_p = any(ctx.needs_input_grad[1:5] if ln else ctx.needs_input_grad[1:3])
        dev = dy.device
        new = lambda t: torch.empty_like(t)  # noqa: E731
        dx = new(xc) if need_x else None
        dw = new(wc) if need_p else None
        db = torch.empty(wc.shape[:-1], dtype=torch.float32, device=dev) if need_p else None
        dlw = new(lwc) if need_p and ln else None
        dlb = new(lbc) if need_p and ln else None
        ws = None
        if ln or mc is not None:
            ws = torch.empty(native.layer_workspace_bytes(desc), dtype=torch.uint8, device=dev)  # torch's caching allocator
        native.layer_backward(desc, xc, wc, lwc, lbc, pre, stat, mc, dy.contiguous(), dx, dw, db, dlw, dlb, ws)
        want = ctx.needs_input_grad
        return (dx.view(ctx.x_shape) if want[0] else None, dw if want[1] else None, db if want[2] else None,
                dlw if ln and want[3] else None, dlb if ln and want[4] else None, None, None, None, None, None)


def _dropout_mask(p: float, shape, device):
    """Dropout's multipliers (0 or 1 / (1 - p)), drawn exactly as nn.Dropout draws them."""
    return F.dropout(torch.ones(shape, dtype=torch.float32, device=device), p, True)


def normed_linear_apply(m, x, mask=None):
    """One module of a `layers.mlp()` Sequential: a NormedLinear (Mish or SimNorm) or a plain nn.Linear."""
    if isinstance(m, layers.NormedLinear):
        if isinstance(m.act, layers.SimNorm):
            kind, sd = native.LAYER_SIMNORM, m.act.dim
        elif isinstance(m.act, nn.Mish):
            kind, sd = native.LAYER_MISH, 0
        else:
            raise native.NativeError(f"the library's layer has Mish and SimNorm only (got {m.act!r})")
        if mask is None and m.dropout is not None and m.training and m.dropout.p > 0:
            mask = _dropout_mask(m.dropout.p, (*x.shape[:-1], m.out_features), x.device)
        return LayerFn.apply(x, m.weight, m.bias, m.ln.weight, m.ln.bias, mask, kind, False, sd, m.ln.eps)
    if type(m) is nn.Linear and m.bias is not None:
        return LayerFn.apply(x, m.weight, m.bias, None, None, mask, native.LAYER_LINEAR, False, 0, 0.0)
    raise native.NativeError(f"mlp_apply: no library layer for {m!r}")


def mlp_apply(seq, x):
    """`seq(x)` for a `layers.mlp()` Sequential, every layer in the library."""
    for m in seq:
        x = normed_linear_apply(m, x)
    return x


class DropoutMasks:
    """A device-side stream of dropout masks (tdmpc2_dropout_mask): Philox keyed by `seed`, counted by two words on the device that
    every `draw` advances by one in stream order.  Nothing here reads the device or synchronises, so a draw can be captured in a
    graph, and every replay then draws the next mask."""

    def __init__(self, seed: int, device):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise native.NativeError(f"DropoutMasks draws on an MI355X only (device {self.device}); there is no CPU fallback")
        self.state = torch.zeros(2, dtype=torch.int32, device=self.device)  # the call counter (lo, hi)

    def draw(self, shape, p: float):
        """-> a fresh fp32 tensor of `shape` holding 0 (probability floor(p 2^32) / 2^32) or 1 / (1 - p), from torch's allocator."""
        out = torch.empty(tuple(int(s) for s in shape), dtype=torch.float32, device=self.device)
        native.dropout_mask(native.dropout_desc(out.numel(), p, self.seed), self.state, out)
        return out

    def state_dict(self):
        """The seed and the counter (one device read): enough to resume the stream.  Not part of the reference's checkpoint."""
        lo, hi = (int(v) & 0xFFFFFFFF for v in self.state.tolist())
        return {"seed": self.seed, "counter": (hi << 32) | lo}

    def load_state_dict(self, sd):
        self.seed = int(sd["seed"]) & 0xFFFFFFFFFFFFFFFF
        c = int(sd["counter"]) & 0xFFFFFFFFFFFFFFFF
        words = [w - (1 << 32) if w >= (1 << 31) else w for w in (c & 0xFFFFFFFF, c >> 32)]
        self.state.copy_(torch.tensor(words, dtype=torch.int32))


class Draws:
    """A device-side stream of a training step's draws (tdmpc2_draw_noise): standard normals and an ordered pair of distinct Q heads
    per call, Philox keyed by (`seed`, native.DRAW_KEY_HI) -- `DropoutMasks` keys the same counter layout with (seed, 0), so the two
    streams of one cfg.seed never coincide -- and counted by two words on the device that every `draw` advances by one in stream
    order.  Nothing here reads the device or synchronises, so a draw can be captured in a graph, and every replay then draws afresh."""

    def __init__(self, seed: int, device):
        self.seed = int(seed) & 0xFFFFFFFF
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise native.NativeError(f"Draws draws on an MI355X only (device {self.device}); there is no CPU fallback")
        self.state = torch.zeros(2, dtype=torch.int32, device=self.device)  # the call counter (lo, hi)

    @property
    def key(self) -> int:
        """The 64-bit Philox key: seed in the low word, native.DRAW_KEY_HI in the high word."""
        return (native.DRAW_KEY_HI << 32) | self.seed

    def draw(self, shape, num_q: int):
        """-> (eps fp32 [shape] of standard normals, qidx int32 [2]: two distinct heads out of num_q), fresh tensors from torch's
        allocator, both from one call counter.  A shape of no elements draws the pair alone (the library takes n == 0 only with a
        NULL normal buffer) and still advances the counter."""
        eps = torch.empty(tuple(int(s) for s in shape), dtype=torch.float32, device=self.device)
        qidx = torch.empty(2, dtype=torch.int32, device=self.device)
        native.draw_noise(native.draw_desc(eps.numel(), num_q, self.key), self.state, eps if eps.numel() else None, qidx)
        return eps, qidx

    def state_dict(self):
        """The seed and the counter (one device read): enough to resume the stream.  Not part of the reference's checkpoint."""
        lo, hi = (int(v) & 0xFFFFFFFF for v in self.state.tolist())
        return {"seed": self.seed, "counter": (hi << 32) | lo}

    def load_state_dict(self, sd):
        self.seed = int(sd["seed"]) & 0xFFFFFFFF
        c = int(sd["counter"]) & 0xFFFFFFFFFFFFFFFF
        words = [w - (1 << 32) if w >= (1 << 31) else w for w in (c & 0xFFFFFFFF, c >> 32)]
        self.state.copy_(torch.tensor(words, dtype=torch.int32))


def ensemble_apply(params, x, mask=None):
    """`QEnsemble.apply_params(params, x, mask)` for a `layers.StackedMLPParams`: x [..., K] -> [n, ..., out]; the first layer reads
    the one x for every member (shared_x), so its dx is the sum over members.  mask: None, or the dropout multipliers of the first
    layer's Linear output, [n, ..., hidden] (fp32, e.g. a `DropoutMasks.draw`); the other layers have none."""
    l0, l1, l2 = params.layer(0), params.layer(1), params.layer(2)
    shared = params.n > 1  # (one member: its x is simply [1, ..., K])
    if mask is not None and tuple(mask.shape) != (params.n, *x.shape[:-1], l0.weight.shape[-2]):
        raise native.NativeError(f"ensemble_apply: mask {tuple(mask.shape)} is not [n, ..., hidden] = "
                                 f"{(params.n, *x.shape[:-1], l0.weight.shape[-2])}")
    h = LayerFn.apply(x if shared else x.unsqueeze(0), l0.weight, l0.bias, l0.ln.weight, l0.ln.bias, mask, native.LAYER_MISH, shared, 0,
                      1e-5)
    h = LayerFn.apply(h, l1.weight, l1.bias, l1.ln.weight, l1.ln.bias, None, native.LAYER_MISH, False, 0, 1e-5)
    return LayerFn.apply(h, l2.weight, l2.bias, None, None, None, native.LAYER_LINEAR, False, 0, 0.0)


class ModelLossFn(torch.autograd.Function):
    """(total, parts) = the losses of TDMPC2._update (tdmpc2_loss_forward); backward = the seeds of `total` (tdmpc2_loss_backward).
    Saves the eight inputs, nothing else: the backward recomputes every row.  `parts` [4] is not differentiable."""

    @staticmethod
    def forward(ctx, desc, z_pred, next_z, reward_logits, reward, q_logits, td_target, term_logit, terminated):
        dev = z_pred.device
        ins = [None if t is None else t.detach().contiguous() for t in
               (z_pred, next_z, reward_logits, reward, q_logits, td_target, term_logit, terminated)]
        losses = torch.empty(5, dtype=torch.float32, device=dev)
        ws = torch.empty(native.loss_workspace_bytes(desc), dtype=torch.uint8, device=dev)  # torch's caching allocator
        native.loss_forward(desc, *ins, losses=losses, ws=ws)
        ctx.desc, ctx.episodic = desc, term_logit is not None
        ctx.shapes = [None if t is None else t.shape for t in (z_pred, reward_logits, q_logits, term_logit)]
        ctx.save_for_backward(*[t for t in ins if t is not None])
        parts = losses[:4]
        ctx.mark_non_differentiable(parts)
        return losses[4], parts

    @staticmethod
    def backward(ctx, g_total, _g_parts):
        saved = list(ctx.saved_tensors)
        ins = saved + [None] * (8 - len(saved))
        need = (ctx.needs_input_grad[1], ctx.needs_input_grad[3], ctx.needs_input_grad[5], ctx.episodic and ctx.needs_input_grad[7])
        src = (ins[0], ins[2], ins[4], ins[6])
        outs = [torch.empty_like(s) if n else None for n, s in zip(need, src)]
        if any(o is not None for o in outs):
            g = g_total.detach().to(torch.float32).reshape(1).contiguous()  # stays on the device: no host read
            native.loss_backward(ctx.desc, *ins, grad_total=g, d_z_pred=outs[0], d_reward_logits=outs[1], d_q_logits=outs[2],
                                 d_term_logit=outs[3])
        dz, drl, dql, dtl = [None if o is None else o.view(s) for o, s in zip(outs, ctx.shapes)]
        return None, dz, None, drl, None, dql, None, dtl, None


def model_loss(cfg, z_pred, next_z, reward_logits, reward, q_logits, td_target, term_logit=None, terminated=None):
    """The four losses of `TDMPC2._update` (reference tdmpc2.py:272-304) and their total in the library.  z_pred, next_z [T, B, L]
    (zs[1:] and encode(obs[1:])), reward_logits [T, B, bins], q_logits [num_q, T, B, bins] (Q(..., 'all')), reward, td_target,
    term_logit, terminated [T, B] or [T, B, 1]; the termination pair is given exactly when cfg.episodic.  Returns (total, parts):
    the 0-d differentiable total and the detached [4] tensor consistency, reward, value, termination.  The targets (next_z, reward,
    td_target, terminated) get no gradient; an input that needs none costs no rows of the backward launch.  There is no fallback:
    a CPU tensor is an error."""
    if (term_logit is None) != (terminated is None) or (term_logit is not None) != bool(cfg.episodic):
        raise native.NativeError("model_loss: term_logit and terminated are given exactly when cfg.episodic")
    if z_pred.dim() != 3 or q_logits.dim() != 4:
        raise native.NativeError(f"model_loss: z_pred [T, B, L] and q_logits [num_q, T, B, bins] (got {tuple(z_pred.shape)}, "
                                 f"{tuple(q_logits.shape)})")
    T, B, L = z_pred.shape
    desc = native.loss_desc(T, B, L, q_logits.shape[0], q_logits.shape[-1], cfg.episodic, cfg.vmin, cfg.vmax, cfg.bin_size, cfg.rho,
                            cfg.consistency_coef, cfg.reward_coef, cfg.value_coef, cfg.termination_coef)
    f32 = lambda t: None if t is None else t.to(torch.float32)  # noqa: E731
    return ModelLossFn.apply(desc, z_pred, f32(next_z), reward_logits, f32(reward), q_logits, f32(td_target), term_logit,
                             f32(terminated))


def pi_desc(cfg, steps, batch, action_dim, num_bins, log_std_min, log_std_dif):
    """The descriptor of the policy-loss unit for a [steps, batch] block of rows; log_std_min / log_std_dif are host floats."""
    return native.pigrad_desc(steps, batch, action_dim, num_bins, cfg.multitask, cfg.vmin, cfg.vmax, cfg.rho, cfg.entropy_coef,
                              log_std_min, log_std_dif)


class PiHeadFn(torch.autograd.Function):
    """(action, entropy, scaled_entropy) = the tail of WorldModel.pi after its MLP (tdmpc2_pigrad_head_forward): pi_out [T, B, 2A],
    eps [T, B, A], mask [B, A] or None.  backward = tdmpc2_pigrad_head_backward, one launch.  Saves pi_out, eps and the mask,
    nothing else: the backward recomputes every row.  `entropy` is not differentiable; eps and the mask get no gradient."""

    @staticmethod
    def forward(ctx, desc, pi_out, eps, mask):
        T, B, A = desc.steps, desc.batch, desc.action_dim
        dev = pi_out.device
        yc, ec = pi_out.detach().contiguous(), eps.detach().to(torch.float32).contiguous()
        mc = None if mask is None else mask.detach().to(torch.float32).contiguous()
        action = torch.empty((T, B, A), dtype=torch.float32, device=dev)
        entropy = torch.empty((T, B), dtype=torch.float32, device=dev)
        se = torch.empty((T, B), dtype=torch.float32, device=dev)
        native.pigrad_head_forward(desc, yc, ec, mc, action, entropy, se)
        ctx.desc, ctx.masked, ctx.shape = desc, mc is not None, pi_out.shape
        ctx.save_for_backward(*([yc, ec] + ([mc] if mc is not None else [])))
        ctx.mark_non_differentiable(entropy)
        return action, entropy, se

    @staticmethod
    def backward(ctx, d_action, _d_entropy, d_se):
        saved = list(ctx.saved_tensors)
        yc, ec, mc = saved[0], saved[1], (saved[2] if ctx.masked else None)
        if not ctx.needs_input_grad[1] or (d_action is None and d_se is None):
            return None, None, None, None
        f = lambda g: None if g is None else g.detach().to(torch.float32).contiguous()  # noqa: E731
        out = torch.empty_like(yc)
        native.pigrad_head_backward(ctx.desc, yc, ec, mc, f(d_action), f(d_se), out)
        return None, out.view(ctx.shape), None, None


class PiLossFn(torch.autograd.Function):
    """(pi_loss, parts) of TDMPC2.update_pi (reference tdmpc2.py:220-226) from the two drawn heads' logits: q = the average of
    two_hot_inv (tdmpc2_pigrad_value_forward), `scale_module.update(q[0])` when asked, then the rho-weighted loss at the scale after
    that update (tdmpc2_pigrad_loss_forward).  `parts` [2] = mean entropy, mean scaled_entropy, not differentiable.  backward = the
    one launch of tdmpc2_pigrad_loss_backward; grad_output is handed over as a device pointer, with no host read.  Saves q_logits
    and a copy of the scale the loss divided by."""

    @staticmethod
    def forward(ctx, desc, q_logits, entropy, scaled_entropy, scale_module, update_scale):
        dev = q_logits.device
        T, B = desc.steps, desc.batch
        ql = q_logits.detach().contiguous()
        en, se = entropy.detach().contiguous(), scaled_entropy.detach().contiguous()
        q = torch.empty((T, B), dtype=torch.float32, device=dev)
        native.pigrad_value_forward(desc, ql, q)
        if update_scale:
            scale_module.update(q[0])
        scale = scale_module.value.detach().to(torch.float32).reshape(1).clone()
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        native.pigrad_loss_forward(desc, q, en, se, scale, losses)
        ctx.desc, ctx.shapes = desc, (q_logits.shape, scaled_entropy.shape)
        ctx.save_for_backward(ql, scale)
        parts = losses[1:]
        ctx.mark_non_differentiable(parts)
        return losses[0], parts

    @staticmethod
    def backward(ctx, g_loss, _g_parts):
        ql, scale = ctx.saved_tensors
        need_q, need_se = ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        dq = torch.empty_like(ql) if need_q else None
        dse = torch.empty((ctx.desc.steps, ctx.desc.batch), dtype=torch.float32, device=ql.device) if need_se else None
        if need_q or need_se:
            g = g_loss.detach().to(torch.float32).reshape(1).contiguous()  # stays on the device: no host read
            native.pigrad_loss_backward(ctx.desc, ql, scale, g, dq, dse)
        return (None, None if dq is None else dq.view(ctx.shapes[0]), None, None if dse is None else dse.view(ctx.shapes[1]), None,
                None)


def pi_loss(cfg, q_logits, entropy, scaled_entropy, scale_module, update_scale=True):
    """The policy loss of `TDMPC2.update_pi` (reference tdmpc2.py:220-226) in the library.  q_logits [2, T, B, bins] (the two drawn
    heads: `WorldModel.Q_pair`), entropy and scaled_entropy [T, B] or [T, B, 1] (`WorldModel.pi`'s info), scale_module a
    `RunningScale` (updated with the first step's q unless `update_scale` is False).  Returns (pi_loss, parts): the 0-d
    differentiable loss and the detached [2] tensor mean entropy, mean scaled_entropy.  Gradients reach q_logits and
    scaled_entropy.  There is no fallback: a CPU tensor is an error."""
    if q_logits.dim() != 4 or q_logits.shape[0] != 2:
        raise native.NativeError(f"pi_loss: q_logits [2, T, B, bins] (got {tuple(q_logits.shape)})")
    _, T, B, NB = q_logits.shape
    desc = pi_desc(cfg, T, B, cfg.action_dim, NB, 0.0, 0.0)  # (the value and loss calls read neither log_std constant)
    return PiLossFn.apply(desc, q_logits, entropy.detach().to(torch.float32), scaled_entropy.to(torch.float32), scale_module,
                          bool(update_scale))  # (entropy only feeds a mean of the info dict)


class TaskConcatFn(torch.autograd.Function):
    """out = [x | weight[ids] | a], the first-layer input of a multitask model's networks (WorldModel.task_emb and the torch.cat of
    its callers), through tdmpc2_task_forward / tdmpc2_task_backward (include/tdmpc2_task.h).  The forward renormalises the rows of
    `weight` that `ids` names in place, on `weight.data`, as F.embedding(max_norm=...) does: the renorm is not differentiated.  Saves
    `ids` alone.  The backward asks the library only for the gradients autograd needs: dtable (summed in the header's fixed order,
    the whole table written), dx and da (copies)."""

    @staticmethod
    def forward(ctx, weight, ids, x, a, desc):
        R, W = desc.steps * desc.batch, desc.x_dim + desc.task_dim + desc.a_dim
        xc = x.detach().to(torch.float32).contiguous()
        ac = None if a is None else a.detach().to(torch.float32).contiguous()
        out = torch.empty((R, W), dtype=torch.float32, device=x.device)
        native.task_forward(desc, weight.data, ids, xc, ac, out)
        ctx.desc, ctx.x_shape, ctx.a_shape = desc, x.shape, None if a is None else a.shape
        ctx.save_for_backward(ids)
        return out.view(*x.shape[:-1], W)

    @staticmethod
    def backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        desc = ctx.desc
        need_w, _, need_x, need_a = ctx.needs_input_grad[:4]
        need_a = need_a and ctx.a_shape is not None
        if not (need_w or need_x or need_a):
            return None, None, None, None, None
        dev = dout.device
        dtable = torch.empty((desc.num_tasks, desc.task_dim), dtype=torch.float32, device=dev) if need_w else None
        dx = torch.empty(ctx.x_shape, dtype=torch.float32, device=dev) if need_x else None
        da = torch.empty(ctx.a_shape, dtype=torch.float32, device=dev) if need_a else None
        native.task_backward(desc, ids, dout.detach().to(torch.float32).contiguous(), dx, da, dtable)
        return dtable, None, dx, da, None


def task_concat(weight, ids, x, a=None, max_norm=1.0):
    """[x | weight[ids] | a] in one library call (two launches with the renorm), differentiable in weight, x and a.  weight
    [num_tasks, T] (contiguous fp32, renormalised in place when max_norm > 0); x [S, B, D] with ids [B] or one id, or x [N, D] with
    ids [N] or one id -- the three branches of WorldModel.task_emb; a, when given, shaped as x but for its last dimension; ids an
    int, or an int32 / int64 tensor (anything else is converted to int64).  There is no fallback: a CPU tensor is an error."""
    if isinstance(ids, int):
        ids = torch.tensor([ids], device=x.device)
    if ids.dtype not in (torch.int32, torch.int64):
        ids = ids.long()
    ids = ids.reshape(-1).contiguous()
    if x.dim() not in (2, 3) or (a is not None and a.shape[:-1] != x.shape[:-1]):
        raise native.NativeError(f"task_concat: x [S, B, D] or [N, D] and a shaped alike (got {tuple(x.shape)}, "
                                 f"{None if a is None else tuple(a.shape)})")
    steps, batch = (int(x.shape[0]), int(x.shape[1])) if x.dim() == 3 else (1, int(x.shape[0]))
    if ids.numel() not in (1, batch):
        raise native.NativeError(f"task_concat: {ids.numel()} ids for {batch} batch columns")
    if weight.dtype != torch.float32 or not weight.is_contiguous() or weight.dim() != 2:
        raise native.NativeError("task_concat: weight must be a contiguous fp32 [num_tasks, T] tensor")
    desc = native.task_desc(steps, batch, ids.numel(), ids.element_size(), weight.shape[0], x.shape[-1], weight.shape[1],
                            0 if a is None else a.shape[-1], max_norm if max_norm is not None else 0.0)
    return TaskConcatFn.apply(weight, ids, x, a, desc)


PIXEL_PASS_IMAGES = 256  # images per pass of a pixel_encode call that saves nothing for a backward


class PixelEncoderFn(torch.autograd.Function):
    """z = SimNorm(conv stack(preprocess(ShiftAug(obs)))) for obs [n, cin, 64, 64] (uint8 or fp32 pixel levels) under the integer
    shifts `shift` int32 [n, 2], through tdmpc2_pixgrad_forward / tdmpc2_pixgrad_backward.  Saves obs, shift, the four weights and
    `acts` (the post-ReLU outputs of layers 0..2 and z); the backward writes dW / db of the layers that need them.  obs and shift get
    no gradient."""

    @staticmethod
    def forward(ctx, obs, shift, *params):
        n, cin, C = int(obs.shape[0]), int(obs.shape[1]), int(params[0].shape[0])
        desc = native.pixgrad_desc(n, cin, C, 0 if obs.dtype == torch.uint8 else 1)
        tab = native.pixgrad_shift_table(obs.device)
        Ws = [w.detach().contiguous() for w in params[0::2]]
        bs = [b.detach().contiguous() for b in params[1::2]]
        ab, fb, _ = native.pixgrad_workspace_bytes(desc)
        acts = torch.empty(ab // 4, dtype=torch.float32, device=obs.device)  # torch's caching allocator
        fwd_ws = torch.empty(fb // 4, dtype=torch.float32, device=obs.device)
        native.pixgrad_forward(desc, obs, shift, tab, Ws, bs, fwd_ws, acts)
        ctx.desc = desc
        ctx.save_for_backward(obs, shift, tab, acts, *Ws)
        return acts[acts.numel() - n * 16 * C:].view(n, 16 * C).clone()

    @staticmethod
    def backward(ctx, dz):
        obs, shift, tab, acts, *Ws = ctx.saved_tensors
        desc = ctx.desc
        need = [ctx.needs_input_grad[2 + 2 * l] or ctx.needs_input_grad[3 + 2 * l] for l in range(4)]
        dW = [torch.empty_like(w) if nd else None for w, nd in zip(Ws, need)]
        db = [torch.empty(desc.C, dtype=torch.float32, device=dz.device) if nd else None for nd in need]
        if any(need):
            bwd_ws = torch.empty(native.pixgrad_workspace_bytes(desc)[2] // 4, dtype=torch.float32, device=dz.device)
            native.pixgrad_backward(desc, obs, shift, tab, Ws, acts, dz.detach().to(torch.float32).contiguous(), bwd_ws, dW, db)
        grads = []
        for l in range(4):
            grads += [dW[l] if ctx.needs_input_grad[2 + 2 * l] else None, db[l] if ctx.needs_input_grad[3 + 2 * l] else None]
        return (None, None, *grads)


def _pixel_params(seq):
    convs = [seq[i] for i in (2, 4, 6, 8)] if len(seq) == 11 else []
    ok = (len(convs) == 4 and isinstance(seq[0], layers.ShiftAug) and seq[0].pad == 3 and isinstance(seq[-1], layers.SimNorm)
          and seq[-1].dim == 8 and all(type(m) is nn.Conv2d and m.bias is not None for m in convs)
          and [(m.kernel_size[0], m.stride[0]) for m in convs] == [(7, 2), (5, 2), (3, 2), (3, 1)])
    if not ok:
        raise native.NativeError("pixel_encode: seq must be layers.conv(..., act=SimNorm(8)): ShiftAug(3), preprocess, Conv 7/2, 5/2, "
                                 "3/2, 3/1 with ReLU between, Flatten, SimNorm(8)")
    return [t for m in convs for t in (m.weight, m.bias)]


def pixel_encode(seq, obs, shift, pass_images: int = PIXEL_PASS_IMAGES):
    """`seq(obs)` for the `layers.conv` Sequential with ShiftAug's draw replaced by `shift` int32 [n, 2] (NativePlanner.draw_shift):
    obs [n, cin, 64, 64], uint8 or floating pixel levels -> z [n, 16 C], differentiable in the four convolutions' parameters.  When
    no gradient is needed (torch.no_grad, or no parameter requires one) nothing is saved and the call runs in passes of `pass_images`
    images over one scratch buffer: rows are independent, so the bits are those of one pass.  There is no fallback: a CPU tensor is
    an error."""
    params = _pixel_params(seq)
    if obs.device.type != "cuda":
        raise native.NativeError(f"pixel_encode runs on an MI355X only (device {obs.device}); there is no CPU fallback")
    if obs.dim() != 4 or tuple(obs.shape[2:]) != (64, 64):
        raise native.NativeError(f"pixel_encode: obs [n, cin, 64, 64] (got {tuple(obs.shape)})")
    if obs.dtype != torch.uint8:
        obs = obs.to(torch.float32)
    obs, shift = obs.contiguous(), shift.to(torch.int32).contiguous()
    n = int(obs.shape[0])
    if torch.is_grad_enabled() and any(t.requires_grad for t in params):
        return PixelEncoderFn.apply(obs, shift, *params)
    C, cin, step = int(params[0].shape[0]), int(obs.shape[1]), max(1, min(int(pass_images), n))
    Ws, bs = [w.detach().contiguous() for w in params[0::2]], [b.detach().contiguous() for b in params[1::2]]
    tab = native.pixgrad_shift_table(obs.device)
    ab, fb, _ = native.pixgrad_workspace_bytes(native.pixgrad_desc(step, cin, C))
    acts = torch.empty(ab // 4, dtype=torch.float32, device=obs.device)
    fwd_ws = torch.empty(fb // 4, dtype=torch.float32, device=obs.device)
    z = torch.empty((n, 16 * C), dtype=torch.float32, device=obs.device)
    for e0 in range(0, n, step):
        m = min(step, n - e0)
        desc = native.pixgrad_desc(m, cin, C, 0 if obs.dtype == torch.uint8 else 1)
        native.pixgrad_forward(desc, obs[e0:e0 + m], shift[e0:e0 + m], tab, Ws, bs, fwd_ws, acts)
        z[e0:e0 + m] = acts[native.pixgrad_workspace_bytes(desc)[0] // 4 - m * 16 * C:][:m * 16 * C].view(m, 16 * C)
    return z
