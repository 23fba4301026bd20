"""WorldModel: host-side container with the reference's attribute names and
checkpoint key layout (tdmpc2/common/world_model.py:11-216).

What lives here: parameters (so `load_state_dict` of a reference checkpoint
works), the observation encoder (`encode`, PyTorch-ROCm, as the north star
keeps it), and plain-torch `next/reward/pi/Q` used only outside planning
(`act()` with `mpc=False`).  The planner reads these parameters once, through
`NativePlanner.bind_state_dict`, and runs in HIP.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import autograd, checkpoint, layers


def _symexp(x):
    return torch.sign(x) * (torch.exp(torch.abs(x)) - 1)


def two_hot_inv(x, cfg):
    """reference tdmpc2/common/math.py:74-83."""
    if cfg.num_bins == 0:
        return x
    if cfg.num_bins == 1:
        return _symexp(x)
    bins = torch.linspace(cfg.vmin, cfg.vmax, cfg.num_bins, device=x.device, dtype=x.dtype)
    return _symexp(torch.sum(F.softmax(x, dim=-1) * bins, dim=-1, keepdim=True))


def _pi_tail(out, eps, m, action_dims, log_std_min, log_std_dif):
    """`WorldModel.pi` after its MLP in torch (reference world_model.py:160-184, math.py:12-39): out [..., 2A], eps [..., A], m the
    mask rows and action_dims their sums (multitask) or None -> (action, info)."""
    mean, log_std = out.chunk(2, dim=-1)
    log_std = log_std_min + 0.5 * log_std_dif * (torch.tanh(log_std) + 1)
    if m is not None:
        mean, log_std, eps = mean * m, log_std * m, eps * m
    log_prob = (-0.5 * eps.pow(2) - log_std - 0.9189385175704956).sum(-1, keepdim=True)  # math.gaussian_logprob
    scaled_log_prob = log_prob * (eps.shape[-1] if action_dims is None else action_dims)
    action = mean + eps * log_std.exp()
    mean, action = torch.tanh(mean), torch.tanh(action)  # math.squash
    log_prob = log_prob - torch.log(F.relu(1 - action.pow(2)) + 1e-6).sum(-1, keepdim=True)
    entropy_scale = scaled_log_prob / (log_prob + 1e-8)
    return action, {"mean": mean, "log_std": log_std, "action_prob": 1.0, "entropy": -log_prob,
                    "scaled_entropy": -log_prob * entropy_scale}


class _PiEntropyGrad(torch.autograd.Function):
    """info['entropy'] of the library's policy head, kept differentiable as the modules' is.  The library's backward takes the
    gradients of the action and of scaled_entropy (what update_pi differentiates); a backward that reaches `entropy` itself -- no
    path of the learner does -- is torch autograd of `_pi_tail` on the saved inputs, evaluated only then.  The forward adds nothing."""

    @staticmethod
    def forward(ctx, entropy, out, eps, m, action_dims, log_std_min, log_std_dif):
        ctx.save_for_backward(out, eps, log_std_min, log_std_dif, *([m, action_dims] if m is not None else []))
        ctx.set_materialize_grads(False)
        return entropy.view(entropy.shape)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None, None, None
        out, eps, lmin, ldif, *rest = ctx.saved_tensors
        m, dims = rest if rest else (None, None)
        with torch.enable_grad():
            y = out.detach().requires_grad_(True)
            ent = _pi_tail(y, eps, m, dims, lmin, ldif)[1]["entropy"]
            (gy,) = torch.autograd.grad(ent, y, g.reshape(ent.shape))
        return None, gy, None, None, None, None, None


class WorldModel(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        L, M, A, T = cfg.latent_dim, cfg.mlp_dim, cfg.action_dim, cfg.task_dim
        if cfg.multitask:
            self._task_emb = nn.Embedding(len(cfg.tasks), T, max_norm=1)
            self.register_buffer("_action_masks", torch.zeros(len(cfg.tasks), A))
            for i in range(len(cfg.tasks)):
                self._action_masks[i, : cfg.action_dims[i]] = 1.0
        self._encoder = layers.encoders(cfg)
        self._dynamics = layers.mlp(L + A + T, 2 * [M], L, act=layers.SimNorm(cfg.simnorm_dim))
        self._reward = layers.mlp(L + A + T, 2 * [M], max(cfg.num_bins, 1))
        self._termination = layers.mlp(L + T, 2 * [M], 1) if cfg.episodic else None
        self._pi = layers.mlp(L + T, 2 * [M], 2 * A)
        self._Qs = layers.QEnsemble(cfg.num_q, L + A + T, M, max(cfg.num_bins, 1))
        # the reference keeps a detached alias and a target copy of the Q parameters in the
        # state dict (world_model.py:38-53); they are training state, kept here for key parity
        self._detach_Qs_params = layers.StackedMLPParams(cfg.num_q, L + A + T, M, max(cfg.num_bins, 1), as_buffer=True)
        self._target_Qs_params = layers.StackedMLPParams(cfg.num_q, L + A + T, M, max(cfg.num_bins, 1), as_buffer=True)
        self.register_buffer("log_std_min", torch.tensor(float(cfg.log_std_min)))
        self.register_buffer("log_std_dif", torch.tensor(float(cfg.log_std_max)) - self.log_std_min)
        # True (and the input on the GPU): the MLPs of encode (state), next, reward, termination, pi and Q run through the library's
        # trainable layer (tdmpc2_amd/autograd.py), so loss.backward() computes their gradients in HIP; off by default -- the modules
        self.native_autograd = False
        # True (train mode, cfg.dropout > 0, the input on the GPU): Q and Q_pair multiply the first layer's Linear output of every
        # member by a dropout mask drawn in the library (autograd.DropoutMasks, tdmpc2_dropout_mask), as the reference's Q heads do in
        # train mode; off by default -- no dropout in any mode
        self.native_dropout = False
        self._q_masks = None  # made by the first read of `q_masks`
        # True (multitask, the input on the GPU): encode (state observations), next, reward, Q, Q_pair and pi build their first-layer
        # input [x | task_emb | a] with one library call each (autograd.task_concat, tdmpc2_task_forward: the max_norm renorm, the
        # lookup and the concatenations; its backward in tdmpc2_task_backward); off by default -- nn.Embedding and torch.cat
        self.native_task_emb = False
        # True (cfg.obs == "rgb", single-task, the input on the GPU): encode runs the convolutional encoder through the library's
        # pixel unit (autograd.pixel_encode, tdmpc2_pixgrad_forward / tdmpc2_pixgrad_backward), so loss.backward() computes the
        # encoder's gradients in HIP; ShiftAug's shifts are drawn with the module's own torch.randint call, one draw per time step;
        # off by default -- the nn.Sequential (MIOpen convolutions, grid_sample)
        self.native_pixel_grad = False
        self._log_std_host = None  # host copies of log_std_min / log_std_dif for the library's policy head (made at first use)
        self.apply(self._weight_init)
        self._register_state_dict_hook(self._add_meta_keys)
        self._register_load_state_dict_pre_hook(self._convert_incoming, with_module=True)

    # reference common/init.py:4-11
    @staticmethod
    def _weight_init(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.Embedding):
            nn.init.uniform_(m.weight, -0.02, 0.02)
        elif isinstance(m, layers._StackedLayer):
            nn.init.trunc_normal_(m.weight, std=0.02)

    # ---- state-dict layout ------------------------------------------------------------
    @staticmethod
    def _add_meta_keys(module, state_dict, prefix, local_metadata):
        dev = module.log_std_min.device
        for p in ("_Qs.params.", "_detach_Qs_params.", "_target_Qs_params."):
            state_dict[prefix + p + "__batch_size"] = torch.Size([module.cfg.num_q])
            state_dict[prefix + p + "__device"] = dev
        return state_dict

    @staticmethod
    def _convert_incoming(module, state_dict, prefix, *args):
        module._log_std_host = None
        incoming = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        conv = checkpoint.convert_state_dict(incoming)
        if checkpoint.is_old_format(incoming):
            # released (old-API) checkpoints predate these buffers; the reference's loader takes them from the freshly
            # constructed model (layers.py:211-215) -- and overwrites any value the file might carry, as done here
            conv["log_std_min"] = module.log_std_min.detach().clone()
            conv["log_std_dif"] = module.log_std_dif.detach().clone()
            if hasattr(module, "_action_masks"):
                conv["_action_masks"] = module._action_masks.detach().clone()
        for k in [k for k in state_dict if k.startswith(prefix)]:
            del state_dict[k]
        for k, v in conv.items():
            state_dict[prefix + k] = v

    def planner_state_dict(self):
        """The tensors the HIP planner binds (new-format keys)."""
        sd = {k: v for k, v in self.state_dict().items() if torch.is_tensor(v)}
        return {k: v for k, v in sd.items()
                if k.startswith(("_dynamics.", "_reward.", "_pi.", "_Qs.params.", "_termination.", "_target_Qs_params."))}

    # ---- forward pieces (reference world_model.py:88-216) ------------------------------
    def task_emb(self, x, task):
        if isinstance(task, int):
            task = torch.tensor([task], device=x.device)
        emb = self._task_emb(task.long())
        if x.ndim == 3:
            emb = emb.unsqueeze(0).repeat(x.shape[0], 1, 1)
        elif emb.shape[0] == 1:
            emb = emb.repeat(x.shape[0], 1)
        return torch.cat([x, emb], dim=-1)

    def _net_in(self, x, task, a=None):
        """The first-layer input of a network: [x | task_emb(task) | a] on multitask models, [x | a] otherwise.  With
        `native_task_emb` and the input on the GPU the multitask form is one `autograd.task_concat` call."""
        if self.cfg.multitask:
            if self.native_task_emb and x.is_cuda:
                return autograd.task_concat(self._task_emb.weight, task, x, a, self._task_emb.max_norm)
            x = self.task_emb(x, task)
        return x if a is None else torch.cat([x, a], dim=-1)

    def _mlp(self, seq, x):
        if self.native_autograd and x.is_cuda:
            return autograd.mlp_apply(seq, x)
        return seq(x)

    def encode(self, obs, task):
        """reference world_model.py:103-112, including the [T, B, C, H, W] pixel-sequence branch."""
        if self.cfg.multitask:  # (rgb observations keep the module's lookup)
            obs = self._net_in(obs, task) if self.cfg.obs == "state" else self.task_emb(obs, task)
        if self.native_pixel_grad and self.cfg.obs == "rgb" and not self.cfg.multitask and obs.is_cuda:
            return self._encode_pixels(obs)
        if self.cfg.obs == "rgb" and obs.ndim == 5:
            return torch.stack([self._encoder[self.cfg.obs](o) for o in obs])
        if self.cfg.obs == "state":
            return self._mlp(self._encoder[self.cfg.obs], obs)
        return self._encoder[self.cfg.obs](obs)

    def _encode_pixels(self, obs):
        """encode of rgb observations in the library: [n, C, H, W], or the [T, B, C, H, W] sequence branch as ONE call over T B
        images; the shifts are the module's draws in the module's order (one torch.randint call per time step)."""
        from .native import NativePlanner
        seq = self._encoder[self.cfg.obs]
        if obs.ndim == 5:
            T, B = int(obs.shape[0]), int(obs.shape[1])
            shift = torch.cat([NativePlanner.draw_shift(B, obs.device) for _ in range(T)])
            return autograd.pixel_encode(seq, obs.reshape(T * B, *obs.shape[2:]), shift).view(T, B, -1)
        return autograd.pixel_encode(seq, obs, NativePlanner.draw_shift(int(obs.shape[0]), obs.device))

    def next(self, z, a, task):
        return self._mlp(self._dynamics, self._net_in(z, task, a))

    def reward(self, z, a, task):
        return self._mlp(self._reward, self._net_in(z, task, a))

    def termination(self, z, task, unnormalized=False):
        """reference world_model.py:132-141 (episodic models only)."""
        assert task is None
        logit = self._mlp(self._termination, z)
        return logit if unnormalized else torch.sigmoid(logit)

    def pi(self, z, task, eps=None):
        """Returns (action, info) like the reference (world_model.py:144-184, math.py:12-29): info carries 'mean', 'log_std',
        'action_prob', 'entropy' and 'scaled_entropy' (a dict; the reference's TensorDict has the same keys).  `eps` pins the
        noise of the sample (shaped as the action); by default it is drawn with torch.randn_like, on either path.  With
        `native_autograd` and the input on the GPU everything after the MLP runs in the library (autograd.PiHeadFn, forward and
        backward): the same expression, so the action stream is unchanged in distribution, but its bits differ from torch's (the
        library's tanh / exp / log and its order of the row sums)."""
        out = self._mlp(self._pi, self._net_in(z, task))
        if self.native_autograd and out.is_cuda:
            return self._pi_native(out, task, eps)
        eps = torch.randn_like(out[..., : out.shape[-1] // 2]) if eps is None else eps
        if self.cfg.multitask:
            return _pi_tail(out, eps, self._action_masks[task], self._action_masks.sum(-1)[task].unsqueeze(-1), self.log_std_min,
                            self.log_std_dif)
        return _pi_tail(out, eps, None, None, self.log_std_min, self.log_std_dif)

    def _log_std_consts(self):
        """(log_std_min, log_std_dif) as host floats: two device reads, once (a load_state_dict drops the cache)."""
        if self._log_std_host is None:
            self._log_std_host = (float(self.log_std_min), float(self.log_std_dif))
        return self._log_std_host

    def _pi_native(self, out, task, eps):
        """The tail of `pi` in the library.  out [..., 2A]: the rows are one block [1, R] of the head kernel, or, for a multitask
        [T, B, 2A] with one task per batch column, [T, B] with the mask rows [B, A]."""
        A = out.shape[-1] // 2
        lead = out.shape[:-1]
        R = 1
        for n in lead:
            R *= int(n)
        mean_raw, ls_raw = out.chunk(2, dim=-1)
        eps = torch.randn_like(mean_raw) if eps is None else eps.to(out.device, torch.float32)
        T_, B_, mask = 1, R, None
        if self.cfg.multitask:
            mask = self._action_masks[task].to(torch.float32).reshape(-1, A)
            if out.dim() == 3 and mask.shape[0] == out.shape[1] and out.shape[0] <= 16:
                T_, B_ = int(out.shape[0]), int(out.shape[1])
            elif out.dim() == 3 and mask.shape[0] == out.shape[1]:
                mask = mask.repeat(out.shape[0], 1)
            elif mask.shape[0] == 1:
                mask = mask.expand(R, A)
            elif mask.shape[0] != R:
                raise autograd.native.NativeError(f"pi: {mask.shape[0]} tasks for rows {tuple(lead)}")
        desc = autograd.pi_desc(self.cfg, T_, B_, A, 2, *self._log_std_consts())  # (the head reads no bins: any valid count)
        action, entropy, se = autograd.PiHeadFn.apply(desc, out.reshape(T_, B_, 2 * A), eps.reshape(T_, B_, A), mask)
        log_std = self.log_std_min + 0.5 * self.log_std_dif * (torch.tanh(ls_raw) + 1)
        mean, m, dims = mean_raw, None, None
        if self.cfg.multitask:
            m, dims = self._action_masks[task], self._action_masks.sum(-1)[task].unsqueeze(-1)
            mean, log_std = mean * m, log_std * m
        entropy = entropy.view(*lead, 1)
        if out.requires_grad:
            entropy = _PiEntropyGrad.apply(entropy, out, eps, m, dims, self.log_std_min, self.log_std_dif)
        return action.view(*lead, A), {"mean": torch.tanh(mean), "log_std": log_std, "action_prob": 1.0, "entropy": entropy,
                                       "scaled_entropy": se.view(*lead, 1)}

    @property
    def q_masks(self):
        """The mask stream of the Q ensemble's dropout (autograd.DropoutMasks keyed by cfg.seed), made on the model's device at first use."""
        if self._q_masks is None:
            self._q_masks = autograd.DropoutMasks(int(getattr(self.cfg, "seed", 0)), self.log_std_min.device)
        return self._q_masks

    def _q_mask(self, n, za, q_mask):
        """The mask of a Q pass over the rows `za` [..., K] for n members: the one given, or in train mode with `native_dropout`,
        cfg.dropout > 0 and the input on the GPU a fresh draw [n, ..., mlp_dim]; else None."""
        if q_mask is not None:
            return q_mask
        if self.training and self.native_dropout and self.cfg.dropout > 0 and za.is_cuda:
            return self.q_masks.draw((n, *za.shape[:-1], self.cfg.mlp_dim), self.cfg.dropout)
        return None

    def Q_pair(self, z, a, task, qidx, q_mask=None):
        """The logits of the two heads `qidx` of the online ensemble on DETACHED parameters -> [2, ..., num_bins]: the reference's
        Q(z, a, task, return_type='avg', detach=True) (world_model.py:186-216) before two_hot_inv, restricted to the two drawn heads
        -- 2 of num_q members' work; gradient reaches `a` (and z), never `_Qs`.  qidx: two head indices (tensor or sequence).  q_mask [2, ..., mlp_dim]: the first layer's dropout multipliers of
        the two heads; None: drawn for the two heads only under the conditions of `_q_mask` (the members' masks are independent, so
        this is the reference's distribution), else no dropout."""
        from types import SimpleNamespace
        za = self._net_in(z, task, a)
        idx = torch.as_tensor(qidx, device=za.device).long().reshape(2)
        pick = lambda t: t.detach().index_select(0, idx)  # noqa: E731

        def layer(i):
            l = self._Qs.params.layer(i)
            ln = SimpleNamespace(weight=pick(l.ln.weight), bias=pick(l.ln.bias)) if i < 2 else None
            return SimpleNamespace(weight=pick(l.weight), bias=pick(l.bias), ln=ln)

        sel = SimpleNamespace(n=2, layer=layer)
        q_mask = self._q_mask(2, za, q_mask)
        if self.native_autograd and za.is_cuda:
            return autograd.ensemble_apply(sel, za, q_mask)
        return layers.QEnsemble.apply_params(sel, za, q_mask)

    def Q(self, z, a, task, return_type="min", q_mask=None):
        """reference world_model.py:186-216 on the online ensemble.  q_mask [num_q, ..., mlp_dim]: the first layer's dropout
        multipliers; None: drawn under the conditions of `_q_mask` (train mode, `native_dropout`, cfg.dropout > 0, GPU), else no
        dropout."""
        assert return_type in {"min", "avg", "all"}
        za = self._net_in(z, task, a)
        q_mask = self._q_mask(self.cfg.num_q, za, q_mask)
        if self.native_autograd and za.is_cuda:
            out = autograd.ensemble_apply(self._Qs.params, za, q_mask)
        elif q_mask is not None:
            out = layers.QEnsemble.apply_params(self._Qs.params, za, q_mask)
        else:
            out = self._Qs(za)
        if return_type == "all":
            return out
        qidx = torch.randperm(self.cfg.num_q, device=out.device)[:2]
        Q = two_hot_inv(out[qidx], self.cfg)
        return Q.min(0).values if return_type == "min" else Q.sum(0) / 2
