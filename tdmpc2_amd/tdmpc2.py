"""TDMPC2: the drop-in boundary (reference tdmpc2/tdmpc2.py:11-120,138-206).

Same constructor argument (`cfg`), same `act(obs, t0, eval_mode, task)` /
`plan(obs, t0, eval_mode, task)` / `load(fp)` / `save(fp)` signatures, same
`model` attribute names and checkpoint layout, same `_prev_mean` buffer — so
the reference's `evaluate.py:57-59,80` works unchanged with this class.  The
planning itself (everything of `_plan` after `encode`) runs in the HIP library;
there is no PyTorch or CPU fallback for it.

Extension over the reference (whose planner is hard-wired to one environment,
tdmpc2.py:111,163): `act_batch` / `plan_batch` plan E independent environments
in one call — the vectorised-env case the north star shards across GPUs.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import checkpoint
from .config import get_discount
from .native import NativePlanner
from .scale import RunningScale
from .world_model import WorldModel


def _rank() -> int:
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return int(torch.distributed.get_rank())
    return int(os.environ.get("RANK", 0))


class TDMPC2(torch.nn.Module):
    def __init__(self, cfg, device: Optional[torch.device] = None, max_envs: int = 1):
        super().__init__()
        self.cfg = cfg
        if device is None:
            device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))  # reference: cuda:0
        self.device = torch.device(device)
        self.model = WorldModel(cfg).to(self.device)
        self.model.eval()
        self.cfg.iterations += 2 * int(cfg.action_dim >= 20)  # reference tdmpc2.py:34
        if cfg.multitask:  # reference tdmpc2.py:35-37
            self.discount = torch.tensor([get_discount(cfg, ep_len) for ep_len in cfg.episode_lengths],
                                         device=self.device)
        else:
            self.discount = get_discount(cfg, cfg.episode_length)
        self._prev_mean = torch.nn.Buffer(torch.zeros(cfg.horizon, cfg.action_dim, device=self.device))
        self.scale = RunningScale(cfg, self.planner, self.device)  # reference tdmpc2.py:38
        self.max_envs = int(max_envs)
        self.native_encoder = True  # False: encode with the PyTorch-ROCm module (the parity tests compare both)
        # True: rgb observations are encoded inside the library too (tdmpc2_plan_run_pix); off by default -- the PyTorch-ROCm
        # conv module encodes them and the planner is handed the latent
        self.native_pixel_encoder = False
        # images per pass of the library's batch route for rgb training batches (model_losses / update_info with
        # native_pixel_encoder): the workspace the agent reserves on first use (NativePlanner.reserve_pix_batch).  Raised later, the
        # next call grows the workspace; lowered later, the reservation stays (the library never shrinks it) and so do the passes
        self.pixel_batch_images = 256
        self._pix_shift = None      # ShiftAug's shifts of the last native pixel plan (a re-planned step reuses them)
        # True: act() with cfg.mpc == False (the policy prior, tdmpc2.py:114-120) runs inside the library too (tdmpc2_plan_act_pi /
        # act_pi_pix / pi); off by default -- the PyTorch-ROCm modules encode and evaluate _pi
        self.native_policy = False
        # True: sync_planner_weights() re-packs an existing handle from the model's own parameter tensors in at most four launches
        # (tdmpc2_plan_refresh_weights: no copies, no stream synchronisation); off by default -- the per-layer binds
        self.native_refresh = False
        # True: the draws of a training step (the policy noise and the two Q heads of the TD target and of `update_pi`) are made in the
        # library from a counter on the device (autograd.Draws, tdmpc2_draw_noise), so the step reads no host seed and no framework
        # generator; off by default -- the host seed and torch's generator, as before
        self.native_draws = False
        self._draws = None  # made by the first read of `draws`
        self._reuse_shift = False
        self._planner: Optional[NativePlanner] = None
        self._optim = self._pi_optim = None  # made by the first read of `optim` / `pi_optim`: nothing for a planning-only user
        self._planner_log_std = None
        self.last_td_targets = None  # the TD target [H, B, 1] of the last update_model call
        self.last_zs = None          # its rollout's latents [H+1, B, L], detached: what update_pi is given
        self.last_term_logit = None  # its termination logits [H, B, 1], detached (episodic models)
        self._prev_mean_batch = None
        # Philox stream of the in-library noise: cfg.seed in the low word, the rank in the high word, so that env-sharded
        # ranks built from one cfg (tdmpc2_amd/dist.py) do not draw identical exploration noise; a per-call counter is
        # added on top.  (torch.manual_seed does not reach the planner: its RNG lives in the kernels.)
        self._seed = (_rank() << 32) ^ (int(getattr(cfg, "seed", 0)) & 0xFFFFFFFF)
        self.noise_tape = None  # optional dict of device tensors (tdmpc2_noise) for reproducible plans
        self._one = torch.ones(1, dtype=torch.uint8, device=self.device) if self.device.type == "cuda" else None
        self._zero = torch.zeros(1, dtype=torch.uint8, device=self.device) if self.device.type == "cuda" else None

    @property
    def native_autograd(self) -> bool:
        """True: the model's MLPs run through the library's trainable layer, forward and backward (WorldModel.native_autograd)."""
        return self.model.native_autograd

    @native_autograd.setter
    def native_autograd(self, on: bool):
        self.model.native_autograd = bool(on)

    @property
    def native_dropout(self) -> bool:
        """True: in train mode the Q ensemble's first layer drops with masks drawn in the library (WorldModel.native_dropout)."""
        return self.model.native_dropout

    @native_dropout.setter
    def native_dropout(self, on: bool):
        self.model.native_dropout = bool(on)

    @property
    def native_task_emb(self) -> bool:
        """True: on a multitask model the first-layer inputs of encode (state), next, reward, Q, Q_pair and pi come from the library's
        task unit, forward and backward (WorldModel.native_task_emb).  The training methods need `native_autograd` as before; the
        no-grad methods (planning, acting, the TD target) do not read the flag."""
        return self.model.native_task_emb

    @native_task_emb.setter
    def native_task_emb(self, on: bool):
        self.model.native_task_emb = bool(on)

    @property
    def native_pixel_grad(self) -> bool:
        """True: on a single-task rgb model `model.encode` runs the convolutional encoder through the library's pixel unit, forward
        and backward (WorldModel.native_pixel_grad).  `native_pixel_encoder` and its handle routes do not read the flag."""
        return self.model.native_pixel_grad

    @native_pixel_grad.setter
    def native_pixel_grad(self, on: bool):
        self.model.native_pixel_grad = bool(on)

    @property
    def draws(self):
        """The draw stream of the training step (autograd.Draws keyed by cfg.seed), made on this device at first use."""
        if self._draws is None:
            from . import autograd
            self._draws = autograd.Draws(int(getattr(self.cfg, "seed", 0)), self.device)
        return self._draws

    # ------------------------------------------------------------------ checkpoint I/O
    def save(self, fp):
        """reference tdmpc2.py:72-79."""
        torch.save({"model": self.model.state_dict()}, fp)

    def load(self, fp):
        """reference tdmpc2.py:81-95: path or dict; old- and new-format Q keys."""
        if isinstance(fp, dict):
            state_dict = fp
        else:
            state_dict = torch.load(fp, map_location=self.device, weights_only=False)
        state_dict = state_dict["model"] if "model" in state_dict else state_dict
        # key conversion (old API -> new, tensordict meta entries dropped, buffers an old file lacks filled from this
        # model as reference layers.py:167-221 does) happens in WorldModel's load_state_dict pre-hook
        self.model.load_state_dict(dict(state_dict))
        self.sync_planner_weights()

    # ------------------------------------------------------------------ native planner
    def planner(self) -> NativePlanner:
        # (log_std_min / log_std_dif are constants of the handle; they can only change in load() / sync_planner_weights(),
        # which drop a stale handle -- no device read, hence no stream sync, on the planning path)
        if self._planner is None:
            self._planner_log_std = self._log_std()
            self._planner = NativePlanner(self.cfg, self.cfg.iterations, self.device, max_envs=self.max_envs,
                                          log_std_min=self._planner_log_std[0], log_std_dif=self._planner_log_std[1])
            self._planner.bind_state_dict(self.model.planner_state_dict())
            self._bind_encoder()
        return self._planner

    def _log_std(self):
        """(log_std_min, log_std_dif) as host floats: two device reads -- only where the weights can change."""
        return float(self.model.log_std_min), float(self.model.log_std_dif)

    def _bind_encoder(self):
        # state observations: WorldModel.encode runs inside the library as well (include/tdmpc2_plan.h,
        # tdmpc2_plan_run_obs); pixel observations are encoded by the PyTorch-ROCm conv module (layers.conv) and enter
        # the library as latents (tdmpc2_plan_run), or -- native_pixel_encoder -- inside the library (tdmpc2_plan_run_pix)
        if self.native_encoder and self.cfg.obs == "state":
            sd = {k: v for k, v in self.model.state_dict().items() if torch.is_tensor(v) and k.startswith("_encoder.state.")}
            self._planner.bind_encoder(sd)
        if self.native_pixel_encoder and self.cfg.obs == "rgb":
            self._bind_pixel_encoder()

    def _bind_pixel_encoder(self):
        sd = {k: v for k, v in self.model.state_dict().items() if torch.is_tensor(v) and k.startswith("_encoder.rgb.")}
        self._planner.bind_pixel_encoder(sd)

    def _bind_policy(self):
        sd = {k: v for k, v in self.model.state_dict().items() if torch.is_tensor(v) and k.startswith("_pi.")}
        self._planner.bind_policy(sd)

    def sync_planner_weights(self):
        """Re-pack the model's current weights into the planner (after load / a training step).  Reads log_std_min / log_std_dif
        from the device (two host reads): a handle made with other constants is dropped and rebuilt by the next planner() call."""
        if self._planner is not None and self._planner_log_std != self._log_std():
            self._planner.close()
            self._planner = None  # rebuilt (with the new constants and weights) by the next planner() call
        self._repack_planner()

    def _repack_planner(self):
        """`sync_planner_weights` without the comparison of the handle's constants: no device read, no synchronisation.  What an
        optimiser step needs -- log_std_min / log_std_dif are buffers that no optimiser holds."""
        if self._planner is not None and self.native_refresh:
            self._planner.refresh_state_dict(self._refresh_state_dict())  # the policy prior's copy included, when bound
            if self.native_pixel_encoder and self.cfg.obs == "rgb":
                self._bind_pixel_encoder()
        elif self._planner is not None:
            self._planner.bind_state_dict(self.model.planner_state_dict())
            self._bind_encoder()
            if self._planner.policy_bound:
                self._bind_policy()

    def _refresh_state_dict(self):
        """The model's own tensors (no copies) that a refresh reads: the planner's nets and, where the library encodes, the state encoder."""
        sd = self.model.planner_state_dict()
        if self.native_encoder and self.cfg.obs == "state":
            sd.update({k: v for k, v in self.model.state_dict().items() if torch.is_tensor(v) and k.startswith("_encoder.state.")})
        return sd

    # ------------------------------------------------------------------ optimisers (reference tdmpc2.py:22-31)
    @property
    def optim(self):
        """The model's optimiser with the reference's groups (the encoder at lr * enc_lr_scale; the termination head and the task
        embedding only where the model has them), clipping at cfg.grad_clip_norm: a tdmpc2_amd.ClipAdam, made at first use.  From
        then on every parameter's .grad is a view into its gradient arena."""
        if self._optim is None:
            from .optim import ClipAdam
            cfg, m = self.cfg, self.model
            self._optim = ClipAdam([
                {"params": m._encoder.parameters(), "lr": cfg.lr * cfg.enc_lr_scale},
                {"params": m._dynamics.parameters()},
                {"params": m._reward.parameters()},
                {"params": m._termination.parameters() if cfg.episodic else []},
                {"params": m._Qs.parameters()},
                {"params": m._task_emb.parameters() if cfg.multitask else []},
            ], lr=cfg.lr, max_norm=cfg.grad_clip_norm)
        return self._optim

    @property
    def pi_optim(self):
        """The policy prior's optimiser (reference tdmpc2.py:31: eps = 1e-5), clipping at cfg.grad_clip_norm (tdmpc2.py:227)."""
        if self._pi_optim is None:
            from .optim import ClipAdam
            self._pi_optim = ClipAdam(self.model._pi.parameters(), lr=self.cfg.lr, eps=1e-5, max_norm=self.cfg.grad_clip_norm)
        return self._pi_optim

    def optimizer_step(self, which: str = "model"):
        """clip_grad_norm_ + step + zero_grad of `optim` ("model") or `pi_optim` ("pi") in the library, then the re-pack of
        `sync_planner_weights()` so that the planner's packed weights follow -- without its comparison of log_std_min / log_std_dif,
        which are buffers no optimiser steps: the call makes no host read of them.  Returns the gradient norm (0-d device tensor)."""
        if which not in ("model", "pi"):
            raise ValueError(f"optimizer_step: which must be 'model' or 'pi', got {which!r}")
        norm = (self.optim if which == "model" else self.pi_optim).step()
        self._repack_planner()
        return norm

    def soft_update_target_Q(self):
        """reference world_model.py:82-86 (the last line of TDMPC2._update, tdmpc2.py:316): `_target_Qs_params` lerped in place
        towards `_Qs.params` with cfg.tau inside the library, which leaves its target ensemble packed from the result."""
        sd = self.model.planner_state_dict()
        self.planner().soft_update_target({k: v for k, v in sd.items() if k.startswith(("_Qs.params.", "_target_Qs_params."))},
                                          float(self.cfg.tau))

    def _disc_pow(self, tasks):
        """discount^0..discount^H exactly as tdmpc2.py:126,130-132 accumulates it: python-float
        products (single task) or fp32 tensor products (multitask)."""
        H = self.cfg.horizon
        if self.cfg.multitask:
            g = self.discount[tasks.long()].to(torch.float32)  # [E]
            cols = [torch.ones_like(g)]
            for _ in range(H):
                cols.append(cols[-1] * g)
            return torch.stack(cols, dim=1).contiguous()
        d, vals = 1, []
        for _ in range(H + 1):
            vals.append(float(d))
            d = d * self.discount
        return torch.tensor(vals, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ reference API
    @property
    def plan(self):
        """reference tdmpc2.py:45-55 (there: optionally torch.compile'd; here: the HIP planner)."""
        return self._plan

    @torch.no_grad()
    def act(self, obs, t0=False, eval_mode=False, task=None):
        """reference tdmpc2.py:97-120."""
        obs = obs.to(self.device, non_blocking=True).unsqueeze(0)
        if task is not None:
            task = torch.tensor([task], device=self.device)
        if self.cfg.mpc:
            a = self.plan(obs, t0=t0, eval_mode=eval_mode, task=task).cpu()
            if self._planner is not None and self._planner.take_fault():
                # a cluster hand-over of THIS plan gave up (another process / kernel held the compute units): the library
                # returned NaN and left _prev_mean alone; it has switched to the path without hand-overs -- plan again
                # (the native pixel route with the same ShiftAug shifts: the step is re-planned, not re-drawn)
                self._reuse_shift = True
                try:
                    a = self.plan(obs, t0=t0, eval_mode=eval_mode, task=task).cpu()
                finally:
                    self._reuse_shift = False
            return a
        if self.native_policy:
            return self._act_policy(obs, eval_mode, task)[0].cpu()
        z = self.model.encode(obs, task)
        action, info = self.model.pi(z, task)
        if eval_mode:
            action = info["mean"]
        return action[0].cpu()

    @torch.no_grad()
    def _plan(self, obs, t0=False, eval_mode=False, task=None):
        """reference tdmpc2.py:138-206.  obs [1, obs_dim] on device; task int64[1] or None."""
        t0 = self._one if t0 else self._zero
        prev = self._prev_mean.view(1, *self._prev_mean.shape)
        if self.native_encoder and self.cfg.obs == "state":
            return self._plan_obs(obs.to(torch.float32).contiguous(), t0, eval_mode, task, prev)[0]
        if self._native_pix():
            return self._plan_pix(obs, t0, eval_mode, prev)[0]
        z = self.model.encode(obs, task)  # PyTorch-ROCm encoder (pixels, or native_encoder = False)
        return self._plan_latent(z.contiguous(), t0, eval_mode, task, prev)[0]

    # ------------------------------------------------------------------ vectorised extension
    @torch.no_grad()
    def plan_batch(self, obs, t0, eval_mode=False, tasks=None):
        """E environments at once.  obs [E, obs_dim]; t0 bool[E] (or bool); tasks int64[E] or None."""
        obs = obs.to(self.device)
        E = obs.shape[0]
        tasks = torch.as_tensor(tasks, device=self.device).long() if self.cfg.multitask else None
        if self._prev_mean_batch is None or self._prev_mean_batch.shape[0] != E:
            self._prev_mean_batch = torch.zeros(E, self.cfg.horizon, self.cfg.action_dim, device=self.device)
        if isinstance(t0, bool):
            t0 = torch.full((E,), int(t0), dtype=torch.uint8, device=self.device)
        else:
            t0 = torch.as_tensor(t0, device=self.device).to(torch.uint8)
        if self.native_encoder and self.cfg.obs == "state":
            return self._plan_obs(obs.to(torch.float32).contiguous(), t0, eval_mode, tasks, self._prev_mean_batch)
        if self._native_pix():
            return self._plan_pix(obs, t0, eval_mode, self._prev_mean_batch)
        if self.cfg.multitask:
            emb = self.model._task_emb(tasks)  # max_norm renorm happens inside the lookup
            z = self.model._encoder[self.cfg.obs](torch.cat([obs, emb], dim=-1))
        else:
            z = self.model._encoder[self.cfg.obs](obs)
        return self._plan_latent(z.contiguous(), t0, eval_mode, tasks, self._prev_mean_batch)

    @torch.no_grad()
    def act_batch(self, obs, t0, eval_mode=False, tasks=None):
        a = self.plan_batch(obs, t0, eval_mode, tasks).cpu()
        if self._planner is not None and self._planner.take_fault():  # see act()
            self._reuse_shift = True
            try:
                a = self.plan_batch(obs, t0, eval_mode, tasks).cpu()
            finally:
                self._reuse_shift = False
        return a

    # ------------------------------------------------------------------ policy prior (act() with cfg.mpc == False)
    @torch.no_grad()
    def act_policy_batch(self, obs, eval_mode=False, tasks=None):
        """act() without planning (tdmpc2.py:114-120) for E environments: obs [E, ...]; tasks int64 [E] or None -> action [E, A]
        on the host.  The library route with `native_policy`, the PyTorch-ROCm modules otherwise."""
        obs = obs.to(self.device)
        tasks = torch.as_tensor(tasks, device=self.device).long() if self.cfg.multitask else None
        if self.native_policy:
            return self._act_policy(obs, eval_mode, tasks).cpu()
        z = self.model.encode(obs, tasks)
        action, info = self.model.pi(z, tasks)
        return (info["mean"] if eval_mode else action).cpu()

    def _act_policy(self, obs, eval_mode, tasks):
        """The policy prior in the library.  eps is drawn with torch.randn on the host framework's generator -- the draw
        WorldModel.pi's randn_like makes, after ShiftAug's for pixels -- so the RNG stream stays the reference's."""
        E = obs.shape[0]
        planner = self.planner()
        if E > planner.max_envs:
            raise ValueError(f"{E} environments exceed max_envs={planner.max_envs} given at construction")
        if not planner.policy_bound:
            self._bind_policy()
        emb = mask = None
        if self.cfg.multitask:
            emb = self.model._task_emb(tasks.long()).to(torch.float32).contiguous()
            mask = self.model._action_masks[tasks.long()].to(torch.float32).contiguous()
        if self.native_encoder and self.cfg.obs == "state":
            eps = torch.randn(E, self.cfg.action_dim, device=self.device)
            a, _ = planner.act_pi(obs.to(torch.float32).contiguous(), task_emb=emb, act_mask=mask, eps=eps, eval_mode=eval_mode)
            return a
        if self._native_pix():
            if planner.__dict__.get("pix_channels") is None:
                self._bind_pixel_encoder()
            if obs.dtype not in (torch.uint8, torch.float32):
                obs = obs.to(torch.float32)
            shift = planner.draw_shift(E, self.device)
            eps = torch.randn(E, self.cfg.action_dim, device=self.device)
            a, _ = planner.act_pi_pix(obs.contiguous(), shift, eps=eps, eval_mode=eval_mode)
            return a
        z = self.model.encode(obs, tasks).to(torch.float32).contiguous()
        eps = torch.randn(E, self.cfg.action_dim, device=self.device)
        a, info = planner.pi(z, task_emb=emb, act_mask=mask, eps=eps)
        return info["mean"] if eval_mode else a

    @torch.no_grad()
    def policy(self, zs, task=None, eps=None):
        """WorldModel.pi on a training batch in the library (the policy-prior counterpart of `policy_value`): zs [..., L], task
        int64 [B] (broadcast over a leading horizon axis, as in update_pi) -> (action [..., A], info with the reference's keys).
        eps [..., A] pins the noise; by default it is drawn inside the library.  Forward only: no gradients."""
        lead = zs.shape[:-1]
        z2 = zs.reshape(-1, zs.shape[-1]).to(self.device, torch.float32).contiguous()
        planner = self.planner()
        if not planner.policy_bound:
            self._bind_policy()
        emb = mask = None
        if self.cfg.multitask:
            task = torch.as_tensor(task, device=self.device)
            if zs.dim() == 3 and task.numel() == zs.shape[1]:
                task = task.repeat(zs.shape[0])
            emb_t, mask_t, _ = self._task_tables()
            task = task.long().reshape(-1)
            emb, mask = emb_t[task].contiguous(), mask_t[task].contiguous()
        if eps is not None:
            eps = eps.reshape(-1, eps.shape[-1]).to(self.device, torch.float32).contiguous()
        self._seed += 1
        a, info = planner.pi(z2, task_emb=emb, act_mask=mask, eps=eps, seed=self._seed)
        info = {k: (v.reshape(*lead, v.shape[-1]) if torch.is_tensor(v) else v) for k, v in info.items()}
        return a.reshape(*lead, -1), info

    def _plan_inputs(self, E, tasks):
        planner = self.planner()
        if E > planner.max_envs:
            raise ValueError(f"{E} environments exceed max_envs={planner.max_envs} given at construction")
        emb = mask = None
        if self.cfg.multitask:
            emb = self.model._task_emb(tasks.long()).to(torch.float32).contiguous()
            mask = self.model._action_masks[tasks.long()].contiguous()
            disc = self._disc_pow(tasks)
        else:
            disc = self._disc_pow(None).unsqueeze(0).repeat(E, 1).contiguous()
        self._seed += 1
        return planner, emb, mask, disc

    def _plan_obs(self, obs, t0, eval_mode, tasks, prev_mean):
        """encode + plan inside the library (tdmpc2_plan_run_obs)."""
        planner, emb, mask, disc = self._plan_inputs(obs.shape[0], tasks)
        return planner.plan_obs(obs, disc, prev_mean, t0, eval_mode=eval_mode, task_emb=emb, act_mask=mask,
                                tape=self.noise_tape, seed=self._seed)

    def _native_pix(self) -> bool:
        return self.native_pixel_encoder and self.cfg.obs == "rgb"

    def _plan_pix(self, obs, t0, eval_mode, prev_mean):
        """ShiftAug's draw on the host framework's generator (as the conv module would draw it), then encode + plan inside the
        library (tdmpc2_plan_run_pix).  A re-planned step (act after a reported fault) reuses the step's shifts."""
        E = obs.shape[0]
        if obs.dtype not in (torch.uint8, torch.float32):
            obs = obs.to(torch.float32)
        obs = obs.contiguous()
        planner, _, _, disc = self._plan_inputs(E, None)
        if planner.__dict__.get("pix_channels") is None:  # flag set after the handle was made
            self._bind_pixel_encoder()
        if not (self._reuse_shift and self._pix_shift is not None and self._pix_shift.shape[0] == E):
            self._pix_shift = planner.draw_shift(E, self.device)
        return planner.plan_pix(obs, self._pix_shift, disc, prev_mean, t0, eval_mode=eval_mode, tape=self.noise_tape,
                                seed=self._seed)

    def _plan_latent(self, z, t0, eval_mode, tasks, prev_mean):
        planner, emb, mask, disc = self._plan_inputs(z.shape[0], tasks)
        return planner.plan(z.to(torch.float32), disc, prev_mean, t0, eval_mode=eval_mode, task_emb=emb,
                            act_mask=mask, tape=self.noise_tape, seed=self._seed)

    # ------------------------------------------------------------------ training-side forward
    def _task_tables(self):
        """The per-task tables a training batch indexes with `task` (world_model.py:88-101; tdmpc2.py:35-37)."""
        w = self.model._task_emb.weight.detach().to(torch.float32)
        n = w.norm(2, dim=-1, keepdim=True)
        emb = torch.where(n > 1.0, w * (1.0 / (n + 1e-7)), w).contiguous()  # nn.Embedding(max_norm=1) at lookup
        return emb, self.model._action_masks.to(torch.float32).contiguous(), self.discount.to(torch.float32).contiguous()

    @torch.no_grad()
    def _td_target(self, next_z, reward, terminated, task=None, pi_eps=None, qidx=None):
        """reference tdmpc2.py:239-254 (already `@torch.no_grad()` there): the TD target of a training batch on the planner's
        kernels.  next_z [H, B, L] (or [R, L]), reward / terminated [H, B, 1]; task int64 [B] for multitask models (the
        reference broadcasts it over the H leading rows).  `pi_eps` / `qidx` pin the policy noise and the two target heads
        (parity tests); by default they are drawn inside the library."""
        lead = next_z.shape[:-1]
        z2 = next_z.reshape(-1, next_z.shape[-1]).to(self.device, torch.float32).contiguous()
        r2 = reward.reshape(-1).to(self.device, torch.float32).contiguous()
        t2 = terminated.reshape(-1).to(self.device, torch.float32).contiguous()
        kw = {}
        if self.cfg.multitask:
            task = torch.as_tensor(task, device=self.device)
            if next_z.dim() == 3 and task.numel() == next_z.shape[1]:
                task = task.repeat(next_z.shape[0])
            emb, mask, disc = self._task_tables()
            kw = dict(task_ids=task.to(torch.int32).contiguous(), task_emb_table=emb, act_mask_table=mask)
            discount = disc
        else:
            discount = self.discount
        if pi_eps is not None:
            pi_eps = pi_eps.reshape(-1, pi_eps.shape[-1]).to(self.device, torch.float32).contiguous()
        # The host seed is passed by value.  With `native_draws` `_update_model` gives both `pi_eps` and `qidx`, so the kernels read
        # no bit of it -- but the stream that plan() / act() share still advances once per training step, and a capture of this
        # call would bake the value in: harmless only as long as both draws are given.
        self._seed += 1
        td = self.planner().td_target(z2, r2, t2, discount, pi_eps=pi_eps, qidx=qidx, seed=self._seed, **kw)
        return td.reshape(*lead, 1)

    @torch.no_grad()
    def policy_value(self, zs, task=None, reduce="avg", target=False, pi_eps=None, qidx=None):
        """The forward half of `update_pi` (reference tdmpc2.py:208-225): action = pi(zs), q = Q(zs, action, 'avg') on the
        online ensemble -- returned as (action [..., A], q [..., 1]); gradients are outside this package's scope."""
        lead = zs.shape[:-1]
        z2 = zs.reshape(-1, zs.shape[-1]).to(self.device, torch.float32).contiguous()
        kw = {}
        if self.cfg.multitask:
            task = torch.as_tensor(task, device=self.device)
            if zs.dim() == 3 and task.numel() == zs.shape[1]:
                task = task.repeat(zs.shape[0])
            emb, mask, _ = self._task_tables()
            kw = dict(task_ids=task.to(torch.int32).contiguous(), task_emb_table=emb, act_mask_table=mask)
        if pi_eps is not None:
            pi_eps = pi_eps.reshape(-1, pi_eps.shape[-1]).to(self.device, torch.float32).contiguous()
        self._seed += 1
        a, q = self.planner().policy_value(z2, use_target=target, reduce=reduce, pi_eps=pi_eps, qidx=qidx, seed=self._seed, **kw)
        return a.reshape(*lead, -1), q.reshape(*lead, 1)

    # ------------------------------------------------------------------ the rest of _update's forward half
    def _batch_task_kw(self, task):
        """task int64 [B] -> the keyword arguments of the native batch calls (multitask models), else {}."""
        if not self.cfg.multitask:
            return {}
        emb, mask, _ = self._task_tables()
        task = torch.as_tensor(task, device=self.device)
        return dict(task_ids=task.to(torch.int32).contiguous(), task_emb_table=emb, act_mask_table=mask)

    @torch.no_grad()
    def model_rollout(self, z0, actions, task=None, target=False, want=("zs", "reward_logits", "reward", "q_logits", "q")):
        """The open-loop latent rollout of `_update` on recorded actions and the predictions on it (reference tdmpc2.py:268-283)
        in the library: z0 [B, L], actions [H, B, A] -> dict with the keys in `want` out of zs [H+1, B, L], reward_logits
        [H, B, bins], reward [H, B, 1], q_logits [num_q, H, B, bins] (every head: Q(..., return_type='all')), q [num_q, H, B, 1],
        term_logit [H+1, B, 1] (episodic models).  Eval mode: no dropout."""
        z0 = z0.to(self.device, torch.float32).contiguous()
        actions = actions.to(self.device, torch.float32).contiguous()
        return self.planner().model_rollout(z0, actions, use_target=target, want=tuple(want), **self._batch_task_kw(task))

    @torch.no_grad()
    def model_losses_latent(self, z0, next_z, action, reward, td_targets, terminated=None, task=None, want=("zs",),
                            step_means=False):
        """The losses of `_update` (reference tdmpc2.py:285-304) from latents: z0 [B, L] = encode(obs[0]), next_z [H, B, L] =
        encode(obs[1:]), action [H, B, A], reward / td_targets / terminated [H, B, 1].  Returns the reference's keys
        consistency_loss, reward_loss, value_loss, termination_loss, total_loss (0-d tensors) plus the outputs in `want`
        (and step_means [4, H]).  Eval mode: equal to what `_update` logs when cfg.dropout == 0."""
        cfg, dev = self.cfg, self.device
        f = lambda x: None if x is None else x.to(dev, torch.float32).contiguous()
        H, B = action.shape[0], action.shape[1]
        res = self.planner().model_losses(
            f(z0), f(action), f(next_z), f(reward).reshape(H, B), f(td_targets).reshape(H, B),
            None if (terminated is None or not cfg.episodic) else f(terminated).reshape(H, B), rho=cfg.rho,
            coefs=(cfg.consistency_coef, cfg.reward_coef, cfg.value_coef, cfg.termination_coef), want=tuple(want),
            step_means=step_means, **self._batch_task_kw(task))
        losses = res.pop("losses")
        for i, k in enumerate(("consistency_loss", "reward_loss", "value_loss", "termination_loss", "total_loss")):
            res[k] = losses[i]
        return res

    @torch.no_grad()
    def model_losses(self, obs, action, reward, terminated=None, task=None, pi_eps=None, qidx=None, want=("zs",)):
        """The forward half of `_update` (reference tdmpc2.py:259-304) with its argument shapes: obs [H+1, B, *], action
        [H, B, A], reward / terminated [H, B, 1], task [B].  encode(obs[0]), encode(obs[1:]) (state observations in the library;
        pixel observations through the PyTorch-ROCm modules or, with `native_pixel_encoder`, the library's batch route in one
        call), `_td_target`, then the rollout and the losses in one library call.
        Returns the reference's loss keys plus td_targets [H, B, 1] and zs [H+1, B, L]."""
        cfg = self.cfg
        obs = obs.to(self.device)
        H, B = action.shape[0], action.shape[1]
        if terminated is None:
            terminated = torch.zeros(H, B, 1, device=self.device)
        if self.native_encoder and cfg.obs == "state":
            flat = obs.reshape((H + 1) * B, -1).to(torch.float32).contiguous()
            emb = None
            if cfg.multitask:
                t = torch.as_tensor(task, device=self.device).long()
                emb = self.model._task_emb(t.repeat(H + 1)).to(torch.float32).contiguous()
            z_all = self.planner().encode(flat, emb).reshape(H + 1, B, cfg.latent_dim)
        elif self._native_pix():
            z_all = self._encode_pix_batch(obs, H, B)
        else:
            t = None if task is None else torch.as_tensor(task, device=self.device)
            z_all = torch.stack([self.model.encode(obs[i], t) for i in range(H + 1)])
        z0, next_z = z_all[0], z_all[1:].contiguous()
        td = self._td_target(next_z, reward, terminated, task, pi_eps=pi_eps, qidx=qidx)
        res = self.model_losses_latent(z0, next_z, action, reward, td, terminated, task, want=want)
        res["td_targets"] = td
        return res

    # ------------------------------------------------------------------ the model half of _update as one method
    def update_model(self, obs, action, reward, terminated=None, task=None, td_targets=None, pi_eps=None, qidx=None, q_mask=None):
        """The model half of `_update` (reference tdmpc2.py:260-310: everything but `update_pi` and the target-Q soft update), every
        piece in the library: obs [H+1, B, *], action [H, B, A], reward / terminated [H, B, 1], task [B].  In order:
          1. under no_grad, next_z = encode(obs[1:]) and the TD target (`_td_target`, or `td_targets` [H, B, 1] as given; `pi_eps` /
             `qidx` pin its noise and heads, which with `native_draws` come from one `draws.draw([H, B, A], num_q)` made on every
             call, else from the host seed; the target used stays readable as `last_td_targets`);
          2. model.train();
          3. the rollout through `model.next`, then `Q(..., 'all')`, `reward` and (episodic) `termination` under `native_autograd`;
          4. `autograd.model_loss` and `total.backward()`;
          5. `optimizer_step("model")`: clip, Adam, zero_grad and the planner's re-pack;
          6. model.eval().
        Returns consistency_loss, reward_loss, value_loss, termination_loss, total_loss and grad_norm as 0-d device tensors.
        Raises NativeError when `native_autograd` is off: there is no torch path.  The reference's Q heads drop elements of their
        first layer's Linear output in train mode (cfg.dropout): with `native_dropout` step 3's Q pass draws those masks in the library
        (`q_mask` [num_q, H, B, mlp_dim] pins them); with the flag off there is no dropout, and the call equals the reference when
        cfg.dropout == 0.  It also leaves `last_zs` ([H+1, B, L], detached) and, on episodic models, `last_term_logit` ([H, B, 1])."""
        from .native import NativeError
        if not self.native_autograd:
            raise NativeError("update_model runs the model's layers and losses in the library: set native_autograd = True")
        return self._update_model(obs, action, reward, terminated, task, td_targets, pi_eps, qidx, keep_train=False, q_mask=q_mask)

    def _update_model(self, obs, action, reward, terminated, task, td_targets, pi_eps, qidx, keep_train, q_mask=None):
        """`update_model`; keep_train: its step 6 is left to the caller (`_update`, which runs `update_pi` in train mode first)."""
        from . import autograd
        cfg = self.cfg
        obs = obs.to(self.device)
        action = action.to(self.device, torch.float32)
        reward = reward.to(self.device, torch.float32)
        H, B = action.shape[0], action.shape[1]
        if terminated is None:
            terminated = torch.zeros(H, B, 1, device=self.device)
        terminated = terminated.to(self.device, torch.float32)
        if task is not None:
            task = torch.as_tensor(task, device=self.device)
        self.optim  # noqa: B018  (made before backward: every .grad is then a view into its gradient arena)
        if self.native_draws:  # one draw, whatever is pinned: the counter is a function of the step count; a pin overrides its value
            eps, pair = self.draws.draw((H, B, cfg.action_dim), cfg.num_q)
            pi_eps = eps if pi_eps is None else pi_eps
            qidx = pair if qidx is None else qidx
        with torch.no_grad():
            next_z = self.model.encode(obs[1:], task)
            if td_targets is None:
                td_targets = self._td_target(next_z, reward, terminated, task, pi_eps=pi_eps, qidx=qidx)
            td_targets = td_targets.to(self.device, torch.float32).reshape(H, B, 1)
        self.last_td_targets = td_targets
        self.model.train()
        try:
            z = self.model.encode(obs[0], task)
            zs = [z]
            for t in range(H):
                z = self.model.next(z, action[t], task)
                zs.append(z)
            _zs, z_pred = torch.stack(zs[:-1]), torch.stack(zs[1:])
            qs = self.model.Q(_zs, action, task, return_type="all", q_mask=q_mask)
            reward_preds = self.model.reward(_zs, action, task)
            term_pred = self.model.termination(z_pred, task, unnormalized=True) if cfg.episodic else None
            total, parts = autograd.model_loss(cfg, z_pred, next_z, reward_preds, reward, qs, td_targets, term_pred,
                                               terminated if cfg.episodic else None)
            total.backward()
            grad_norm = self.optimizer_step("model").clone()
            self.last_zs = torch.stack(zs).detach()
            self.last_term_logit = None if term_pred is None else term_pred.detach()
        finally:
            if not keep_train:
                self.model.eval()
        return {"consistency_loss": parts[0], "reward_loss": parts[1], "value_loss": parts[2], "termination_loss": parts[3],
                "total_loss": total.detach(), "grad_norm": grad_norm}

    # ------------------------------------------------------------------ the policy half of _update, and _update itself
    def update_pi(self, zs, task=None, pi_eps=None, qidx=None, q_mask=None):
        """`update_pi` of the reference (tdmpc2.py:208-239) in its order, every piece in the library: zs [H+1, B, L] (detached here
        as `_update` detaches it), task [B].
          1. action, info = model.pi(zs, task): the MLP through the trainable layer, its tail through `autograd.PiHeadFn`
             (`pi_eps` [H+1, B, A] pins the noise, else torch.randn_like draws it);
          2. `model.Q_pair` on the online parameters, detached: the two heads `qidx` (drawn with torch.randperm on the device when
             not given), the reference's Q(..., 'avg', detach=True); with `native_draws` the noise and the heads that are not
             pinned come from one `draws.draw([H+1, B, A], num_q)`, made on every call;
          3. `scale.update(qs[0])`, 4. the rho-weighted loss at the updated scale (both inside `autograd.pi_loss`);
          5. `pi_loss.backward()`: the seeds of the loss, the Q pair's dx, the head and `_pi`'s layers, all in HIP;
          6. `optimizer_step("pi")`: clip at cfg.grad_clip_norm, Adam with eps 1e-5, zero_grad and the planner's re-pack.
        Returns pi_loss, pi_grad_norm, pi_entropy, pi_scaled_entropy (means, as `_update` reports them) and pi_scale as 0-d device
        tensors.  The model's mode is left as it is (`_update` calls this in train mode, as the reference does).  Raises
        NativeError when `native_autograd` is off: there is no torch path.  The reference's detached Q copy is a train-mode copy,
        so its first layers drop here too: in train mode with `native_dropout` step 2 draws the two heads' masks in the library
        (`q_mask` [2, H+1, B, mlp_dim] pins them); with the flag off there is no dropout, and the call equals the reference when
        cfg.dropout == 0."""
        from . import autograd
        from .native import NativeError
        if not self.native_autograd:
            raise NativeError("update_pi runs the policy's layers, its head and its loss in the library: set native_autograd = True")
        cfg = self.cfg
        zs = zs.detach().to(self.device, torch.float32)
        if zs.dim() != 3:
            raise NativeError(f"update_pi: zs [H+1, B, L] (got {tuple(zs.shape)})")
        if task is not None:
            task = torch.as_tensor(task, device=self.device)
        if pi_eps is not None:
            pi_eps = pi_eps.to(self.device, torch.float32)
        if self.native_draws:  # one draw, whatever is pinned (see _update_model)
            eps, pair = self.draws.draw((*zs.shape[:2], cfg.action_dim), cfg.num_q)
            pi_eps = eps if pi_eps is None else pi_eps
            qidx = pair if qidx is None else qidx
        if qidx is None:
            qidx = torch.randperm(cfg.num_q, device=self.device)[:2]
        self.pi_optim  # noqa: B018  (made before backward: every .grad of _pi is then a view into its gradient arena)
        action, info = self.model.pi(zs, task, eps=pi_eps)
        q_logits = self.model.Q_pair(zs, action, task, qidx, q_mask=q_mask)
        pi_loss, parts = autograd.pi_loss(cfg, q_logits, info["entropy"], info["scaled_entropy"], self.scale)
        pi_loss.backward()
        pi_grad_norm = self.optimizer_step("pi").clone()
        return {"pi_loss": pi_loss.detach(), "pi_grad_norm": pi_grad_norm.reshape(()), "pi_entropy": parts[0],
                "pi_scaled_entropy": parts[1], "pi_scale": self.scale.value.detach().clone().reshape(())}

    def _update(self, obs, action, reward, terminated=None, task=None, pins=None):
        """`_update` of the reference (tdmpc2.py:259-332): `update_model`, then `update_pi(zs.detach(), task)` with the model still
        in train mode, then `soft_update_target_Q()`, then model.eval() and the reference's info dict as 0-d device tensors
        (consistency_loss, reward_loss, value_loss, termination_loss, total_loss, grad_norm; on episodic models termination_rate and
        termination_f1 of the last step through `termination_stats`; pi_loss, pi_grad_norm, pi_entropy, pi_scaled_entropy,
        pi_scale).  With `native_dropout` (and cfg.dropout > 0) the two train-mode Q passes drop as the reference's do: one `_update`
        makes exactly two mask draws, the value-loss pass first, then `update_pi`'s pair; the TD target draws none (the target
        ensemble is in eval mode in the reference too).  With the flag off there is no dropout, and equality with the reference holds
        for cfg.dropout == 0.  With `native_draws` one `_update` makes exactly two draws from `draws`, the TD target's first, then
        `update_pi`'s, whatever is pinned: no host seed and no framework generator is read.
        `pins` (parity tests): a dict with any of td_pi_eps [H, B, A] / td_qidx (the TD target's noise and heads), td_targets
        [H, B, 1] (the target itself), pi_eps [H+1, B, A] / qidx (`update_pi`'s), q_mask [num_q, H, B, mlp_dim] (the value-loss
        pass's dropout multipliers) and pi_q_mask [2, H+1, B, mlp_dim] (`update_pi`'s); None: every draw is made as before."""
        from .native import NativeError
        if not self.native_autograd:
            raise NativeError("_update runs in the library: set native_autograd = True")
        cfg = self.cfg
        pins = dict(pins or {})
        unknown = set(pins) - {"td_pi_eps", "td_qidx", "td_targets", "pi_eps", "qidx", "q_mask", "pi_q_mask"}
        if unknown:
            raise ValueError(f"_update: unknown pins {sorted(unknown)}")
        if terminated is None:
            terminated = torch.zeros(action.shape[0], action.shape[1], 1, device=self.device)
        try:
            info = self._update_model(obs, action, reward, terminated, task, pins.get("td_targets"), pins.get("td_pi_eps"),
                                      pins.get("td_qidx"), keep_train=True, q_mask=pins.get("q_mask"))
            pi_info = self.update_pi(self.last_zs, task, pi_eps=pins.get("pi_eps"), qidx=pins.get("qidx"), q_mask=pins.get("pi_q_mask"))
            self.soft_update_target_Q()
        finally:
            self.model.eval()
        if cfg.episodic:
            st = self.planner().termination_stats(self.last_term_logit[-1].contiguous(),
                                                  terminated[-1].to(self.device, torch.float32).contiguous())
            info["termination_rate"], info["termination_f1"] = st[0], st[1]
        info.update(pi_info)
        return info

    def update(self, buffer):
        """One training iteration of the reference (tdmpc2.py:334-349): `_update` on `buffer.sample()` (a tdmpc2_amd.Buffer, whose
        batch comes out time-major and on this device)."""
        obs, action, reward, terminated, task = buffer.sample()
        return self._update(obs, action, reward, terminated, task)

    def _encode_pix_batch(self, obs, H, B):
        """encode(obs[i]) for i = 0 .. H in one library call (tdmpc2_plan_encode_pix_batch): ShiftAug's shifts are drawn on the host
        framework's generator once per time step, in the order and with the calls of the module branch."""
        planner = self.planner()
        if planner.__dict__.get("pix_channels") is None:  # flag set after the handle was made
            self._bind_pixel_encoder()
        if planner.pix_batch_chunk < self.pixel_batch_images:  # first use, or the attribute was raised since
            planner.reserve_pix_batch(self.pixel_batch_images)
        if obs.dtype not in (torch.uint8, torch.float32):
            obs = obs.to(torch.float32)
        flat = obs.reshape((H + 1) * B, *obs.shape[2:]).contiguous()
        shift = torch.cat([planner.draw_shift(B, self.device) for _ in range(H + 1)])
        return planner.encode_pix_batch(flat, shift).reshape(H + 1, B, self.cfg.latent_dim)

    # ------------------------------------------------------------------ update_pi's forward and the info dict of _update
    @torch.no_grad()
    def policy_loss(self, zs, task=None, pi_eps=None, qidx=None, update_scale=True, want=()):
        """The forward of `update_pi` (reference tdmpc2.py:208-239) in one library call: action, info = pi(zs), qs = Q(zs, action,
        'avg') on the online ensemble, `self.scale.update(qs[0])` (unless `update_scale` is False), qs / scale and the rho-weighted
        loss.  zs [H+1, B, L], task [B].  Returns pi_loss, pi_entropy, pi_scaled_entropy (means, as `_update` reports them) and
        pi_scale [1] (the scale after the call), plus the outputs in `want` (action, q, entropy, scaled_entropy, step_means,
        percentiles).  Eval mode; no gradients, no optimiser step."""
        cfg = self.cfg
        zs = zs.to(self.device, torch.float32).contiguous()
        if pi_eps is not None:
            pi_eps = pi_eps.to(self.device, torch.float32).contiguous()
        self._seed += 1
        res = self.planner().policy_loss(zs, self.scale.value, rho=cfg.rho, entropy_coef=cfg.entropy_coef, tau=cfg.tau,
                                         update_scale=update_scale, pi_eps=pi_eps, qidx=qidx, seed=self._seed, want=tuple(want),
                                         **self._batch_task_kw(task))
        loss = res.pop("loss")
        res["pi_loss"], res["pi_entropy"], res["pi_scaled_entropy"], res["pi_scale"] = loss[0], loss[1], loss[2], loss[3:4]
        return res

    @torch.no_grad()
    def update_info(self, obs, action, reward, terminated=None, task=None, pi_eps=None, qidx=None):
        """The info dict of `_update` (reference tdmpc2.py:259-331) without `grad_norm` / `pi_grad_norm`: `model_losses`, then (episodic
        models) `termination_statistics` on the last step's termination logit, then `policy_loss` on the rollout's zs.  It equals what
        `_update` returns when no optimiser step is taken between the model loss and `update_pi`, and when cfg.dropout == 0.
        `pi_eps` [H+1, B, A] / `qidx` pin the noise and the two heads of `update_pi` (the TD target draws its own)."""
        cfg = self.cfg
        if cfg.episodic and terminated is None:
            terminated = torch.zeros(action.shape[0], action.shape[1], 1, device=self.device)
        res = self.model_losses(obs, action, reward, terminated, task, want=("zs", "term_logit") if cfg.episodic else ("zs",))
        info = {k: res[k] for k in ("consistency_loss", "reward_loss", "value_loss", "termination_loss", "total_loss")}
        if cfg.episodic:
            st = self.planner().termination_stats(res["term_logit"][-1].contiguous(),
                                                  terminated[-1].to(self.device, torch.float32).contiguous())
            info["termination_rate"], info["termination_f1"] = st[0], st[1]
        pl = self.policy_loss(res["zs"], task, pi_eps=pi_eps, qidx=qidx)
        for k in ("pi_loss", "pi_entropy", "pi_scaled_entropy"):
            info[k] = pl[k]
        info["pi_scale"] = pl["pi_scale"].mean()
        return info

    @torch.no_grad()
    def update_info_sampled(self, buffer, pi_eps=None, qidx=None):
        """`update_info` on a batch drawn from `buffer` (a tdmpc2_amd.Buffer): what the forward of `TDMPC2.update(buffer)` does with
        `buffer.sample()` (reference tdmpc2.py:334-346).  The batch comes out of the library's replay buffer time-major and on
        this device, so nothing runs between the gather and the first encoder launch."""
        obs, action, reward, terminated, task = buffer.sample()
        return self.update_info(obs, action, reward, terminated, task, pi_eps=pi_eps, qidx=qidx)
