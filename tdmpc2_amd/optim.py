"""ClipAdam: `clip_grad_norm_` + `torch.optim.Adam` + `zero_grad` of the learner (reference tdmpc2/tdmpc2.py:22-31, 227-230,
307-310) as one library call of three launches (include/tdmpc2_plan.h: tdmpc2_optim_*).

The gradients and both moments of all parameters live in three flat fp32 arenas; every `p.grad` is a view into the gradient arena,
so autograd accumulates in place and the pointers the library holds stay fixed.  Every parameter is stepped on every call: a
gradient that backward left at zero counts as a zero gradient (the reference's optimisers see a gradient for each of their
parameters on every step).  No weight decay, amsgrad or maximize.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, List

import torch

from .native import NativeError, NativeOptim


class ClipAdam:
    def __init__(self, param_groups, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, max_norm: float = float("inf")):
        """param_groups as for torch.optim.Adam: an iterable of parameters, or a list of dicts with `params` and an optional `lr`
        (a group may be empty).  max_norm: clip_grad_norm_'s, over all parameters of this optimiser."""
        groups = list(param_groups)
        if not groups or not isinstance(groups[0], dict):
            groups = [{"params": groups}]
        self.param_groups: List[Dict] = [{"params": list(g["params"]), "lr": float(g.get("lr", lr))} for g in groups]
        self.betas, self.eps, self.max_norm = (float(betas[0]), float(betas[1])), float(eps), float(max_norm)
        self.params = [p for g in self.param_groups for p in g["params"]]
        if not self.params:
            raise NativeError("ClipAdam: no parameters")
        if len({id(p) for p in self.params}) != len(self.params):
            raise NativeError("ClipAdam: a parameter appears in more than one group")
        device = self.params[0].device
        for p in self.params:
            if p.device.type != "cuda":
                raise NativeError(f"ClipAdam runs on an MI355X only (parameter on {p.device}); there is no CPU fallback")
            if p.device != device or p.dtype != torch.float32 or not p.is_contiguous():
                raise NativeError(f"ClipAdam: parameters must be contiguous fp32 tensors on one device ({p.dtype}, {p.device}, "
                                  f"contiguous={p.is_contiguous()})")
        self.device = device
        segs = [(p.data_ptr(), p.numel(), gi) for gi, g in enumerate(self.param_groups) for p in g["params"]]
        # max_norm = inf (no clipping) is a clip coefficient of 1 for every finite norm: the largest finite fp32 says the same
        clip = min(self.max_norm, float(torch.finfo(torch.float32).max))
        self._native = NativeOptim(segs, [g["lr"] for g in self.param_groups], self.betas[0], self.betas[1], self.eps, clip, device)
        self.offsets, n = self._native.offsets, self._native.arena_floats
        self.grad = torch.zeros(n, dtype=torch.float32, device=device)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=device)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=device)
        self.grad_norm = torch.zeros((), dtype=torch.float32, device=device)  # rewritten by every step
        for p, off in zip(self.params, self.offsets):
            p.grad = self.grad[off:off + p.numel()].view_as(p)
        self._grad_ptrs = [p.grad.data_ptr() for p in self.params]

    def step(self, zero_grad: bool = True) -> torch.Tensor:
        """Clip, step and (by default) zero the gradients on the current stream; returns the 0-d device tensor `grad_norm` (the norm
        before clipping, as clip_grad_norm_ returns it; the same tensor on every call).  zero_grad = False leaves the CLIPPED
        gradients in place, as torch's clip does."""
        for p, ptr in zip(self.params, self._grad_ptrs):
            if p.grad is None or p.grad.data_ptr() != ptr:
                raise NativeError("ClipAdam: a parameter's .grad was replaced (zero_grad(set_to_none=True)?); the gradients "
                                  "live in the optimiser's arena and are zeroed by step()")
        self._native.step(self.grad, self.exp_avg, self.exp_avg_sq, zero_grad, self.grad_norm)
        return self.grad_norm

    def zero_grad(self):
        self.grad.zero_()

    def state_dict(self) -> dict:
        return {"step": self._native.get_step(), "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
                "offsets": list(self.offsets)}

    def load_state_dict(self, sd: dict):
        if list(sd["offsets"]) != list(self.offsets) or sd["exp_avg"].numel() != self.exp_avg.numel():
            raise NativeError("ClipAdam.load_state_dict: the saved arenas have another layout")
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self._native.set_step(int(sd["step"]))

    def close(self):
        self._native.close()
