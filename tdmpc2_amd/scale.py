"""RunningScale: the running trimmed scale of Q (reference tdmpc2/common/scale.py), updated inside the HIP library.

Same buffers (`value`, `_percentiles`), the same `state_dict` / `load_state_dict` keys and the same `update(x)` /
`forward(x, update=False)` as the reference class; `update` is one call of `tdmpc2_plan_running_scale` (one workgroup: rank
selection of the two percentiles, clamp, lerp).  Only the reference's percentiles 5 / 95 and one column are supported.
"""
from __future__ import annotations

import torch

from .native import RUNNING_SCALE_MAX_N


class RunningScale(torch.nn.Module):
    """Running trimmed scale estimator."""

    def __init__(self, cfg, planner_fn, device):
        """`planner_fn`: callable returning the NativePlanner whose stream / device the update runs on (TDMPC2.planner)."""
        super().__init__()
        self.cfg = cfg
        self._planner_fn = planner_fn
        self.value = torch.nn.Buffer(torch.ones(1, dtype=torch.float32, device=device))
        self._percentiles = torch.nn.Buffer(torch.tensor([5, 95], dtype=torch.float32, device=device))

    def state_dict(self):
        return dict(value=self.value, percentiles=self._percentiles)

    def load_state_dict(self, state_dict):
        pct = torch.as_tensor(state_dict["percentiles"], dtype=torch.float32).flatten().cpu()
        if pct.tolist() != [5.0, 95.0]:
            raise ValueError(f"RunningScale supports the percentiles [5, 95] only; got {pct.tolist()}")
        self.value.copy_(torch.as_tensor(state_dict["value"]).reshape(1))

    @torch.no_grad()
    def update(self, x):
        x = x.detach()
        if x.dim() > 1 and x[0].numel() != 1:
            raise ValueError(f"RunningScale supports one column; got shape {tuple(x.shape)}")
        if x.numel() > RUNNING_SCALE_MAX_N:
            raise ValueError(f"RunningScale.update takes at most {RUNNING_SCALE_MAX_N} values; got {x.numel()}")
        x = x.to(self.value.device, torch.float32).contiguous()
        self._planner_fn().running_scale(x, self.value, tau=self.cfg.tau)

    def forward(self, x, update=False):
        if update:
            self.update(x)
        return x / self.value

    def __repr__(self):
        return f"RunningScale(S: {self.value})"
