"""Replay buffer with the surface of the reference's `Buffer` (tdmpc2/common/buffer.py:13-115) over the library's episode ring
(`tdmpc2_buffer_*`, include/tdmpc2_plan.h): storage, slice sampling and the time-major batch of `_prepare_batch` run in HIP, two
launches per `sample()`.  No torchrl, no tensordict: `td` is any mapping of tensors with the reference's keys.  Storage is device
memory only (the reference falls back to host memory when the GPU is short, buffer.py:61-63; this one raises)."""
from __future__ import annotations

from typing import Optional

import torch

from .native import NativeBuffer, NativeError

# the reference's keys in storage order, with the steps of a slice that _prepare_batch keeps (buffer.py:98-110):
# obs every step, action / reward / terminated [1:], task [0]
_KEYS = ("obs", "action", "reward", "terminated", "task")


class Buffer:
    """`Buffer(cfg, device=None)`: `capacity`, `num_eps`, `add(td)`, `load(td)`, `sample()` as the reference's.

    add takes one episode, tensors [T, ...]; load takes [N, T, ...].  Storage is created from the first episode's shapes and
    dtypes, which are preserved (a row is copied as bytes).  `sample()` draws cfg.batch_size slices of cfg.horizon + 1 steps:
    an eligible episode uniformly, then a start uniformly (the strict-length slice sampler of buffer.py:17-24), Philox keyed by
    `seed` (default cfg.seed) and a call counter that lives on the device -- a `sample()` captured in a graph draws fresh slices
    at every replay."""

    def __init__(self, cfg, device=None, seed: Optional[int] = None):
        self.cfg = cfg
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise NativeError(f"the replay buffer keeps its storage on an MI355X only (device {device}); there is no host storage")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._device = device
        self._capacity = min(int(cfg.buffer_size), int(cfg.steps))  # buffer.py:16
        self._batch = int(cfg.batch_size)
        self._slice = int(cfg.horizon) + 1
        self._seed = int(cfg.seed if seed is None else seed)
        self._num_eps = 0
        self._native: Optional[NativeBuffer] = None
        self._keys = ()
        self._meta = {}  # key -> (dtype, per-step shape)

    @property
    def capacity(self) -> int:
        return self._capacity

    @property
    def num_eps(self) -> int:
        return self._num_eps

    @property
    def native(self) -> Optional[NativeBuffer]:
        return self._native

    # ------------------------------------------------------------------ storage
    def _init(self, td, lead: int):
        """Storage from the first episode's shapes and dtypes (buffer.py:50-67)."""
        keys = tuple(k for k in _KEYS if k in td and td[k] is not None)
        for k in ("obs", "action", "reward"):
            if k not in keys:
                raise KeyError(f"an episode needs '{k}'")
        S = self._slice
        steps = {"obs": (0, S), "action": (1, S - 1), "reward": (1, S - 1), "terminated": (1, S - 1), "task": (0, 1)}
        fields = []
        for k in keys:
            t = td[k]
            shape = tuple(t.shape[lead:])
            n = 1
            for d in shape:
                n *= int(d)
            self._meta[k] = (t.dtype, shape)
            fields.append((n * t.element_size(),) + steps[k])
        self._keys = keys
        self._native = NativeBuffer(self._capacity, S, fields, self._device, max_batch=self._batch)

    def _tensors(self, td, lead: int):
        if self._native is None:
            self._init(td, lead)
        out = []
        for k in self._keys:
            if k not in td or td[k] is None:
                raise KeyError(f"episode without '{k}', which the first episode had")
            dtype, shape = self._meta[k]
            t = td[k]
            if t.dtype != dtype or tuple(t.shape[lead:]) != shape:
                raise ValueError(f"'{k}': expected {dtype} {shape} per step, got {t.dtype} {tuple(t.shape[lead:])}")
            out.append(t.to(self._device).contiguous())
        return out

    def add(self, td) -> int:
        """Add one episode (buffer.py:84-91): tensors [T, ...]."""
        ts = self._tensors(td, 1)  # (creates the storage from the first episode)
        self._native.add(ts)
        self._num_eps += 1
        return self._num_eps

    def load(self, td) -> int:
        """Load N episodes of equal length at once (buffer.py:69-82): tensors [N, T, ...]."""
        ts = self._tensors(td, 2)
        self._native.load(ts)
        self._num_eps += int(ts[0].shape[0])
        return self._num_eps

    # ------------------------------------------------------------------ sampling
    def sample(self, return_index: bool = False):
        """(obs [H+1, B, ...], action [H, B, A], reward [H, B, 1], terminated [H, B, 1], task [B] or None), as `_prepare_batch`
        shapes them (buffer.py:93-115).  return_index: additionally the int64 [B] logical index of step 0 of every slice."""
        if self._native is None:
            raise NativeError("sample() before the first episode: the buffer has no storage yet")
        B, H = self._batch, self._slice - 1
        lead = {"obs": (H + 1, B), "action": (H, B), "reward": (H, B), "terminated": (H, B), "task": (B,)}
        outs = {k: torch.empty(lead[k] + self._meta[k][1], dtype=self._meta[k][0], device=self._device) for k in self._keys}
        index = torch.empty(B, dtype=torch.int64, device=self._device) if return_index else None
        self._native.sample([outs[k] for k in self._keys], seed=self._seed, index_out=index)
        reward = outs["reward"].reshape(H, B, 1)
        terminated = outs["terminated"].reshape(H, B, 1) if "terminated" in outs else torch.zeros_like(reward)
        batch = (outs["obs"], outs["action"], reward, terminated, outs.get("task"))
        return batch + (index,) if return_index else batch
