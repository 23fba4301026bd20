"""Run the REFERENCE's own planner code, verbatim, on CPU.  TEST INFRASTRUCTURE ONLY.

Works only where `/root/reference` exists (the build container).  Nothing is
copied: the reference's modules are imported from where they lie, with a stub
`tensordict` in `sys.modules` (the real package is absent and is used by the
planner only for parameter stacking).  Recipe: SURVEY.md Appendix A.

Executed verbatim from the reference: `TDMPC2._plan`, `TDMPC2._estimate_value`
(tdmpc2/tdmpc2.py:122-206), `WorldModel.{task_emb,encode,next,reward,
termination,pi,Q}` (tdmpc2/common/world_model.py:88-216), `layers.mlp /
NormedLinear / SimNorm / enc` (tdmpc2/common/layers.py:74-164) and
`common.math` (tdmpc2/common/math.py).  The only restated piece is the Q
`Ensemble` container (layers.py:8-33 needs real tensordict): the same vmap over
stacked parameters via `torch.func`.

RNG: the six draw sites are served from a noise tape by
patching `torch.randn`, `torch.randn_like`, `torch.randperm` and
`Tensor.exponential_` while `_plan` runs — reference code untouched.
Per-iteration locals (value, elite idx, score, mean, std) are read with
`sys.settrace`, again without touching the reference.

Training side: `run_reference_updates` runs `TDMPC2._update`, `update_pi` and
`_td_target` (tdmpc2/tdmpc2.py:208-332) verbatim in the same way; what it has
to restate (the optimisers, RunningScale's constructor, the soft update,
`_detach_Qs`) is listed in its docstring.
"""
from __future__ import annotations

import copy
import inspect
import os
import sys
import types
from typing import Dict, Optional

import torch
import torch.nn as nn

REF_ROOT = os.environ.get("TDMPC2_REFERENCE", "/root/reference")


def available() -> bool:
    return os.path.isdir(os.path.join(REF_ROOT, "tdmpc2", "common"))


_ref = None


def _import_reference():
    global _ref
    if _ref is not None:
        return _ref
    if not available():
        raise RuntimeError(f"reference tree not found at {REF_ROOT}")
    td = types.ModuleType("tensordict")
    td.from_modules = None
    td.TensorDict = dict  # pi() builds TensorDict({...}); a dict is enough
    tdn = types.ModuleType("tensordict.nn")
    tdn.TensorDictParams = object
    sys.modules.setdefault("tensordict", td)
    sys.modules.setdefault("tensordict.nn", tdn)
    path = os.path.join(REF_ROOT, "tdmpc2")
    saved = list(sys.path)
    saved_mods = {k: sys.modules.get(k) for k in ("common", "tdmpc2")}
    sys.path.insert(0, path)
    try:
        for k in [m for m in sys.modules if m == "common" or m.startswith("common.")]:
            del sys.modules[k]
        import importlib

        layers = importlib.import_module("common.layers")
        rmath = importlib.import_module("common.math")
        wm = importlib.import_module("common.world_model")
        # `tdmpc2` here is the reference's tdmpc2/tdmpc2.py module
        spec = importlib.util.spec_from_file_location("_ref_tdmpc2_module", os.path.join(path, "tdmpc2.py"))
        # tdmpc2.py imports common.scale (hard-codes cuda in its ctor only; import is fine)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path[:] = saved
    _ref = types.SimpleNamespace(layers=layers, math=rmath, WorldModel=wm.WorldModel, TDMPC2=mod.TDMPC2)
    return _ref


class _Ens(nn.Module):
    """Stand-in for layers.Ensemble (layers.py:8-33): vmap over stacked params."""

    def __init__(self, mods):
        super().__init__()
        from torch.func import stack_module_state

        p, _ = stack_module_state(mods)
        self.base = copy.deepcopy(mods[0]).to("meta")
        self.p = nn.ParameterDict({k.replace(".", "__"): nn.Parameter(v) for k, v in p.items()})

    def forward(self, x):
        from torch.func import functional_call

        P = {k.replace("__", "."): v for k, v in self.p.items()}
        return torch.vmap(lambda p, x: functional_call(self.base, (p,), (x,)), (0, None), randomness="different")(P, x)


class _DetachedEns(nn.Module):
    """`_detach_Qs` (world_model.py:40: `_Qs.params.data`): the online ensemble's values, cut from autograd.  The ensemble it reads
    is no registered child, so the parameters stay `_Qs`'s alone and a backward through this module never reaches them."""

    def __init__(self, ens):
        super().__init__()
        self.__dict__["ens"] = ens

    def forward(self, x):
        from torch.func import functional_call

        P = {k.replace("__", "."): v.detach() for k, v in self.ens.p.items()}
        return torch.vmap(lambda p, x: functional_call(self.ens.base, (p,), (x,)), (0, None), randomness="different")(P, x)


def build_agent(cfg, state_dict: Dict[str, torch.Tensor], discount):
    """Duck-typed host objects carrying the reference's unbound methods."""
    ref = _import_reference()
    layers, WorldModel, TDMPC2 = ref.layers, ref.WorldModel, ref.TDMPC2

    class WM(nn.Module):
        def __init__(s):
            super().__init__()
            s.cfg = cfg
            D = cfg.latent_dim + cfg.action_dim + cfg.task_dim
            if cfg.multitask:
                s._task_emb = nn.Embedding(len(cfg.tasks), cfg.task_dim, max_norm=1)
                s.register_buffer("_action_masks", torch.zeros(len(cfg.tasks), cfg.action_dim))
            s._encoder = layers.enc(cfg, out={})
            s._dynamics = layers.mlp(D, 2 * [cfg.mlp_dim], cfg.latent_dim, act=layers.SimNorm(cfg))
            s._reward = layers.mlp(D, 2 * [cfg.mlp_dim], max(cfg.num_bins, 1))
            s._termination = layers.mlp(cfg.latent_dim + cfg.task_dim, 2 * [cfg.mlp_dim], 1) if cfg.episodic else None
            s._pi = layers.mlp(cfg.latent_dim + cfg.task_dim, 2 * [cfg.mlp_dim], 2 * cfg.action_dim)
            s._Qs = _Ens([layers.mlp(D, 2 * [cfg.mlp_dim], max(cfg.num_bins, 1), dropout=cfg.dropout)
                          for _ in range(cfg.num_q)])
            # the target / detached ensembles of world_model.py:38-53 (there: deep copies of _Qs holding separate
            # parameter sets); WorldModel.Q picks one by its `target` / `detach` flags (world_model.py:201-206)
            s._target_Qs = _Ens([layers.mlp(D, 2 * [cfg.mlp_dim], max(cfg.num_bins, 1), dropout=cfg.dropout)
                                 for _ in range(cfg.num_q)])
            s._detach_Qs = _DetachedEns(s._Qs)
            s.register_buffer("log_std_min", torch.tensor(float(cfg.log_std_min)))
            s.register_buffer("log_std_dif", torch.tensor(float(cfg.log_std_max)) - s.log_std_min)

    for m in ["task_emb", "encode", "next", "reward", "termination", "pi", "Q"]:
        setattr(WM, m, getattr(WorldModel, m))

    class Agent(nn.Module):
        def __init__(s):
            super().__init__()
            s.cfg = cfg
            s.device = torch.device("cpu")
            s.model = WM().eval()
            s.discount = discount
            s._prev_mean = torch.nn.Buffer(torch.zeros(cfg.horizon, cfg.action_dim))

    Agent._plan = TDMPC2._plan
    Agent._estimate_value = TDMPC2._estimate_value
    Agent._td_target = TDMPC2._td_target
    Agent._update = TDMPC2._update
    Agent.update_pi = TDMPC2.update_pi
    agent = Agent()
    # load weights (checkpoint keys -> host modules)
    own = agent.model.state_dict()
    with torch.no_grad():
        for k, v in state_dict.items():
            if k.startswith("_Qs.params."):
                kk = "_Qs.p." + k[len("_Qs.params."):].replace(".", "__")
            elif k.startswith("_target_Qs_params."):
                kk = "_target_Qs.p." + k[len("_target_Qs_params."):].replace(".", "__")
            elif k.startswith("_detach_Qs_params."):
                continue  # an alias of _Qs.params in the reference (world_model.py:40)
            else:
                kk = k
            if kk not in own:
                raise KeyError(f"{k} -> {kk} not in reference host model")
            own[kk].copy_(torch.as_tensor(v))
    return agent


class TapePlayer:
    """Serves the reference's RNG calls from a per-env tape, in call order."""

    def __init__(self, cfg, tape: Dict[str, torch.Tensor], iterations: int, eval_mode: bool):
        self.q = []
        H = cfg.horizon
        if cfg.num_pi_trajs > 0:
            for t in range(H):
                self.q.append(("randn_like", tape["pi_traj_eps"][t]))
        for it in range(iterations):
            self.q.append(("randn", tape["sample_eps"][it]))
            self.q.append(("randn_like", tape["pi_eps"][it]))
            self.q.append(("randperm", tape["qidx"][it]))
        self.q.append(("exponential_", tape["gumbel_exp"]))
        if not eval_mode:
            self.q.append(("randn", tape["final_eps"]))
        self.pos = 0
        self.num_q = cfg.num_q

    def _next(self, kind, shape=None):
        k, v = self.q[self.pos]
        assert k == kind, f"RNG call #{self.pos}: reference called {kind}, tape expected {k}"
        if shape is not None:
            assert tuple(v.shape) == tuple(shape), f"RNG call #{self.pos} ({kind}): shape {tuple(shape)} vs tape {tuple(v.shape)}"
        self.pos += 1
        return torch.as_tensor(v).clone()

    def __enter__(self):
        self._saved = (torch.randn, torch.randn_like, torch.randperm, torch.Tensor.exponential_)
        player = self

        def randn(*size, **kw):
            if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
                size = tuple(size[0])
            return player._next("randn", size).to(torch.float32)

        def randn_like(x, **kw):
            return player._next("randn_like", x.shape).to(x.dtype)

        def randperm(n, **kw):
            first = player._next("randperm").long()
            rest = torch.tensor([i for i in range(n) if i not in first.tolist()], dtype=torch.long)
            return torch.cat([first, rest])

        def exponential_(self_t, *a, **kw):
            self_t.copy_(player._next("exponential_", self_t.shape))
            return self_t

        torch.randn, torch.randn_like, torch.randperm = randn, randn_like, randperm
        torch.Tensor.exponential_ = exponential_
        return self

    def __exit__(self, *exc):
        torch.randn, torch.randn_like, torch.randperm, torch.Tensor.exponential_ = self._saved
        if exc[0] is None:
            assert self.pos == len(self.q), f"reference consumed {self.pos} of {len(self.q)} tape entries"
        return False


def run_reference_td_target(cfg, state_dict, *, next_z, reward, terminated, task, discount, pi_eps, qidx):
    """Call the reference's `TDMPC2._td_target` (tdmpc2/tdmpc2.py:239-254) once with its two RNG draws (the policy's
    randn_like, world_model.py:156, and Q's randperm, world_model.py:212) served from the arguments.
    next_z [H, B, L], reward / terminated [H, B, 1]; `discount` = what the reference holds in self.discount."""
    agent = build_agent(cfg, state_dict, discount)
    saved = (torch.randn_like, torch.randperm)

    def randn_like(x, **kw):
        assert tuple(x.shape) == tuple(pi_eps.shape)
        return torch.as_tensor(pi_eps).to(x.dtype).clone()

    def randperm(n, **kw):
        first = torch.as_tensor(qidx).long()
        rest = torch.tensor([i for i in range(n) if i not in first.tolist()], dtype=torch.long)
        return torch.cat([first, rest])

    torch.randn_like, torch.randperm = randn_like, randperm
    try:
        with torch.no_grad():
            task_t = None if task is None else torch.as_tensor(task)
            return agent._td_target(torch.as_tensor(next_z), torch.as_tensor(reward), torch.as_tensor(terminated), task_t)
    finally:
        torch.randn_like, torch.randperm = saved


UPDATE_CONTROLS = ("enc_lr", "pi_eps", "no_emb_leak", "no_soft_update", "soft_update_first", "stale_pi_td", "soft_update_before_step")


def run_reference_updates(cfg, state_dict, batch, pins, iterations, dtype, scale0, control=None):
    """Call the reference's `TDMPC2._update` (tdmpc2/tdmpc2.py:259-332; `update_pi` :208-239 and `_td_target` :241-257 under it)
    `iterations` times on one batch, verbatim, on the CPU in `dtype`.

    batch: obs [H+1, B, *], action [H, B, A], reward [H, B, 1], terminated [H, B, 1] or None, task [B] or None.
    pins: td_pi_eps [K, H, B, A], td_qidx [K, 2], pi_eps [K, H+1, B, A], qidx [K, 2] -- the four RNG draws of an iteration
    (`randn_like` world_model.py:156 and `randperm` world_model.py:212, once under `_td_target` and once under `update_pi`), served by
    patching `torch.randn_like` / `torch.randperm` while `_update` runs.
    Returns {"infos": one dict of python floats per iteration, "td": [K, H, B, 1] `_update`'s own `td_targets`, "term_logit":
    [K, B, 1] its `termination_pred[-1]` (episodic models, else None)}; both read from `_update`'s locals with `sys.settrace`.

    Restated, because the reference's own cannot be imported as it is (nothing else is):
      - the two optimisers of tdmpc2.py:22-31 (there with `capturable=True`, which is for CUDA graphs);
      - `RunningScale` (common/scale.py:8-12: the constructor hard-codes cuda:0): made without it, with `cfg`, `value` = scale0 and
        `_percentiles` = [5, 95] on the CPU, both in `dtype`; its methods are the reference's;
      - `soft_update_target_Q` (world_model.py:82-86; needs tensordict): the lerp of the stacked target parameters towards the
        online ones;
      - `_detach_Qs` (world_model.py:40): `_DetachedEns`;
      - `_action_masks` (world_model.py:22-24): loaded from the state dict.
    cfg.dropout is 0 (the port's Q ensemble has none) and cfg.batch_size the batch's B.  Every hyperparameter the C ABI carries as
    fp32 reaches the reference widened (tests.optim_common.widen): lr, the encoder's lr, both betas, both eps,
    grad_clip_norm, rho, tau, entropy_coef and the four loss coefficients.  fp64 runs happen under
    `torch.set_default_dtype(torch.float64)`: `_update` allocates `zs` with the default dtype.

    control: one deliberately WRONG variant (UPDATE_CONTROLS), each in a restated piece or in a hook between the verbatim calls --
    enc_lr: the encoder group at the plain lr; pi_eps: pi_optim's eps 1e-8; no_emb_leak: `_task_emb.weight.grad` cleared after
    `update_pi`; no_soft_update; soft_update_first: the target lerped before `update_pi`; stale_pi_td: `_td_target` evaluated on
    the `_pi` of one iteration earlier; soft_update_before_step: the target lerped before the model optimiser's step, towards the
    online parameters of before it.  (`soft_update_first` commutes with `update_pi` -- one writes `_pi`, the other the target, both
    only read the online Q -- and so reproduces the verbatim run bit for bit; `soft_update_before_step` is the order that is wrong.)"""
    import numpy as np

    from tdmpc2_amd.config import get_discount
    from tests.optim_common import widen as w

    assert control is None or control in UPDATE_CONTROLS, control
    ref = _import_reference()
    K = int(iterations)
    H, B, A = cfg.horizon, int(batch["action"].shape[1]), cfg.action_dim
    enc_lr = w(cfg.lr * cfg.enc_lr_scale)  # the product the port's optimiser forms (tdmpc2.py:23), then fp32
    cfg = cfg.replace(dropout=0.0, batch_size=B, lr=w(cfg.lr), grad_clip_norm=w(cfg.grad_clip_norm), rho=w(cfg.rho), tau=w(cfg.tau),
                      entropy_coef=w(cfg.entropy_coef), consistency_coef=w(cfg.consistency_coef), reward_coef=w(cfg.reward_coef),
                      value_coef=w(cfg.value_coef), termination_coef=w(cfg.termination_coef))
    lr = cfg.lr
    saved_dtype = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        if cfg.multitask:  # tdmpc2.py:35-37: an fp32 tensor there
            discount = torch.tensor([get_discount(cfg, n) for n in cfg.episode_lengths], dtype=torch.float32).to(dtype)
        else:
            discount = get_discount(cfg, cfg.episode_length)
        agent = build_agent(cfg, state_dict, discount).to(dtype)
        m = agent.model
        if cfg.multitask:
            assert torch.equal(m._action_masks, torch.as_tensor(state_dict["_action_masks"]).to(dtype))
        # ---- restated: tdmpc2.py:22-31 without capturable
        betas = (w(0.9), w(0.999))
        agent.optim = torch.optim.Adam([
            {"params": m._encoder.parameters(), "lr": lr if control == "enc_lr" else enc_lr},
            {"params": m._dynamics.parameters()},
            {"params": m._reward.parameters()},
            {"params": m._termination.parameters() if cfg.episodic else []},
            {"params": m._Qs.parameters()},
            {"params": m._task_emb.parameters() if cfg.multitask else []},
        ], lr=lr, betas=betas, eps=w(1e-8))
        agent.pi_optim = torch.optim.Adam(m._pi.parameters(), lr=lr, betas=betas, eps=w(1e-8 if control == "pi_eps" else 1e-5))
        # ---- restated: common/scale.py:8-12 without the constructor
        RunningScale = sys.modules["common.scale"].RunningScale
        scale = RunningScale.__new__(RunningScale)
        nn.Module.__init__(scale)
        scale.cfg = cfg
        scale.value = torch.nn.Buffer(torch.full((1,), float(scale0), dtype=dtype))
        scale._percentiles = torch.nn.Buffer(torch.tensor([5, 95], dtype=dtype))
        agent.scale = scale

        # ---- restated: world_model.py:82-86
        def soft_update_target_Q():
            with torch.no_grad():
                for k in m._Qs.p:
                    m._target_Qs.p[k].lerp_(m._Qs.p[k], cfg.tau)

        moved = ("no_soft_update", "soft_update_first", "soft_update_before_step")
        m.soft_update_target_Q = (lambda: None) if control in moved else soft_update_target_Q
        # ---- hooks between the verbatim calls (controls only)
        if control == "soft_update_first":
            def update_pi(zs, task):
                soft_update_target_Q()
                return ref.TDMPC2.update_pi(agent, zs, task)

            agent.update_pi = update_pi
        if control == "soft_update_before_step":
            step = agent.optim.step

            def step_after_lerp(*a, **kw):
                soft_update_target_Q()
                return step(*a, **kw)

            agent.optim.step = step_after_lerp
        pi_at_start = []  # _pi's parameters at the start of every iteration
        if control == "stale_pi_td":
            def _td_target(next_z, reward, terminated, task):
                now = [p.detach().clone() for p in m._pi.parameters()]
                with torch.no_grad():
                    for p, old in zip(m._pi.parameters(), pi_at_start[max(len(pi_at_start) - 2, 0)]):
                        p.copy_(old)
                    try:
                        return ref.TDMPC2._td_target(agent, next_z, reward, terminated, task)
                    finally:
                        for p, cur in zip(m._pi.parameters(), now):
                            p.copy_(cur)

            agent._td_target = _td_target

        f = lambda x: None if x is None else torch.as_tensor(np.asarray(x)).to(dtype)  # noqa: E731
        obs, action, reward = f(batch["obs"]), f(batch["action"]), f(batch["reward"])
        terminated = f(batch.get("terminated"))
        if terminated is None:
            terminated = torch.zeros(H, B, 1, dtype=dtype)
        task = None if batch.get("task") is None else torch.as_tensor(np.asarray(batch["task"])).long()
        assert obs.shape[:2] == (H + 1, B) and action.shape == (H, B, A) and reward.shape == (H, B, 1) and terminated.shape == (H, B, 1)

        update_code = getattr(ref.TDMPC2._update, "__wrapped__", ref.TDMPC2._update).__code__
        seen = {}

        def tracer(frame, event, arg):
            if frame.f_code is not update_code:
                return None

            def local(frame, event, arg):
                if event == "return":
                    seen["td"] = frame.f_locals["td_targets"].detach().clone()
                    if cfg.episodic:
                        seen["term"] = frame.f_locals["termination_pred"][-1].detach().clone()
                return local

            return local

        infos, tds, terms = [], [], []
        saved = (torch.randn_like, torch.randperm)
        for k in range(K):
            draws = [("randn_like", pins["td_pi_eps"][k], (H, B, A)), ("randperm", pins["td_qidx"][k], (2,)),
                     ("randn_like", pins["pi_eps"][k], (H + 1, B, A)), ("randperm", pins["qidx"][k], (2,))]
            for kind, v, shape in draws:
                assert tuple(np.shape(v)) == shape, (k, kind, np.shape(v), shape)

            def draw(kind, shape=None):
                assert draws and draws[0][0] == kind, f"iteration {k}: the reference called {kind}, expected {draws[0][0] if draws else 'nothing'}"
                _, v, want = draws.pop(0)
                assert shape is None or tuple(shape) == want, (k, kind, tuple(shape), want)
                return torch.as_tensor(np.asarray(v))

            def randn_like(x, **kw):
                return draw("randn_like", x.shape).to(x.dtype).clone()

            def randperm(n, **kw):
                first = draw("randperm").long()
                rest = torch.tensor([i for i in range(n) if i not in first.tolist()], dtype=torch.long)
                return torch.cat([first, rest])

            pi_at_start.append([p.detach().clone() for p in m._pi.parameters()])
            seen.clear()
            torch.randn_like, torch.randperm = randn_like, randperm
            sys.settrace(tracer)
            try:
                info = agent._update(obs, action, reward, terminated, task)
            finally:
                sys.settrace(None)
                torch.randn_like, torch.randperm = saved
            assert not draws, f"iteration {k}: the reference consumed {4 - len(draws)} of 4 draws"
            if control == "no_emb_leak" and cfg.multitask:
                m._task_emb.weight.grad = None
            assert not m.training
            infos.append({n: float(v) for n, v in info.items()})
            tds.append(seen["td"])
            terms.append(seen.get("term"))
        return {"infos": infos, "td": torch.stack(tds).numpy(),
                "term_logit": torch.stack(terms).numpy() if cfg.episodic else None}
    finally:
        torch.set_default_dtype(saved_dtype)


def run_reference_plan(cfg, state_dict, *, obs=None, z0=None, tape, prev_mean, t0, eval_mode, task, discount,
                       iterations):
    """Call the reference's `_plan` once.  If `z0` is given, `encode` is
    bypassed (the planner is benchmarked on synthetic latents) by handing the
    model an `encode` that returns it.  Returns (action, new_prev_mean, stages)."""
    agent = build_agent(cfg, state_dict, discount)
    cfg_run = copy.copy(cfg)
    cfg_run.iterations = iterations
    agent.cfg = cfg_run
    agent.model.cfg = cfg_run
    with torch.no_grad():
        agent._prev_mean.copy_(torch.as_tensor(prev_mean))
    if z0 is not None:
        zz = torch.as_tensor(z0).reshape(1, -1).clone()
        agent.model.encode = lambda o, tk: zz
        obs = torch.zeros(1, 1)
    else:
        obs = torch.as_tensor(obs).reshape(1, -1)
    task_t = None if task is None else torch.tensor([task])

    plan_code = agent._plan.__func__.__wrapped__.__code__ if hasattr(agent._plan.__func__, "__wrapped__") \
        else agent._plan.__func__.__code__
    snaps = []

    def tracer(frame, event, arg):
        if frame.f_code is not plan_code:
            return None

        def local(frame, event, arg):
            if event == "line":
                loc = frame.f_locals
                src_line = lines[frame.f_lineno - first].strip()
                # `std` is final for an iteration when control is back at the loop
                # header (next iteration / exit check) or at the first line after the loop.
                at_header = src_line.startswith("for _ in range")
                at_exit = src_line.startswith("rand_idx")
                if "score" in loc and "elite_idxs" in loc and (at_header or (at_exit and len(snaps) < iterations)):
                    snaps.append({k: loc[k].detach().clone() for k in
                                  ("value", "elite_idxs", "score", "mean", "std", "actions")})
            return local

        return local

    src, first = inspect.getsourcelines(ref_plan_function())
    lines = src
    with TapePlayer(cfg_run, tape, iterations, eval_mode):
        sys.settrace(tracer)
        try:
            with torch.no_grad():
                a = agent._plan(obs, t0=t0, eval_mode=eval_mode, task=task_t)
        finally:
            sys.settrace(None)
    assert len(snaps) == iterations, f"captured {len(snaps)} iteration snapshots, expected {iterations}"
    stages = {
        "value": torch.stack([s["value"].squeeze(1) for s in snaps]),
        "elite_idx": torch.stack([s["elite_idxs"] for s in snaps]),
        "score": torch.stack([s["score"].squeeze(1) for s in snaps]),
        "mean": torch.stack([s["mean"] for s in snaps]),
        "std": torch.stack([s["std"] for s in snaps]),
        "actions": torch.stack([s["actions"] for s in snaps]),
    }
    return a.detach().clone(), agent._prev_mean.detach().clone(), stages


def time_reference_plan(cfg, state_dict, *, z0, tape, task, discount, iterations, budget_s=6.0, min_plans=3):
    """Wall time per call of the reference's `_plan` run verbatim (no line tracer, the agent built once, the recorded noise
    replayed per call) -- bench.py's measured `port_vs_reference` when the reference tree is on the machine.
    Returns (ms per plan, plans timed)."""
    import time

    agent = build_agent(cfg, state_dict, discount)
    cfg_run = copy.copy(cfg)
    cfg_run.iterations = iterations
    agent.cfg = cfg_run
    agent.model.cfg = cfg_run
    zz = torch.as_tensor(z0).reshape(1, -1).clone()
    agent.model.encode = lambda o, tk: zz
    obs = torch.zeros(1, 1)
    task_t = None if task is None else torch.tensor([task])

    def one(t0):
        with TapePlayer(cfg_run, tape, iterations, False):
            with torch.no_grad():
                agent._plan(obs, t0=t0, eval_mode=False, task=task_t)

    one(True)
    n, t_start = 0, time.perf_counter()
    while n < min_plans or time.perf_counter() - t_start < budget_s:
        one(False)
        n += 1
    return 1e3 * (time.perf_counter() - t_start) / n, n


def ref_plan_function():
    ref = _import_reference()
    f = ref.TDMPC2._plan
    return getattr(f, "__wrapped__", f)
