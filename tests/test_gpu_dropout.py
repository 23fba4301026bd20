"""GPU: the dropout-mask unit (tdmpc2_dropout_mask, autograd.DropoutMasks), the mask argument of autograd.ensemble_apply, the mode logic
of WorldModel.Q / Q_pair under `native_dropout`, and TDMPC2._update / update with the two train-mode Q passes dropping.

Bit checks compare the kernel with the numpy restatement of tests/dropout_common.py.  Gates: e <= MARGIN * max(e_ref32,
FLOOR), e = max |T - T64| / max |T64| per tensor (per info key: |x - x64| / |x64|); for the fixture e_ref32 is the reference's own fp32
run (tests/golden/q_dropout.npz), for `_update` a torch-only fp32 path of the port beside its fp64 path.  Worst ratios go to the file
TDMPC2_DROPOUT_JSON names (profiles/dropout_edges.json).  Nothing here reads the reference tree."""
import json
import os

import numpy as np
import pytest
import torch

from tests import dropout_common as dc
from tests import loss_grad_common as lc
from tests import update_common as uc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = 64  # floats behind every mask
SENTINEL = -777.25
SEEDS = dc.FREQ_SEEDS


def _merge_json(key, value):
    path = os.environ.get("TDMPC2_DROPOUT_JSON")
    if not path:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.setdefault("gate", "e <= 4 * max(e_ref32, 2^-23) per tensor (per info key), against fp64; values are the worst e / max(e_ref32, 2^-23)")
    doc[key] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def _state(words):
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32, device=DEV)


def _counter(state):
    lo, hi = (int(v) & 0xFFFFFFFF for v in state.tolist())
    return (hi << 32) | lo


# ---------------------------------------------------------------- 1. the kernel against the restatement, bit for bit
@pytest.mark.parametrize("p", (0.0, 0.01, 0.25, 0.9))
def test_mask_equals_the_restatement_bit_for_bit(p):
    from tdmpc2_amd import native

    seed = SEEDS[1]
    keep = dc.keep_of(p)
    calls0 = native.DROPOUT_CALLS
    start = 0xFFFFFFFE  # the device counter crosses the carry on its second call
    state = _state((start & 0xFFFFFFFF, start >> 32))
    k = 0
    for n in dc.SIZES + (dc.FREQ_N, dc.PAST_ONE_PASS):
        # host counter (state NULL): the descriptor's call counter, both words in use
        call = 0x0000000300000000 + n
        buf = torch.full((n + GUARD,), SENTINEL, device=DEV)
        native.dropout_mask(native.dropout_desc(n, p, seed, call), None, buf)
        got = buf.cpu().numpy()
        assert got[:n].tobytes() == dc.mask_model(n, p, seed, call).tobytes(), (n, "host counter")
        assert (got[n:] == SENTINEL).all(), (n, "guard")
        assert set(np.unique(got[:n]).tolist()) <= {0.0, float(keep)} and not np.signbit(got[:n]).any()
        # device counter: read from state (the descriptor's is ignored), then advanced by one
        buf.fill_(SENTINEL)
        native.dropout_mask(native.dropout_desc(n, p, seed, 12345), state, buf)
        got = buf.cpu().numpy()
        assert got[:n].tobytes() == dc.mask_model(n, p, seed, start + k).tobytes(), (n, "device counter", k)
        assert (got[n:] == SENTINEL).all(), (n, "guard")
        k += 1
        assert _counter(state) == start + k  # after k calls the state reads start + k
    assert native.DROPOUT_CALLS - calls0 == 2 * k
    if p == 0.0:
        assert keep == 1.0
    # a view at a 16-byte aligned offset is taken, one that is not is refused before anything is written
    buf = torch.full((64,), SENTINEL, device=DEV)
    native.dropout_mask(native.dropout_desc(5, p, seed, 1), None, buf[4:])
    assert buf[4:9].cpu().numpy().tobytes() == dc.mask_model(5, p, seed, 1).tobytes() and (buf[9:] == SENTINEL).all() and (buf[:4] == SENTINEL).all()
    with pytest.raises(native.NativeError, match="not 16-byte aligned"):
        native.dropout_mask(native.dropout_desc(5, p, seed, 1), None, buf[2:])
    torch.cuda.synchronize()


def test_torch_s_kept_value_on_the_device():
    """F.dropout on the GPU gives kept elements the same multiplier as on the CPU (tests/test_dropout_route.py pins the CPU's)."""
    import torch.nn.functional as F

    for p in dc.PS:
        pf = float(np.float32(p))
        m = F.dropout(torch.ones(1 << 16, device=DEV), pf, True)
        kept = torch.unique(m[m != 0]).cpu().numpy()
        assert kept.size == 1 and kept[0].tobytes() == dc.keep_of(p).tobytes(), (p, kept)


def test_draws_state_dict_and_resume():
    from tdmpc2_amd import autograd, native

    dm = autograd.DropoutMasks(SEEDS[0], DEV)
    assert dm.state_dict() == {"seed": SEEDS[0], "counter": 0}
    shape = (dc.FREQ_G, 96, 512)
    a, b = dm.draw(shape, dc.FREQ_P), dm.draw(shape, dc.FREQ_P)
    assert a.shape == shape and a.dtype == torch.float32 and a.is_contiguous() and a.data_ptr() != b.data_ptr()
    for call, m in enumerate((a, b)):
        assert m.cpu().numpy().tobytes() == dc.mask_model(dc.FREQ_N, dc.FREQ_P, SEEDS[0], call).reshape(shape).tobytes()
    sd = dm.state_dict()
    assert sd == {"seed": SEEDS[0], "counter": 2}
    c = dm.draw((7, 3), 0.25)
    other = autograd.DropoutMasks(999, DEV)
    other.load_state_dict(sd)
    assert torch.equal(other.draw((7, 3), 0.25), c) and other.state_dict()["counter"] == 3
    other.load_state_dict({"seed": 5, "counter": (1 << 32) - 1})  # the carry through a resumed counter
    d = other.draw((9,), 0.5)
    assert d.cpu().numpy().tobytes() == dc.mask_model(9, 0.5, 5, (1 << 32) - 1).tobytes() and other.state_dict()["counter"] == 1 << 32
    with pytest.raises(native.NativeError, match=r"outside \[0, 1\)"):
        dm.draw((4,), 1.0)


# ---------------------------------------------------------------- 2. capture
def test_a_captured_draw_draws_a_fresh_mask_on_every_replay():
    from tdmpc2_amd import autograd

    seed, shape, p = SEEDS[1], (3, 5, 67), 0.25
    n = int(np.prod(shape))
    dm = autograd.DropoutMasks(seed, DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        dm.draw(shape, p)  # warm-up outside the capture: counter 0
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    c = dm.state_dict()["counter"]
    assert c == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = dm.draw(shape, p)
    torch.cuda.synchronize()
    assert dm.state_dict()["counter"] == c  # nothing ran during the capture
    for r in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == dc.mask_model(n, p, seed, c + r).reshape(shape).tobytes(), r
    assert dm.state_dict()["counter"] == c + 3


# ---------------------------------------------------------------- 3. ensemble_apply with the fixture's masks
def _fixture_run(g, cot):
    from tdmpc2_amd import autograd

    f = dc.FIX
    params, leaves = dc.stacked_params(g, torch.float32, DEV)
    x = torch.tensor(g["x"], device=DEV).requires_grad_(True)
    mask = torch.tensor(g["mask"], device=DEV)
    out = autograd.ensemble_apply(params, x, mask)
    assert out.shape == (f["G"], f["T"], f["B"], f["out"])
    (out * torch.tensor(cot, device=DEV)).sum().backward()
    torch.cuda.synchronize()
    res = {"logits": out.detach().cpu().numpy(), "d_x": x.grad.cpu().numpy()}
    res.update({"d_" + k: leaves[k].grad.cpu().numpy() for k in dc.PARAMS})
    return res


def test_ensemble_apply_with_the_fixture_s_masks():
    from tdmpc2_amd import autograd, native

    g = dc.golden()
    got = _fixture_run(g, g["cot"])
    worst = {}
    fails = []
    for k, v in got.items():
        e, e32 = dc.rel_err(v, g[k + ".f64"]), dc.rel_err(g[k + ".f32"], g[k + ".f64"])
        worst[k] = e / max(e32, dc.FLOOR)
        print(k, "e", e, "e_ref32", e32, "ratio", round(worst[k], 3))
        if not e <= dc.MARGIN * max(e32, dc.FLOOR):
            fails.append((k, e, e32))
    _merge_json("fixture", {k: round(v, 3) for k, v in worst.items()})
    assert not fails, fails
    # the all-dropped row: a cotangent on that row alone reaches no Linear of layer 0 (pre is 0, the variance is 0, and the mask zeroes
    # what the LayerNorm hands back), so every gradient in front of the mask is exactly +-0 -- x included, which every member shares
    gi, ti, bi = dc.DROPPED_ROW
    cot = np.zeros_like(g["cot"])
    cot[gi, ti, bi] = g["cot"][gi, ti, bi]
    one = _fixture_run(g, cot)
    for k in ("d_x", "d_w0", "d_b0"):
        assert not one[k].any(), k
    assert one["d_be0"][gi].any() and one["d_w2"][gi].any() and not one["d_be0"][[i for i in range(dc.FIX["G"]) if i != gi]].any()
    # the forward of that row is ln_b through Mish and the rest: the row of another x is the same row
    params, _ = dc.stacked_params(g, torch.float32, DEV, requires_grad=False)
    x2 = torch.tensor(g["x"], device=DEV) * 3.0 + 1.0
    with torch.no_grad():
        moved = autograd.ensemble_apply(params, x2, torch.tensor(g["mask"], device=DEV)).cpu().numpy()
    assert moved[gi, ti, bi].tobytes() == got["logits"][gi, ti, bi].tobytes() and (moved[gi, ti, (bi + 1) % 5] != got["logits"][gi, ti, (bi + 1) % 5]).any()
    # a mask of another shape is refused
    with pytest.raises(native.NativeError, match="mask"):
        autograd.ensemble_apply(params, x2, torch.ones(2, 2, 5, 16, device=DEV))


# ---------------------------------------------------------------- 4. WorldModel
def _tiny_model(dropout=0.25, num_q=5):
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.world_model import WorldModel

    cfg = named_config("tiny", num_q=num_q, dropout=dropout, seed=SEEDS[0])
    torch.manual_seed(3)
    m = WorldModel(cfg).to(DEV)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.add_(torch.randn_like(p) * 0.1)
    m.native_autograd = True
    return m, cfg


def _restated(cfg, shape, call, p=None):
    p = cfg.dropout if p is None else p
    return torch.tensor(dc.mask_model(int(np.prod(shape)), p, cfg.seed, call).reshape(shape), device=DEV)


def test_world_model_draws_in_train_mode_with_the_flag_on():
    from tdmpc2_amd import autograd, native

    m, cfg = _tiny_model()
    H, B = 3, 7
    rng = np.random.default_rng(5)
    z = torch.tensor(rng.random((H, B, cfg.latent_dim)).astype(np.float32), device=DEV)
    a = torch.tensor(rng.uniform(-1, 1, (H, B, cfg.action_dim)).astype(np.float32), device=DEV)
    za = torch.cat([z, a], -1)
    with torch.no_grad():
        plain = autograd.ensemble_apply(m._Qs.params, za)
        m.train()
        m.native_dropout = True
        calls0 = native.DROPOUT_CALLS
        q0, q1 = m.Q(z, a, None, "all"), m.Q(z, a, None, "all")
        assert native.DROPOUT_CALLS - calls0 == 2 and not torch.equal(q0, q1) and not torch.equal(q0, plain)
        shape = (cfg.num_q, H, B, cfg.mlp_dim)
        for call, q in enumerate((q0, q1)):
            assert torch.equal(q, autograd.ensemble_apply(m._Qs.params, za, _restated(cfg, shape, call))), call
        # Q_pair draws for its two members only
        drawn = []
        real = m.q_masks.draw
        m.q_masks.draw = lambda s, p: (drawn.append((tuple(s), p)), real(s, p))[1]
        qidx = (3, 1)
        pair = m.Q_pair(z, a, None, qidx)
        assert drawn == [((2, H, B, cfg.mlp_dim), cfg.dropout)] and native.DROPOUT_CALLS - calls0 == 3
        pm = _restated(cfg, (2, H, B, cfg.mlp_dim), 2)
        assert torch.equal(pair, m.Q_pair(z, a, None, qidx, q_mask=pm)) and native.DROPOUT_CALLS - calls0 == 3
        full = torch.ones(shape, device=DEV)
        full[list(qidx)] = pm
        assert torch.equal(pair, m.Q(z, a, None, "all", q_mask=full)[list(qidx)])
        # 'min' / 'avg' draw too (train mode), once each
        m.Q(z, a, None, "avg")
        assert native.DROPOUT_CALLS - calls0 == 4 and m.q_masks.state_dict()["counter"] == 4
        # eval mode, the flag off, or cfg.dropout == 0: nothing is drawn and the output is what it was
        calls1 = native.DROPOUT_CALLS
        m.eval()
        assert torch.equal(m.Q(z, a, None, "all"), plain) and torch.equal(m.Q_pair(z, a, None, qidx), plain[list(qidx)])
        m.train()
        m.native_dropout = False
        assert torch.equal(m.Q(z, a, None, "all"), plain) and torch.equal(m.Q_pair(z, a, None, qidx), plain[list(qidx)])
        m.native_dropout = True
        m.cfg = cfg.replace(dropout=0.0)
        assert torch.equal(m.Q(z, a, None, "all"), plain) and torch.equal(m.Q_pair(z, a, None, qidx), plain[list(qidx)])
        assert native.DROPOUT_CALLS == calls1 and m.q_masks.state_dict()["counter"] == 4
    # with native_autograd off the torch path takes the drawn mask (rows: the module path of the ensemble takes [R, .])
    m.cfg = cfg
    m.native_autograd = False
    with torch.no_grad():
        rows = m.Q(z.reshape(H * B, -1), a.reshape(H * B, -1), None, "all")
    assert native.DROPOUT_CALLS == calls1 + 1
    want = autograd.ensemble_apply(m._Qs.params, za, _restated(cfg, shape, 4)).reshape(rows.shape)
    assert dc.rel_err(rows.cpu().numpy(), want.detach().cpu().numpy()) <= 1e-4


def _dropout_agent(case_id, dropout, flag=True):
    from tdmpc2_amd.tdmpc2 import TDMPC2

    cfg, sd = uc.build(case_id)
    cfg = cfg.replace(dropout=dropout, seed=SEEDS[0])
    agent = TDMPC2(cfg, device=DEV)
    agent.load({k: torch.as_tensor(v) for k, v in sd.items()})
    agent.native_autograd = True
    agent.native_dropout = flag
    agent.planner()
    agent.scale.value.fill_(uc.SCALE0)
    return agent, cfg, sd


def _batch(g, case_id):
    b = uc.batch_of(g, case_id)
    return tuple(None if b[k] is None else torch.tensor(b[k], device=DEV) for k in ("obs", "action", "reward", "terminated", "task"))


def test_the_forward_only_entry_points_draw_nothing():
    from tdmpc2_amd import native

    g = uc.golden()
    case_id = "tiny-B33"
    agent, cfg, _ = _dropout_agent(case_id, 0.25)
    obs, action, reward, _, _ = _batch(g, case_id)
    calls0 = native.DROPOUT_CALLS
    for mode in (agent.model.eval, agent.model.train):  # (the mode these are called in does not matter: the target is in eval in the reference)
        mode()
        try:
            with torch.no_grad():
                next_z = agent.model.encode(obs[1:], None)
                agent._td_target(next_z, reward, torch.zeros_like(reward))
                agent.act(obs[0, 0].cpu(), t0=True)
                res = agent.model_losses(obs, action, reward)
                agent.policy_loss(res["zs"])
                agent.update_info(obs, action, reward)
        finally:
            agent.model.eval()
    torch.cuda.synchronize()
    assert native.DROPOUT_CALLS == calls0 and agent.model._q_masks is None


# ---------------------------------------------------------------- 5. _update against a torch-only path with pinned masks
ITERS = 2
P_UPDATE = 0.25


def _masked_at_layer(layer):
    """QEnsemble.apply_params with the multipliers on `layer`'s Linear output: layer 0 is the function itself, layer 1 the control."""
    import torch.nn.functional as F

    def apply_params(p, x, mask=None):
        h = x.unsqueeze(0).expand(p.n, *x.shape)
        for i in (0, 1):
            l = p.layer(i)
            h = torch.baddbmm(l.bias.unsqueeze(1), h, l.weight.transpose(1, 2))
            if i == layer and mask is not None:
                h = h * mask.to(h.dtype).reshape(h.shape)
            h = F.layer_norm(h, (h.shape[-1],), None, None, 1e-5) * l.ln.weight.unsqueeze(1) + l.ln.bias.unsqueeze(1)
            h = F.mish(h)
        l = p.layer(2)
        return torch.baddbmm(l.bias.unsqueeze(1), h, l.weight.transpose(1, 2))
    return apply_params


def _update_pins(g, case_id, cfg, it, B):
    H, M = cfg.horizon, cfg.mlp_dim
    qs, ps = (cfg.num_q, H, B, M), (2, H + 1, B, M)
    return {"td_targets": g[f"{case_id}.td64"][it].astype(np.float32), "td_pi_eps": g[f"{case_id}.td_pi_eps"][it],
            "td_qidx": g[f"{case_id}.td_qidx"][it], "pi_eps": g[f"{case_id}.pi_eps"][it], "qidx": g[f"{case_id}.qidx"][it],
            "q_mask": dc.mask_model(int(np.prod(qs)), P_UPDATE, SEEDS[1], 2 * it).reshape(qs),
            "pi_q_mask": dc.mask_model(int(np.prod(ps)), P_UPDATE, SEEDS[1], 2 * it + 1).reshape(ps)}


def _torch_update_path(cfg, sd, g, case_id, h_pi, dtype, mask_layer, monkeypatch):
    """ITERS iterations of the port's `_update` in torch on the CPU in `dtype`: the modules, lc.torch_total, the RunningScale formulas,
    clip_grad_norm_ and Adam (widened fp32 hyperparameters), in the reference's order -- the model step and its zero_grad, then
    update_pi on the detached latents, whose backward leaves its remainder on the task embedding.  The TD target is pinned, so the
    target ensemble is never read and its soft update is left out.  -> [ITERS][info keys]."""
    from tdmpc2_amd import layers
    from tdmpc2_amd.world_model import WorldModel, two_hot_inv
    from tests import optim_common as oc
    from tests.test_gpu_pi_grad import _scale_update

    monkeypatch.setattr(layers.QEnsemble, "apply_params", staticmethod(_masked_at_layer(mask_layer)))
    m = WorldModel(cfg)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    m = m.to(dtype=dtype)
    b = uc.batch_of(g, case_id)
    t = lambda v: torch.tensor(np.asarray(v), dtype=dtype)  # noqa: E731
    obs, action, reward = t(b["obs"]), t(b["action"]), t(b["reward"])
    task = None if b["task"] is None else torch.tensor(b["task"])
    H, B = action.shape[:2]
    T = H + 1
    groups = [{"params": list(m._encoder.parameters()), "lr": oc.widen(cfg.lr * cfg.enc_lr_scale)}] + \
             [{"params": list(x.parameters())} for x in (m._dynamics, m._reward, m._Qs, m._task_emb if cfg.multitask else None) if x is not None]
    ps = [p for grp in groups for p in grp["params"]]
    opt = torch.optim.Adam(groups, lr=oc.widen(cfg.lr), betas=(oc.widen(0.9), oc.widen(0.999)), eps=oc.widen(1e-8))
    pi_ps = list(m._pi.parameters())
    pi_opt = torch.optim.Adam(pi_ps, lr=oc.widen(cfg.lr), betas=(oc.widen(0.9), oc.widen(0.999)), eps=oc.widen(1e-5))
    case = dict(T=H, B=B, L=cfg.latent_dim, NB=cfg.num_bins, Q=cfg.num_q, episodic=False)
    h = lc.hyper(cfg.num_bins, cfg.vmin, cfg.vmax, cfg.rho, (cfg.consistency_coef, cfg.reward_coef, cfg.value_coef, cfg.termination_coef))
    value = torch.full((1,), uc.SCALE0, dtype=dtype)
    rows = lambda tk, n: None if tk is None else tk.repeat(n)  # noqa: E731  (the module path of the Q ensemble takes rows)
    out = []
    m.train()
    for it in range(ITERS):
        pins = _update_pins(g, case_id, cfg, it, B)
        with torch.no_grad():
            next_z = m.encode(obs[1:], task)
        td = t(pins["td_targets"])
        z = m.encode(obs[0], task)
        zs = [z]
        for s in range(H):
            z = m.next(z, action[s], task)
            zs.append(z)
        _zs, z_pred = torch.stack(zs[:-1]), torch.stack(zs[1:])
        qs = m.Q(_zs.reshape(H * B, -1), action.reshape(H * B, -1), rows(task, H), "all",
                 q_mask=t(pins["q_mask"]).reshape(cfg.num_q, H * B, -1)).reshape(cfg.num_q, H, B, -1)
        rp = m.reward(_zs, action, task)
        losses, _ = lc.torch_total(z_pred, next_z, rp, reward[..., 0], qs, td[..., 0], None, None, case, h)
        losses[4].backward()
        norm = torch.nn.utils.clip_grad_norm_(ps, oc.widen(cfg.grad_clip_norm))
        opt.step()
        opt.zero_grad()
        # update_pi
        zd = torch.stack(zs).detach()
        act, info = m.pi(zd, task, eps=t(pins["pi_eps"]))
        ql = m.Q_pair(zd.reshape(T * B, -1), act.reshape(T * B, -1), rows(task, T), [int(i) for i in pins["qidx"]],
                      q_mask=t(pins["pi_q_mask"]).reshape(2, T * B, -1)).reshape(2, T, B, -1)
        q = two_hot_inv(ql, cfg).sum(0) / 2
        value = _scale_update(value, q[0].detach(), oc.widen(cfg.tau))
        rho = torch.tensor([h_pi["rho"] ** i for i in range(T)], dtype=dtype)
        pi_loss = (-(h_pi["entropy_coef"] * info["scaled_entropy"] + q / value).mean(dim=(1, 2)) * rho).mean()
        pi_loss.backward()
        pi_norm = torch.nn.utils.clip_grad_norm_(pi_ps, oc.widen(cfg.grad_clip_norm))
        pi_opt.step()
        pi_opt.zero_grad()
        row = {k: float(v.detach()) for k, v in zip(uc.LOSS_KEYS, losses + [norm])}
        row.update(pi_loss=float(pi_loss.detach()), pi_grad_norm=float(pi_norm), pi_entropy=float(info["entropy"].detach().mean()),
                   pi_scaled_entropy=float(info["scaled_entropy"].detach().mean()), pi_scale=float(value))
        out.append([row[k] for k in uc.info_keys(cfg)])
    return np.asarray(out)


@pytest.mark.parametrize("case_id", ["tiny-B33", "tiny_mt-B12"])
def test_update_with_pinned_masks_against_a_torch_only_path(case_id, monkeypatch):
    from tdmpc2_amd import native
    from tests.test_gpu_pi_grad import _hyper_of

    g = uc.golden()
    agent, cfg, sd = _dropout_agent(case_id, P_UPDATE)
    keys = uc.info_keys(cfg)
    h_pi = _hyper_of(agent, cfg)
    with monkeypatch.context() as mp:
        ref = _torch_update_path(cfg, sd, g, case_id, h_pi, torch.float64, 0, mp)
        t32 = _torch_update_path(cfg, sd, g, case_id, h_pi, torch.float32, 0, mp)
        control = _torch_update_path(cfg, sd, g, case_id, h_pi, torch.float64, 1, mp)
    batch = _batch(g, case_id)
    B = batch[1].shape[1]
    calls0 = native.DROPOUT_CALLS
    got = np.zeros((ITERS, len(keys)))
    for it in range(ITERS):
        pins = _update_pins(g, case_id, cfg, it, B)
        pins = {k: torch.tensor(v, device=DEV) for k, v in pins.items()}
        pins["qidx"] = pins["qidx"].long()
        info = agent._update(*batch, pins=pins)
        assert set(info) == set(keys) and not agent.model.training
        got[it] = [float(info[k]) for k in keys]
    assert native.DROPOUT_CALLS == calls0  # every mask was given: nothing is drawn
    worst, fails, control_worst = {}, [], (0.0, None)
    for it in range(ITERS):
        for j, k in enumerate(keys):
            r = ref[it, j]
            if r == 0:
                assert got[it, j] == 0 and t32[it, j] == 0, (it, k)
                continue
            e, e32, ec = abs(got[it, j] - r) / abs(r), abs(t32[it, j] - r) / abs(r), abs(control[it, j] - r) / abs(r)
            bound = dc.MARGIN * max(e32, dc.FLOOR)
            worst[k] = max(worst.get(k, 0.0), e / (bound / dc.MARGIN))
            print(case_id, "iteration", it, k, "lib", got[it, j], "ref64", r, "e", e, "e_torch32", e32, "ratio", round(e / (bound / dc.MARGIN), 3),
                  "control misses by", round(ec / bound, 1), "bounds")
            if ec / bound > control_worst[0]:
                control_worst = (ec / bound, k)
            if not e <= bound:
                fails.append((it, k, e, e32))
    _merge_json(f"update_{case_id}", {k: round(v, 3) for k, v in worst.items()})
    _merge_json(f"update_{case_id}.control_layer1", {"bounds": round(control_worst[0], 1), "key": control_worst[1]})
    assert not fails, fails
    # the sensitivity floor: the masks' zeros moved to layer 1 miss the gate by at least 10 bounds on some key
    assert control_worst[0] >= uc.SENSITIVITY, control_worst


@pytest.mark.parametrize("case_id", ["tiny-B33", "tiny_mt-B12"])
def test_update_without_pins_draws_exactly_two_masks(case_id):
    from tdmpc2_amd import native

    g = uc.golden()
    agent, cfg, _ = _dropout_agent(case_id, P_UPDATE)
    batch = _batch(g, case_id)
    H, B, M = cfg.horizon, batch[1].shape[1], cfg.mlp_dim
    masks = agent.model.q_masks
    drawn = []
    real = masks.draw
    masks.draw = lambda s, p: (drawn.append((tuple(s), p)), real(s, p))[1]
    torch.manual_seed(11)
    for it in range(2):
        calls0 = native.DROPOUT_CALLS
        info = agent._update(*batch)
        torch.cuda.synchronize()
        assert native.DROPOUT_CALLS - calls0 == 2 and masks.state_dict()["counter"] == 2 * (it + 1)
        assert drawn[-2:] == [((cfg.num_q, H, B, M), P_UPDATE), ((2, H + 1, B, M), P_UPDATE)]  # the value pass first
        assert set(info) == set(uc.info_keys(cfg)) and all(bool(torch.isfinite(v)) for v in info.values())
        assert not agent.model.training
    # the flag off: the same call draws nothing
    agent.native_dropout = False
    calls0 = native.DROPOUT_CALLS
    agent._update(*batch)
    assert native.DROPOUT_CALLS == calls0 and masks.state_dict()["counter"] == 4
    with pytest.raises(ValueError, match="unknown pins"):
        agent._update(*batch, pins={"mask": None})


# ---------------------------------------------------------------- 6. update(buffer) at the default cfg.dropout
def test_update_from_a_buffer_at_the_default_dropout():
    from tdmpc2_amd import native
    from tests.test_gpu_update import _buffer, _fresh_packed

    from tdmpc2_amd.config import named_config

    case_id = "tiny-B33"
    default = named_config("tiny").dropout
    assert default == 0.01
    agent, cfg, _ = _dropout_agent(case_id, default)
    assert agent.native_dropout and agent.model.native_dropout
    buf = _buffer(cfg)
    torch.manual_seed(11)
    before = agent.planner().export_packed()
    for it in range(3):
        calls0 = native.DROPOUT_CALLS
        info = agent.update(buf)
        torch.cuda.synchronize()
        assert native.DROPOUT_CALLS - calls0 == 2 and all(bool(torch.isfinite(v)) for v in info.values())
        packed = agent.planner().export_packed()
        assert packed == _fresh_packed(agent), it  # after the model step, the policy step and the soft update
        assert packed != before
        before = packed
    assert agent.model.q_masks.state_dict() == {"seed": SEEDS[0], "counter": 6}
