"""-m gpu: the loss rows of tdmpc2_plan_model_losses at their edges, with PINNED LOGITS.  A head whose last layer is bound with
weight 0 and bias l returns the logits l on every row (0 x + b = b in either arithmetic), so every loss term has an fp64 closed
form on the host that owes nothing to the code under test (tests/model_common.py; tests/test_model_edges.py checks that closed
form against the reference and that the gate admits the reference's own fp32).

Gate of items 2-5, per element: max(1e-5 max(1, |v|), 2 |restatement in fp32 - restatement in fp64|) (mc.edge_gate).  With B = 1 a
`step_means` entry is the term of ONE row; at B = 130 every row gets the same target and the mean must equal the row term.
The row "off+10000" (lse = m + log(sum) in fp32 loses the digits of log(sum) at m = 1e4) is printed, not gated.
TDMPC2_EDGES_JSON=<file>: the worst err / gate per item, family and arithmetic is written there (profiles/model_edges.json).

What bites, from scratch builds of model_rows.cuh run once each on the MI355X: without the fminf(.., vmax) clamp the edge-target,
fresh-model, offset-1e4 (finiteness) and non-finite-target tests fail while all 73 of tests/test_gpu_model.py pass; with `off` and
`1 - off` swapped the edge-target, tail and termination tests fail (37 of test_gpu_model.py too); with the sign of x y flipped in
model_bce the termination, tail (episodic handles) and two-piece tests fail (10 of test_gpu_model.py too).  With logf in symlog_f the
edge-target test fails; on the library before NaN propagated the non-finite-target test fails as well."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import model_common as mc
from tests.gpu_common import case_on_gpu, dev

pytestmark = pytest.mark.gpu

HANDLES = [("c2", 1), ("c1_ep", 1), ("mt5", 1), ("small_ep_fire", 2), ("c3", 2)]
RUNS = [(n, p, prec) for n, p in HANDLES for prec in (1, 2) if not (n == "c3" and prec == 1)]   # c3 (48M): split arithmetic only
SMALL_RUNS = [r for r in RUNS if r[0] != "c3"]
ROWS = 8 * 130

_handles = {}
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_worst():
    yield
    path = os.environ.get("TDMPC2_EDGES_JSON")
    if path:
        with open(path, "w") as f:
            json.dump({"gate": "max(1e-5 max(1,|v|), 2 |restatement fp32 - restatement fp64|); item 6: max(1e-4 max(1,|v|), 2 |oracle fp32 - oracle fp64|)",
                       "worst_err_over_gate": [dict(item=k[0], family=k[1], arithmetic=k[2], worst=v) for k, v in sorted(_worst.items())]},
                      f, indent=1)


def _note(item, planner, ratio):
    key = (item, "fused" if planner.path == 1 else "layered", "fp32" if planner.precision == 1 else "split")
    _worst[key] = max(_worst.get(key, 0.0), float(ratio))


class Handle:
    def __init__(self, name, path, prec, max_envs=None):
        from tdmpc2_amd.native import NativePlanner

        self.c, self.model, _ = case_on_gpu(name, path, prec)
        self.cfg = cfg = self.c["cfg"]
        me = max(2, -(-ROWS // cfg.num_samples)) if max_envs is None else max_envs
        self.planner = NativePlanner(cfg, self.c["iterations"], dev(), max_envs=me, path=path, precision=prec)
        assert self.planner.path == path
        self.bound = None
        self.tag = f"{name} path {path} prec {prec}"
        self.kw = {}
        if cfg.multitask:
            emb = self.model.sd["_task_emb.weight"]
            norm = emb.norm(2, dim=-1, keepdim=True)
            emb = torch.where(norm > 1.0, emb * (1.0 / (norm + 1e-7)), emb)  # nn.Embedding(max_norm=1)
            self.kw = dict(task_emb_table=emb.to(dev()).contiguous(),
                           act_mask_table=self.model.sd["_action_masks"].to(torch.float32).to(dev()).contiguous())

    def bind(self, key, reward_row=None, q_rows=None, term_x=None):
        """Bind the case's weights with the named last layers pinned (key: what is bound now; None: the case's own weights)."""
        if self.bound == ("sd", key):
            return
        sd = self.model.sd if key is None else mc.pin_heads(self.model.sd, self.cfg, reward_row, q_rows,
                                                            term_x if self.cfg.episodic else None)
        self.planner.bind_state_dict(sd)
        self.bound = ("sd", key)

    def args(self, B, H):
        cfg = self.cfg
        inp = mc.inputs(cfg, B)
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev())
        kw = dict(self.kw)
        if cfg.multitask:
            kw["task_ids"] = d(inp["tasks"].astype(np.int32))
        act = np.random.default_rng(31 + H).uniform(-1, 1, (H, B, cfg.action_dim)).astype(np.float32)
        return d(inp["z0"]), d(act), kw

    def losses(self, B, H, reward, td, term=None, next_z=None, rho=0.5, coefs=(20.0, 0.1, 0.1, 1.0), want=()):
        """reward / td / term: [H] (one target per step, given to every row) or [H, B]."""
        cfg = self.cfg
        z0, act, kw = self.args(B, H)
        full = lambda a: torch.as_tensor(np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32).reshape(H, -1), (H, B)))).to(dev())
        nz = torch.zeros(H, B, cfg.latent_dim, device=dev()) if next_z is None else next_z
        tm = full(np.zeros(H) if term is None else term) if cfg.episodic else None
        return self.planner.model_losses(z0, act, nz, full(reward), full(td), tm, rho=rho, coefs=coefs, want=want, step_means=True, **kw)


def _row_cap(h):
    """The rows the layered activation workspace holds, AS THE LIBRARY REPORTS IT: a call beyond it is refused before anything
    is launched, and the refusal names the capacity."""
    import re
    from tdmpc2_amd.native import NativeError

    z0, act, kw = h.args(1 << 14, 1)
    with pytest.raises(NativeError) as ex:
        h.planner.model_rollout(z0, act, want=("zs",), **kw)
    m = re.search(r"workspace holds (\d+) rows", str(ex.value))
    assert m, str(ex.value)
    return int(m.group(1))


def _handle(name, path, prec):
    key = (name, path, prec)
    if key not in _handles:
        if name == "c3":   # one 48M handle at a time
            for k in [k for k in _handles if k[0] == "c3"]:
                del _handles[k]
        _handles[key] = Handle(name, path, prec)
    return _handles[key]


def _expected(cfg, rr, qr, tx, reward, td, term, rho, coefs, dtype):
    """(losses [5], step_means [4, H]) of pinned logits and one target per step: the B = 1 restatement, in `dtype`.  The
    consistency slots are 0 here (compared separately)."""
    H = len(reward)
    ns = SimpleNamespace(num_bins=cfg.num_bins, vmin=cfg.vmin, vmax=cfg.vmax, rho=rho, episodic=cfg.episodic, consistency_coef=coefs[0],
                         reward_coef=coefs[1], value_coef=coefs[2], termination_coef=coefs[3])
    a = lambda v: np.asarray(v, np.float32).astype(dtype)
    R = np.broadcast_to(a(rr), (H, 1, cfg.num_bins))
    Q = np.broadcast_to(a(qr)[:, None, None, :], (len(qr), H, 1, cfg.num_bins))
    tl = np.full((H + 1, 1), a(0.0 if tx is None else tx))
    with np.errstate(all="ignore"):
        return mc.losses_from(ns, np.zeros((H + 1, 1, 1), dtype), R, Q, tl, np.zeros((H, 1, 1), dtype), a(reward)[:, None], a(td)[:, None],
                              a(np.zeros(H) if term is None else term)[:, None])


def _gated(item, h, got, cfg, rr, qr, tx, reward, td, term=None, rho=0.5, coefs=(20.0, 0.1, 0.1, 1.0), what="", gate=True):
    """Compare losses[1:4] and step_means[1:4] of one call with the closed form; returns the worst err / gate."""
    l64, s64 = _expected(cfg, rr, qr, tx, reward, td, term, rho, coefs, np.float64)
    l32, s32 = _expected(cfg, rr, qr, tx, reward, td, term, rho, coefs, np.float32)
    gl, gs = got["losses"].cpu().numpy().astype(np.float64), got["step_means"].cpu().numpy().astype(np.float64)
    rows = [1, 2] + ([3] if cfg.episodic else [])
    rl = np.abs(gl[rows] - l64[rows]) / mc.edge_gate(l64[rows], l32[rows])
    rs = np.abs(gs[rows] - s64[rows]) / mc.edge_gate(s64[rows], s32[rows])
    worst = max(rl.max(), rs.max())
    if gate:
        _note(item, h.planner, worst)
        if not worst <= 1:
            k, t = np.unravel_index(np.argmax(rs), rs.shape)
            raise AssertionError(f"[{h.tag}] {what}: err / gate losses {rl}, step_means worst {rs.max():.3f} at kind {rows[k]} step {t} "
                                 f"(reward {reward[t]!r}, td {td[t]!r}): got {gs[rows[k], t]!r}, closed form {s64[rows[k], t]!r}")
    if not cfg.episodic:
        assert gl[3] == 0 and not gs[3].any()
    return worst


def _configs(cfg, name):
    """Pinned configurations (key, reward row, q rows, term x, names): every row of the edge table sits on the reward head once,
    the next num_q rows of the table on the Q heads (a different row per head), the termination inputs go round."""
    rows = mc.edge_logit_rows(cfg)
    names = [n for n in rows if n != mc.UNGATED_ROW]
    if name == "c3":   # 48M: one configuration.  c3 does not see: on the reward head any row but n30; on any head n10, n100,
        # hot0, hot50, off+0, off+-30, off-300; the termination inputs (not episodic); the offset-1e4 row and the non-finite
        # targets (SMALL_RUNS).  small_ep_fire runs every one of them on the same layered kernels in both arithmetics.
        pick = [["n30", "zero", "n1", "hot100", "twomax", "off+300"]]
    else:
        pick = [[names[(k + i) % len(names)] for i in range(1 + cfg.num_q)] for k in range(len(names))]
    out = []
    for k, p in enumerate(pick):
        p = p[:1 + cfg.num_q]
        out.append((f"edge{k}", rows[p[0]], np.stack([rows[n] for n in p[1:]]), mc.TERM_XS[k % len(mc.TERM_XS)], p))
    return out


# ---------------------------------------------------------------- 1. the pinned logits come back bit for bit
@pytest.mark.parametrize("name,path,prec", RUNS)
def test_pinned_logits_come_back_bit_for_bit(name, path, prec):
    """Bias rows head * 1000 + bin (exactly representable, distinct per bin and head): a column, padding (101 -> 128), head or step
    permutation would show.  Online and target ensemble, B = 130 at the case's horizon, B = 1 and 65 at H = 8."""
    h = _handle(name, path, prec)
    cfg = h.cfg
    nb = cfg.num_bins
    rr = np.arange(nb, dtype=np.float32)
    qr = np.stack([(i + 1) * 1000 + rr for i in range(cfg.num_q)])
    tx = 7.25
    h.bind("bits", rr, qr, tx)
    q64, q32 = mc.two_hot_inv_rows(qr.astype(np.float64), cfg), mc.two_hot_inv_rows(qr, cfg)
    r64, r32 = mc.two_hot_inv_rows(rr.astype(np.float64), cfg), mc.two_hot_inv_rows(rr, cfg)
    want = ("reward_logits", "reward", "q_logits", "q") + (("term_logit",) if cfg.episodic else ())
    for B, H in ((130, cfg.horizon), (1, 8), (65, 8)):
        for target in (False, True):
            z0, act, kw = h.args(B, H)
            got = h.planner.model_rollout(z0, act, use_target=target, want=want, **kw)
            assert torch.equal(got["reward_logits"], torch.as_tensor(rr).to(dev()).expand(H, B, nb)), (B, H, "reward_logits")
            assert torch.equal(got["q_logits"], torch.as_tensor(qr).to(dev())[:, None, None, :].expand(-1, H, B, -1)), (B, H, target)
            if cfg.episodic:
                assert torch.equal(got["term_logit"], torch.full((H + 1, B, 1), tx, device=dev())), (B, H)
            ev = np.abs(got["reward"].cpu().numpy().astype(np.float64) - r64).max() / mc.edge_gate(r64, r32)
            eq = (np.abs(got["q"].cpu().numpy().astype(np.float64)[..., 0] - q64[:, None, None]) / mc.edge_gate(q64, q32)[:, None, None]).max()
            _note("1 two_hot_inv of pinned rows", h.planner, max(ev, eq))
            assert ev <= 1 and eq <= 1, (B, H, ev, eq)
    assert h.planner.take_fault() == 0


# ---------------------------------------------------------------- 2. edge targets on the reward head and every Q head
@pytest.mark.parametrize("name,path,prec", RUNS)
def test_edge_targets_and_logit_rows(name, path, prec):
    """Every target of mc.edge_targets against every row of mc.edge_logit_rows: eight targets per call at B = 1, H = 8 (one row
    per step_means entry), the same at B = 130 with the target repeated over the rows; `reward` / `q` against two_hot_inv."""
    h = _handle(name, path, prec)
    cfg = h.cfg
    t = mc.edge_targets(cfg)
    assert not mc.EDGE_REMOVED   # (a removed pair would be masked here)
    worst = 0.0
    for key, rr, qr, tx, names in _configs(cfg, name):
        h.bind(key, rr, qr, tx)
        for j in range(0, len(t), 8):
            rew, td = t[j:j + 8], t[j:j + 8][::-1].copy()
            for B in (1, 130):
                got = h.losses(B, 8, rew, td, want=("reward", "q") if j == 0 else ())
                worst = max(worst, _gated("2 edge targets", h, got, cfg, rr, qr, tx, rew, td, what=f"{names} B {B} targets {j}.."))
                if j == 0:
                    lg = np.concatenate([rr[None], qr])
                    v64, v32 = mc.two_hot_inv_rows(lg.astype(np.float64), cfg), mc.two_hot_inv_rows(lg, cfg)
                    v = np.concatenate([got["reward"].cpu().numpy()[None], got["q"].cpu().numpy()])[..., 0].astype(np.float64)
                    ratio = (np.abs(v - v64[:, None, None]) / mc.edge_gate(v64, v32)[:, None, None]).max()
                    _note("2 two_hot_inv", h.planner, ratio)
                    assert ratio <= 1, (names, ratio)
    print(f"[{h.tag}] edge targets: worst err / gate {worst:.3f}")
    assert h.planner.take_fault() == 0


@pytest.mark.parametrize("name,path,prec", SMALL_RUNS)
def test_offset_1e4_row_is_measured_not_gated(name, path, prec):
    """c = 1e4 added to the scale-3 row: lse = m + logf(sum) keeps about 1e-3 absolute of log(sum) at m = 1e4, the reference's
    log_softmax subtracts m first.  Printed and recorded, finite; not gated (model_soft_ce keeps the one-sum form).  On the MI355X:
    worst relative error of a row term 1.3e-4 (the reference's fp32: 1.3e-5, tests/test_model_edges.py)."""
    h = _handle(name, path, prec)
    cfg = h.cfg
    r = mc.edge_logit_rows(cfg)[mc.UNGATED_ROW]
    qr = np.repeat(r[None], cfg.num_q, 0)
    h.bind("ungated", r, qr, 0.0)
    t = mc.edge_targets(cfg)
    worst = rel = 0.0
    for j in range(0, len(t), 8):
        got = h.losses(1, 8, t[j:j + 8], t[j:j + 8])
        assert torch.isfinite(got["losses"]).all() and torch.isfinite(got["step_means"]).all()
        worst = max(worst, _gated("", h, got, cfg, r, qr, 0.0, t[j:j + 8], t[j:j + 8], gate=False))
        s64 = _expected(cfg, r, qr, 0.0, t[j:j + 8], t[j:j + 8], None, 0.5, (20.0, 0.1, 0.1, 1.0), np.float64)[1][1:3]
        rel = max(rel, (np.abs(got["step_means"].cpu().numpy().astype(np.float64)[1:3] - s64) / np.maximum(1, np.abs(s64))).max())
    # the ratio says little here: the fp32 restatement has the same one-sum form, so its own loss widens the gate.  The figure
    # to read is the relative error of the row terms against fp64.
    print(f"[{h.tag}] offset 1e4 row (ungated): worst relative error {rel:.2e}, err / gate {worst:.2f}")
    _note("2 offset 1e4 row, UNGATED", h.planner, worst)
    _note("2 offset 1e4 row, UNGATED: relative error of the row terms, not a ratio", h.planner, rel)
    assert h.planner.take_fault() == 0


# ---------------------------------------------------------------- 3. termination BCE
@pytest.mark.parametrize("name,path,prec", [r for r in SMALL_RUNS if r[0] in ("c1_ep", "small_ep_fire")])
def test_termination_bce_edges(name, path, prec):
    """x in +-0, 1e-8, +-20, +-88, +-104, +-1e4 against y in 0, 1, 0.3.  The logit is compared as a bit pattern (torch.equal
    alone takes -0 for +0); the logit of the pinned -0 is +0, the sum 0 x + (-0) rounded to nearest."""
    h = _handle(name, path, prec)
    cfg = h.cfg
    rows = mc.edge_logit_rows(cfg)
    rr, qr = rows["n1"], np.stack([rows["n10"]] * cfg.num_q)
    ys = np.array([0, 1, 0.3, 1, 0.3, 0, 0.3, 1], np.float32)
    for x in mc.TERM_XS:
        h.bind(f"term{x!r}", rr, qr, x)
        for B in (1, 130):
            got = h.losses(B, 8, np.ones(8), np.ones(8), term=ys, want=("term_logit",))
            bits = torch.full((9, B, 1), float(np.float32(x) + np.float32(0.0)), device=dev()).view(torch.int32)   # -0 + 0 = +0
            assert torch.equal(got["term_logit"].view(torch.int32), bits), (x, got["term_logit"].flatten()[:2])
            _gated("3 termination BCE", h, got, cfg, rr, qr, x, np.ones(8, np.float32), np.ones(8, np.float32), term=ys, what=f"x {x!r} B {B}")
    assert h.planner.take_fault() == 0


# ---------------------------------------------------------------- 4. a fresh model
@pytest.mark.parametrize("name,path,prec", RUNS)
def test_fresh_model_zero_last_layers(name, path, prec):
    """The reference zero-initialises the last layer of the reward head and of every Q head (common/world_model.py:32): max |W| = 0
    in the weight scaling.  Logits exactly 0, values symexp(sum(bins) / 101), every soft-CE row log(101) whatever its target."""
    h = _handle(name, path, prec)
    cfg = h.cfg
    nb, nq = cfg.num_bins, cfg.num_q
    rr, qr = np.zeros(nb, np.float32), np.zeros((nq, nb), np.float32)
    h.bind("fresh", rr, qr, 0.0)
    B, H = 130, cfg.horizon
    t = mc.edge_targets(cfg)
    rew = np.resize(t, (H, B))
    td = np.resize(t[::-1], (H, B))
    got = h.losses(B, H, rew, td, rho=cfg.rho, want=("reward_logits", "q_logits", "reward", "q"))
    assert not got["reward_logits"].any() and not got["q_logits"].any()
    v64, v32 = mc.two_hot_inv_rows(rr.astype(np.float64), cfg), mc.two_hot_inv_rows(rr, cfg)
    for k in ("reward", "q"):
        ratio = np.abs(got[k].cpu().numpy().astype(np.float64) - v64).max() / mc.edge_gate(v64, v32)
        _note("4 fresh model", h.planner, ratio)
        assert ratio <= 1, (k, ratio)
    # every row's term is log(101): the batch means are too, and the losses follow from rho and H.  (The closed form below is given
    # column 0's targets as if every row had them: with all-zero logits the term cannot depend on the target.)
    worst = _gated("4 fresh model", h, got, cfg, rr, qr, 0.0, rew[:, 0], td[:, 0], rho=cfg.rho, what="fresh")
    sm = got["step_means"].cpu().numpy().astype(np.float64)
    assert np.abs(sm[1:3] - np.log(101)).max() <= 2e-5   # (1e-5 max(1, |v|) of the gate, v = 4.615)
    want = np.log(101) * sum(cfg.rho ** k for k in range(H)) / H
    assert np.abs(got["losses"].cpu().numpy()[1:3] - want).max() <= 1e-5 * max(1, want)
    for j in range(0, len(t), 8):   # row by row: B = 1, H = 8, a step_means entry is ONE row's term, eight edge targets per call
        one = h.losses(1, 8, t[j:j + 8], t[j:j + 8][::-1].copy(), rho=cfg.rho)
        worst = max(worst, _gated("4 fresh model", h, one, cfg, rr, qr, 0.0, t[j:j + 8], t[j:j + 8][::-1].copy(), rho=cfg.rho, what=f"fresh rows {j}.."))
        assert np.abs(one["step_means"].cpu().numpy().astype(np.float64)[1:3] - np.log(101)).max() <= 2e-5, j
    tq = h.planner.model_rollout(*h.args(B, H)[:2], use_target=True, want=("q_logits",), **h.args(B, H)[2])
    assert not tq["q_logits"].any()
    print(f"[{h.tag}] fresh model: worst err / gate {worst:.3f}")
    assert h.planner.take_fault() == 0


# ---------------------------------------------------------------- 5. tail arithmetic
STEP_T = np.array([0.5, -3.0, 123.0, 22025.4, -1e6, 1e-8, 7.0, -0.2], np.float32)


@pytest.mark.parametrize("name,path,prec", RUNS)
def test_tail_arithmetic(name, path, prec):
    """Pinned logits and one target per step, so the expected means are known without summation error: ragged B, H, rho (rho^0 = 1
    at rho = 0 too), coefficients with a zero and a negative one; total against the coefficient-weighted sum of the four returned
    losses to 1e-6 of sum |c_i l_i| (three fp32 additions: at most 3 x 2^-24 of it); consistency exactly 0 against the call's own
    zs[1:], and the fp64 mean of zs^2 against next_z = 0."""
    h = _handle(name, path, prec)
    cfg = h.cfg
    rows = mc.edge_logit_rows(cfg)
    names = ["n10", "n1", "twomax", "off-30", "n30", "hot50"]
    rr, qr, tx = rows[names[0]], np.stack([rows[n] for n in names[1:1 + cfg.num_q]]), 1.5
    h.bind("tail", rr, qr, tx)
    ys = np.array([0, 1, 0.3, 1, 0, 0, 1, 0.3], np.float32)
    defaults = (20.0, 0.1, 0.1, 1.0)
    shapes = [(B, 1) for B in (1, 63, 64, 65, 255, 256, 257, 1040)] + [(B, 8) for B in (1, 63, 64, 65, 130)] + [(130, H) for H in (2, 7)]
    runs = [(B, H, 0.5, defaults) for B, H in shapes]
    runs += [(65, 8, rho, defaults) for rho in (0.0, 1.0)] + [(65, 7, 0.5, cf) for cf in ((20.0, 0.0, 0.1, 1.0), (20.0, 0.1, -0.7, 1.0), (0.0, 2.0, 0.5, -1.0))]
    worst = 0.0
    for B, H, rho, coefs in runs:
        rew, td = STEP_T[:H], STEP_T[::-1][:H].copy()
        got = h.losses(B, H, rew, td, term=ys[:H], rho=rho, coefs=coefs, want=("zs",))
        worst = max(worst, _gated("5 tail", h, got, cfg, rr, qr, tx, rew, td, term=ys[:H], rho=rho, coefs=coefs, what=f"B {B} H {H} rho {rho} coefs {coefs}"))
        ls = got["losses"].cpu().numpy().astype(np.float64)
        terms = np.array([coefs[0] * ls[0], coefs[1] * ls[1], coefs[3] * ls[3], coefs[2] * ls[2]])
        assert abs(ls[4] - terms.sum()) <= 1e-6 * max(1.0, np.abs(terms).sum()), (B, H, rho, coefs, ls)
        # consistency against next_z = 0: the fp64 mean of zs^2
        zs = got["zs"].cpu().numpy()
        c64 = (zs[1:].astype(np.float64) ** 2).mean((1, 2))
        c32 = (zs[1:] ** 2).mean((1, 2), dtype=np.float32)
        sm0 = got["step_means"].cpu().numpy().astype(np.float64)[0]
        w = np.array([rho ** k for k in range(H)])
        l64, l32 = (c64 * w).sum() / H, np.float32((c32 * w.astype(np.float32)).sum() / np.float32(H))
        ratio = max((np.abs(sm0 - c64) / mc.edge_gate(c64, c32)).max(), abs(ls[0] - l64) / mc.edge_gate(l64, l32))
        _note("5 consistency", h.planner, ratio)
        assert ratio <= 1, (B, H, rho, ratio)
        # ... and against the call's own zs[1:]: exactly 0
        same = h.losses(B, H, rew, td, term=ys[:H], rho=rho, coefs=coefs, next_z=got["zs"][1:].contiguous())
        assert float(same["losses"][0]) == 0.0 and not same["step_means"][0].any(), (B, H)
        assert torch.equal(same["losses"][1:4], got["losses"][1:4]) and torch.equal(same["step_means"][1:], got["step_means"][1:])
    print(f"[{h.tag}] tail: worst err / gate {worst:.3f}")
    assert h.planner.take_fault() == 0


# ---------------------------------------------------------------- 6. chunked termination on the layered family
@pytest.mark.parametrize("prec", [1, 2])
def test_chunked_termination_layered(prec, tmp_path):
    """small_ep_fire with max_envs = 3: the activation workspace holds 384 rows (the figure is read back from the library's own
    refusal of an oversized call, not recomputed here), H B = 300 fits and (H + 1) B = 400 does not, so MS_TERM runs in two
    pieces (asserted through model_route.h itself on the reported capacity).  term_logit and the termination loss against the fp64
    oracle under the suite's gate max(1e-4 max(1, |v|), 2 |oracle fp32 - oracle fp64|), and against a roomy handle (one piece)
    at 1e-5; the last row and the first row of the second piece by name."""
    from oracle import planner_oracle as po
    from tests import model_route_model as mr

    B, H = 100, 3
    tight = Handle("small_ep_fire", 2, prec, max_envs=3)
    cfg = tight.cfg
    cap = _row_cap(tight)
    assert H * B <= cap < (H + 1) * B
    lib = mr.build(tmp_path)
    route = lambda c: mr.route(lib, mr.LAYERED, B, H, cfg.num_q, cfg.num_bins, 1, mr.TERM | mr.LOSSES, c, 0 if prec == 2 else 1)
    assert route(cap)["refuse"] == mr.OK and route(cap)["st"][mr.TERM_STAGE]["chunks"] >= 2
    roomy = _handle("small_ep_fire", 2, prec)
    room_cap = _row_cap(roomy)
    assert room_cap >= (H + 1) * B and route(room_cap)["st"][mr.TERM_STAGE]["chunks"] == 1
    tight.bind(None)
    roomy.bind(None)
    term = (np.random.default_rng(3).random((H, B)) < 0.3).astype(np.float32)
    got = tight.losses(B, H, np.zeros((H, B)), np.zeros((H, B)), term=term, want=("term_logit",))
    one = roomy.losses(B, H, np.zeros((H, B)), np.zeros((H, B)), term=term, want=("term_logit",))
    # the oracle, fp64 and fp32, on the same inputs
    z0, act, _ = tight.args(B, H)
    ref = {}
    for dt in (torch.float64, torch.float32):
        m = po.OracleModel(cfg, tight.model.sd, dtype=dt)
        z, zs = z0.cpu().to(dt), []
        zs.append(z)
        for t in range(H):
            z = m.next(z, act[t].cpu().to(dt), None)
            zs.append(z)
        lg = po.mlp_forward(m.sd, "_termination", torch.stack(zs))[..., 0].numpy().astype(np.float64)   # [H + 1, B]
        sm = mc.bce_logits(lg[1:], term.astype(np.float64)).mean(-1)
        ref[dt] = (lg, sm, sm.mean())
    names = ("term_logit", "step_means[3]", "termination_loss")
    gv = (got["term_logit"].cpu().numpy()[..., 0], got["step_means"].cpu().numpy()[3], got["losses"].cpu().numpy()[3])
    ov = (one["term_logit"].cpu().numpy()[..., 0], one["step_means"].cpu().numpy()[3], one["losses"].cpu().numpy()[3])
    for k, v, o, r64, r32 in zip(names, gv, ov, ref[torch.float64], ref[torch.float32]):
        gate = mc.tol(r64, np.abs(np.asarray(r32) - np.asarray(r64)).max())
        ratio = np.max(np.abs(v.astype(np.float64) - r64) / gate)
        rel = np.max(np.abs(v.astype(np.float64) - o) / np.maximum(1, np.abs(o)))
        print(f"[chunked termination prec {prec}] {k}: err / gate {ratio:.3f}, against one piece {rel:.2e}")
        _note("6 chunked termination", tight.planner, ratio)
        assert ratio <= 1 and rel <= 1e-5, k
    lg64 = ref[torch.float64][0]
    gate = mc.tol(lg64, np.abs(ref[torch.float32][0] - lg64).max())
    for label, (t, b) in (("the last row", (H, B - 1)), ("first row of the second piece", divmod(cap, B))):
        assert abs(gv[0][t, b] - lg64[t, b]) <= gate[t, b], label
        assert abs(gv[0][t, b] - ov[0][t, b]) <= 1e-5 * max(1, abs(ov[0][t, b])), label
    assert np.ptp(lg64) > 1   # the logits differ from row to row: a misplaced piece would show
    assert tight.planner.take_fault() == 0 and roomy.planner.take_fault() == 0


# ---------------------------------------------------------------- 7. non-finite targets
@pytest.mark.parametrize("name,path,prec", SMALL_RUNS)
def test_nan_target_poisons_exactly_its_losses(name, path, prec):
    """A NaN reward / td target / next_z / terminated makes exactly the losses that consume it NaN -- that loss, its step_means
    entry, total -- and the others keep the bits of the clean call (the reference: two_hot raises on the index, every torch op
    propagates NaN; a training loop that watches its losses must see it).  +-Inf targets stay finite: the vmin / vmax bin."""
    h = _handle(name, path, prec)
    cfg = h.cfg
    rows = mc.edge_logit_rows(cfg)
    rr, qr, tx = rows["n10"], np.stack([rows["n1"]] * cfg.num_q), 0.5
    h.bind("nonfinite", rr, qr, tx)
    for B, H, (t, b) in ((130, 3, (1, 77)), (1, 8, (5, 0)), (65, 2, (0, 64))):
        rng = np.random.default_rng(B)
        rew, td = rng.standard_normal((H, B)).astype(np.float32) * 5, rng.standard_normal((H, B)).astype(np.float32) * 50
        term = (rng.random((H, B)) < 0.3).astype(np.float32)
        nz = torch.as_tensor(rng.random((H, B, cfg.latent_dim)).astype(np.float32)).to(dev())
        clean = h.losses(B, H, rew, td, term=term, next_z=nz)
        assert torch.isfinite(clean["losses"]).all() and torch.isfinite(clean["step_means"]).all()

        def poisoned(kind, value):
            r, d, e, n = rew.copy(), td.copy(), term.copy(), nz.clone()
            if kind == 0:
                n[t, b, 3] = value
            else:
                (r, d, e)[kind - 1][t, b] = value
            return h.losses(B, H, r, d, term=e, next_z=n)

        kinds = [0, 1, 2] + ([3] if cfg.episodic else [])   # consistency <- next_z, reward <- reward, value <- td, termination <- terminated
        for kind in kinds:
            got = poisoned(kind, np.nan)
            ls, sm = got["losses"].cpu().numpy(), got["step_means"].cpu().numpy()
            cl, cs = clean["losses"].cpu().numpy(), clean["step_means"].cpu().numpy()
            assert np.isnan(ls[kind]) and np.isnan(ls[4]) and np.isnan(sm[kind, t]), (kind, B, H, ls, sm[kind])
            keep = np.ones((4, H), bool)
            keep[kind, t] = False
            assert np.array_equal(sm[keep].view(np.uint32), cs[keep].view(np.uint32)), (kind, B, H)
            others = [i for i in range(4) if i != kind]
            assert np.array_equal(ls[others].view(np.uint32), cl[others].view(np.uint32)), (kind, B, H, ls, cl)
        for kind in (1, 2):   # +-Inf: the clamped bin, the bits of any other target beyond the clamp
            for v in (np.inf, -np.inf):
                got, ref = poisoned(kind, v), poisoned(kind, np.float32(1e6) * np.sign(v))
                assert torch.isfinite(got["losses"]).all() and torch.isfinite(got["step_means"]).all()
                assert torch.equal(got["losses"], ref["losses"]) and torch.equal(got["step_means"], ref["step_means"]), (kind, v)
    assert h.planner.take_fault() == 0
