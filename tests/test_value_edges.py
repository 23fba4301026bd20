"""CPU: what tests/test_gpu_value_edges.py gates against, before any kernel sees it (tests/value_common.py).  td_from equals the tail
of oracle.planner_oracle.td_target bit for bit in fp32 and the reference-minted td_target fixtures in fp64; the pinned head rows are
separated (every head a different value, every pair mean apart by more than 100 gates, so a returned mean names its pair); and the
pinned gate admits the reference: the oracle's own fp32 result lies inside it on every combination the GPU file runs.  A combination
at which the reference alone left the gate would be listed in value_common.REMOVED with its measured ratio (none is; at most 2 %).
Measured here: worst reference err / gate 0.07 on pinned heads (7 426 combinations on c1; the pair of off-300 and n10 under avg)."""
import numpy as np
import pytest
import torch

from oracle import cases
from oracle import planner_oracle as po
from tdmpc2_amd import synth
from tests import model_common as mc
from tests import value_common as vc
from tests.helpers import load_golden

PIN_CASES = ("c1", "small_ep", "tiny_mt", "c1_nb0", "small_nb1_ep")   # num_q 5 / 3 / 3 (multitask), regression heads 0 and 1
_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = cases.build_case(name)
    return _cases[name]


class _FedQ:
    """A model whose two heads return given values: oracle.td_target / policy_value run their own tail on them."""

    def __init__(self, qa, qb):
        self.qa, self.qb = torch.as_tensor(qa), torch.as_tensor(qb)

    def pi(self, z, task, eps):
        return torch.zeros(z.shape[0], 1)

    def Q_pair(self, z, a, task, qidx, return_type="min", target=False):
        Q = torch.stack([self.qa, self.qb])[..., None]
        return Q.min(0).values if return_type == "min" else Q.sum(0) / 2   # (OracleModel.Q_pair's last line)


def test_td_from_fp32_is_the_oracle_tail_bit_for_bit():
    rng = np.random.default_rng(1)
    qa, qb = (rng.standard_normal(200) * 100).astype(np.float32), (rng.standard_normal(200) * 100).astype(np.float32)
    for q32 in (np.float32(-22025.467), np.float32(2.1289895)):
        rew, term, disc = vc.tail_table(q32)
        keep = np.isfinite(rew)
        z = torch.zeros(len(rew), 4)
        for d in vc.TAIL_DISCOUNTS:
            m = disc == np.float32(d)
            want = po.td_target(_FedQ(qa[m], qb[m]), z[m], torch.as_tensor(rew[m])[:, None], torch.as_tensor(term[m])[:, None], None, d,
                                torch.zeros(m.sum(), 1), torch.tensor([0, 1]))[:, 0].numpy()
            got = vc.td_from(qa[m], qb[m], rew[m], term[m], np.float32(d), "min", np.float32)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), d
        assert keep.all()
    # a per-row discount tensor (multitask, tdmpc2.py:249-250) and the bare reduces
    disc = vc.distinct_discounts(30)[np.arange(200) % 30]
    rew, term = vc.row_inputs(200, big=True)
    want = po.td_target(_FedQ(qa, qb), torch.zeros(200, 4), torch.as_tensor(rew)[:, None], torch.as_tensor(term)[:, None], None,
                        torch.as_tensor(disc)[:, None], torch.zeros(200, 1), torch.tensor([0, 1]))[:, 0].numpy()
    assert np.array_equal(vc.td_from(qa, qb, rew, term, disc, "min", np.float32), want)
    _, avg = po.policy_value(_FedQ(qa, qb), torch.zeros(200, 4), None, torch.zeros(200, 1), torch.tensor([0, 1]))
    assert np.array_equal(vc.td_from(qa, qb, None, None, None, "avg", np.float32), avg[:, 0].numpy())
    assert np.array_equal(vc.td_from(qa, qb, None, None, None, "min", np.float32), np.minimum(qa, qb))


@pytest.mark.parametrize("name", ["c1", "mt5", "small_ep"])
def test_td_from_fp64_agrees_with_the_reference_fixture(name):
    """The stored `td_target` (the reference's own _td_target) against td_from in fp64 on the fp32 oracle's Q, under the unpinned gate."""
    from tdmpc2_amd.config import get_discount

    c = _case(name)
    cfg = c["cfg"]
    tb = cases.td_batch(cfg)
    H, B = tb["reward"].shape[:2]
    z, eps = tb["next_z"].reshape(H * B, -1), tb["pi_eps"].reshape(H * B, -1)
    task = np.tile(tb["tasks"], H) if cfg.multitask else None
    disc = (np.array([get_discount(cfg, ln) for ln in cfg.episode_lengths], np.float32)[task] if cfg.multitask
            else np.float32(c["discounts"][0]))
    o32, o64 = vc.oracle_chain(cfg, c["sd"], z, eps, task)
    pair = tuple(int(i) for i in tb["qidx"])
    rew, term = tb["reward"].reshape(-1), tb["terminated"].reshape(-1)
    q32 = o32[1][1].astype(np.float32)
    v = vc.td_from(q32[pair[0]], q32[pair[1]], rew, term, disc, "min", np.float64)
    _, gate = vc.chain_expect(o32, o64, True, pair, "min", rew, term, disc)
    ratio = np.abs(v - load_golden(name)["td_target"].reshape(-1).astype(np.float64)) / gate
    print(f"[{name}] td_from fp64 on the fp32 oracle's Q against the fixture: worst err / gate {ratio.max():.3f}")
    assert ratio.max() <= 1
    # the helper evaluates the heads as OracleModel.Q_pair does, and the unpinned gate admits the oracle's own fp32
    m = po.OracleModel(cfg, {k: torch.as_tensor(x) for k, x in c["sd"].items()})
    tk = None if task is None else torch.as_tensor(task.astype(np.int64))
    a = m.pi(torch.as_tensor(z), tk, torch.as_tensor(eps))
    for target in (False, True):
        for red in ("min", "avg"):
            want = m.Q_pair(torch.as_tensor(z), a, tk, torch.as_tensor(tb["qidx"]), red, target)[:, 0].numpy()
            got = vc.reduce_of(o32[1][int(target)][pair[0]], o32[1][int(target)][pair[1]], red).astype(np.float32)
            assert np.array_equal(got, want), (target, red)
            v64, g = vc.chain_expect(o32, o64, target, pair, red)
            assert (np.abs(want - v64) <= g).all()


@pytest.mark.parametrize("name", PIN_CASES)
def test_head_rows_are_separated(name):
    cfg = _case(name)["cfg"]
    on, tg = vc.head_rows(cfg)
    assert on.shape == tg.shape == (cfg.num_q, max(cfg.num_bins, 1)) and on.dtype == np.float32
    if cfg.num_bins > 1:
        assert mc_names_ok() and "hot0" in vc.TARGET_ROWS[:3] and "hot100" in vc.TARGET_ROWS[:3]   # the tail edges run on these
    ratios, distinct = vc.separation(cfg)
    print(f"[{name}] pair means apart by {ratios[0]:.1f} (online) / {ratios[1]:.1f} (target) x 100 gates")
    assert distinct and min(ratios) > 1
    # ... and the two ensembles answer differently on every ordered pair and reduce: a wrong use_target shows
    for pair in vc.ordered_pairs(cfg.num_q):
        for red in ("min", "avg"):
            a, _, ga = vc.pinned_expect(cfg, False, pair, red)
            b, _, gb = vc.pinned_expect(cfg, True, pair, red)
            assert abs(a - b) > 100 * max(ga, gb), (pair, red, a, b)
    # every ordered pair gives its own (min, avg) within an ensemble, except its reverse
    for target in (False, True):
        seen = {}
        for pair in vc.ordered_pairs(cfg.num_q):
            key = tuple(float(vc.pinned_expect(cfg, target, pair, red)[0]) for red in ("min", "avg"))
            assert seen.setdefault(key, frozenset(pair)) == frozenset(pair), (pair, seen[key])


def mc_names_ok():
    allowed = {"zero", "n1", "n10", "hot0", "hot50", "hot100", "twomax", "off+300", "off-300"}
    return set(vc.ONLINE_ROWS) <= allowed and set(vc.TARGET_ROWS) <= allowed


def _oracle_pinned(name):
    c = _case(name)
    cfg = c["cfg"]
    sd = vc.pin_value_heads(c["sd"], cfg, *vc.head_rows(cfg))
    return c, cfg, po.OracleModel(cfg, sd)


def test_pin_value_heads_pins_the_two_ensembles_differently():
    c, cfg, m = _oracle_pinned("small_ep")
    on, tg = vc.head_rows(cfg)
    assert np.array_equal(m.sd["_Qs.params.2.bias"].numpy(), on) and np.array_equal(m.sd["_target_Qs_params.2.bias"].numpy(), tg)
    assert not m.sd["_Qs.params.2.weight"].any() and not m.sd["_target_Qs_params.2.weight"].any()
    assert torch.equal(m.sd["_pi.2.weight"], torch.as_tensor(c["sd"]["_pi.2.weight"]))   # nothing else moves
    plain = mc.pin_heads(c["sd"], cfg, q_rows=on)   # existing callers: both ensembles alike
    assert torch.equal(plain["_Qs.params.2.bias"], plain["_target_Qs_params.2.bias"])


@pytest.mark.parametrize("name", PIN_CASES)
def test_pinned_gate_admits_the_reference_fp32(name):
    """Every (head pair, reward, terminated, discount, reduce) the GPU file runs on pinned heads, through the ORACLE in fp32
    (OracleModel.pi, Q_pair on the pinned state dict, the tail of td_target): err / gate <= 1 against the fp64 closed form."""
    c, cfg, m = _oracle_pinned(name)
    n = len(cfg.tasks) if cfg.multitask else 0
    worst, count, removed = (0.0, ()), 0, 0

    def run(rows, target, pair, red, rew=None, term=None, disc=None, what=""):
        nonlocal worst, count, removed
        z = torch.as_tensor(synth.make_latents(cfg, rows, seed=rows))
        tk = torch.as_tensor(vc.task_pattern("mod", rows, n).astype(np.int64)) if n else None
        a = m.pi(z, tk, torch.zeros(rows, cfg.action_dim))
        q = m.Q_pair(z, a, tk, torch.tensor(pair), red, target)
        if rew is not None:
            q = torch.as_tensor(rew)[:, None] + torch.as_tensor(disc).reshape(-1, 1) * (1 - torch.as_tensor(term)[:, None]) * q   # planner_oracle.py: td_target
        got = q[:, 0].numpy().astype(np.float64)
        v64, v32, gate = vc.pinned_expect(cfg, target, pair, red, rew, term, disc)
        with np.errstate(all="ignore"):
            ratio = np.abs(got - v64) / gate
        for i, r in enumerate(np.atleast_1d(ratio)):
            key = (name, what, target, pair, red, i)
            count += 1
            if key in vc.REMOVED:
                removed += 1
                continue
            assert r <= 1, (key, r)
            worst = max(worst, (float(r), key))

    for pair in vc.ordered_pairs(cfg.num_q):   # item 2a
        for red in ("min", "avg"):
            for target in (False, True):
                run(65, target, pair, red, what="2a")
        rew, term = vc.row_inputs(65)
        run(65, True, pair, "min", rew, term, np.full(65, 0.99, np.float32), what="2a td")
    for rows in (1, 5, 257):   # item 2b (a row count changes nothing on the host: three of them)
        for big in (False, True):
            rew, term = vc.row_inputs(rows, big)
            run(rows, True, (0, 2), "min", rew, term, np.full(rows, 0.99, np.float32), what=f"2b big {big}")
    for pair in ((0, 2), (1, 0)):   # item 2c
        q32 = vc.pinned_expect(cfg, True, pair, "min")[1]
        rew, term, disc = vc.tail_table(q32)
        run(len(rew), True, pair, "min", rew, term, disc, what="2c")
    if n:   # item 2e: the distinct discount table through the row's task
        for rows in (63, 130):
            rew, term = vc.row_inputs(rows)
            run(rows, True, (0, 2), "min", rew, term, vc.distinct_discounts(n)[vc.task_pattern("mod", rows, n)], what="2e")
    print(f"[{name}] {count} combinations, worst reference err / gate {worst[0]:.3f} at {worst[1]}; removed {removed}")
    assert removed <= 0.02 * count and len(vc.REMOVED) <= 0.02 * count


def test_tables_are_what_the_issue_lists():
    assert vc.ROW_COUNTS == (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
    rew, term, disc = vc.tail_table(np.float32(-22025.467))
    assert len(rew) == 10 * 5 * 4 and np.isfinite(rew).all()
    assert np.signbit(rew[5]) and rew[5] == 0 and np.float32(3e38) in rew and np.float32(1 - 2.0 ** -24) in term and term.max() == 2
    assert (rew[disc == 1][45:50] == np.float32(22025.467)).all()   # the cancelling reward at discount 1
    d = vc.distinct_discounts(30)
    assert d.dtype == np.float32 and len(set(d.tolist())) == 30 and abs(d[29] - 1.19) < 1e-6
    for kind in vc.TASK_PATTERNS:
        for rows in (63, 64, 65, 130):
            t = vc.task_pattern(kind, rows, 30)
            assert t.dtype == np.int32 and t.shape == (rows,) and t.min() >= 0 and t.max() < 30
    assert vc.task_pattern("lastonly", 65, 30)[-1] == 29 and not vc.task_pattern("lastonly", 65, 30)[:-1].any()
    assert len(set(vc.task_pattern("blocks64", 130, 30).tolist())) == 3
    eps = vc.chain_eps(65, 6)
    assert not eps[0].any() and (eps[1] == 5).all() and (eps[2] == -5).all() and set(eps[3].tolist()) == {5.0, -5.0}
    assert vc.chain_eps(1, 6).shape == (1, 6)
