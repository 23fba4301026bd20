"""-m gpu: tdmpc2_plan_td_target / tdmpc2_plan_policy_value at their row and head edges, on both kernel families and in both
arithmetics (tests/value_common.py; tests/test_value_edges.py checks the restatement, the separation of the pinned rows and that the
gates admit the reference's own fp32).

Items 2a-2g run with PINNED HEADS: the last layer of every Q head is bound with weight 0 and bias l, a different l on every head and
on the two ensembles, so a call returns two_hot_inv of exactly two known rows through the tail, whatever pi and the hidden layers do.
Which head, which ensemble, which reduce, which row's reward / terminated / task then has an fp64 closed form.  Gate, per element:
max(1e-5 max(1, |reward|, |discount (1 - terminated) q64|), 2 |td_from fp32 - td_from fp64|).  Item 3 runs the case's own weights
against the fp64 oracle: max(1e-4 max(1, |reward|, |discount (1 - terminated) q64|), 2 |oracle fp32 - oracle fp64|).
The calls go through the C entry points directly: `out` and `action` are eight rows longer than asked and prefilled, and the eight
trailing rows must come back untouched.  TDMPC2_VALUE_EDGES_JSON=<file>: the worst err / gate per item, family and arithmetic is
written there (profiles/value_edges.json).

What bites, from five scratch builds of the library, each run once on the MI355X against this file (121 tests) and against
tests/test_gpu_td_target.py + tests/test_gpu_policy_loss.py (their 317M cases left out):
1. `BE_Q0 + q0` for the second head's first-layer bias in ks_value: the whole-chain test fails on mt5 fused in both arithmetics (the
   pinned items cannot see a hidden-layer bias); the older files fail too (5 tests, all mt5 fused).
2. fmaxf for fminf in the reduce (ks_value, l_value_head): head pairs, row counts, tail edges, non-finite inputs, multitask tables and
   the whole chain fail on every handle (94 tests); the older files fail 28.
3. `disc_tab[s_task[0]]` / `row_env[0]`: head pairs, row counts, multitask tables and the whole chain fail on every multitask handle
   (32 tests); the older files fail 8 (td_target on mt5, small_mt, c3: their two-valued discount table still differs by row).
4. `(1 - terminated)` dropped: the same 94 tests as under 2; the older files fail 27.
5. `q1 > q0` for `q1 >= q0` in the in-library draw (ks_value, l_qidx): the two in-library draw tests fail on every handle (21 tests:
   a call returns one head's value, which is no pair's mean); the older files PASS (73 of 73): nothing there reads the drawn pair."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import cases
from tests import value_common as vc
from tests.gpu_common import dev

pytestmark = pytest.mark.gpu

HANDLES = [("c1", 1), ("c1_ep", 1), ("mt5", 1), ("mt5", 2), ("small_ep", 2), ("small_mt", 2), ("tiny_mt", 0), ("c1_nb0", 1), ("small_nb1_ep", 2)]
RUNS = [(n, p, prec) for n, p in HANDLES for prec in (1, 2)]
REGRESSION = ("c1_nb0", "small_nb1_ep")   # items 2a-2d only
FULL_RUNS = [r for r in RUNS if r[0] not in REGRESSION]
MT_RUNS = [r for r in FULL_RUNS if r[0] in ("mt5", "small_mt", "tiny_mt")]
SEED = 11

_cases, _handles, _worst, _draws, _oracle = {}, {}, {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _dump_worst():
    yield
    path = os.environ.get("TDMPC2_VALUE_EDGES_JSON")
    if path:
        with open(path, "w") as f:
            json.dump({"gate": vc.GATES, "worst_err_over_gate": [dict(item=k[0], family=k[1], arithmetic=k[2], worst=v)
                                                                  for k, v in sorted(_worst.items())]}, f, indent=1)
            f.write("\n")


def d(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev())


def _case(name):
    if name not in _cases:
        _cases[name] = cases.build_case(name)
    return _cases[name]


class Handle:
    """One planner per (case, family, arithmetic), roomy enough for 257 rows; `bind` rebinds only when the pin changes."""

    def __init__(self, name, path, prec):
        from tdmpc2_amd.native import NativePlanner

        self.name, self.seen = name, 0.0
        self.c = c = _case(name)
        self.cfg = cfg = c["cfg"]
        self.sd = {k: torch.as_tensor(v) for k, v in c["sd"].items()}
        self.planner = NativePlanner(cfg, c["iterations"], dev(), max_envs=max(1, -(-257 // cfg.num_samples)), path=path, precision=prec)
        assert self.planner.path == (path or 2) and self.planner.precision == prec   # (path 0: the 64-wide models, layered only)
        self.layered = self.planner.path == 2
        self.tag = f"{name} path {self.planner.path} prec {prec}"
        self.bound = "nothing"
        self.n_tasks = len(cfg.tasks) if cfg.multitask else 0
        self.discount = float(c["discounts"][0]) if not cfg.multitask else None
        if cfg.multitask:
            emb = self.sd["_task_emb.weight"].to(torch.float32)
            norm = emb.norm(2, dim=-1, keepdim=True)
            emb = torch.where(norm > 1.0, emb * (1.0 / (norm + 1e-7)), emb)  # nn.Embedding(max_norm=1)
            self.emb, self.mask = emb.to(dev()).contiguous(), self.sd["_action_masks"].to(torch.float32).to(dev()).contiguous()
            self.disc_np = vc.distinct_discounts(self.n_tasks)
            self.disc_tab = d(self.disc_np)
        self._z = {}

    def bind(self, key):
        """key "pin": the case's weights with value_common's head rows pinned; None: the case's own weights."""
        if self.bound != key:
            self.planner.bind_state_dict(self.sd if key is None else vc.pin_value_heads(self.sd, self.cfg, *vc.head_rows(self.cfg)))
            self.bound = key
        return self

    def z(self, rows):
        from tdmpc2_amd import synth

        if rows not in self._z:
            self._z[rows] = synth.make_latents(self.cfg, rows, seed=rows)
        return self._z[rows]

    def _tables(self, R, tasks, disc_tab):
        if not self.cfg.multitask:
            return None, ()
        assert tasks.dtype == torch.int32 and tasks.shape == (R,) and tasks.is_contiguous()
        return self.planner._task_tables(R, tasks, self.emb, self.mask, disc_tab)

    def _call(self, fn, R, *args):
        p = self.planner
        with torch.cuda.device(dev()):
            p._check(fn(p._h, R, *args, p._stream()))

    def td(self, rows, reward, terminated, discount=None, tasks=None, pair=None, eps=None, seed=SEED, z=None, disc_tab=None):
        """tdmpc2_plan_td_target_mt on `rows` rows into an out of rows + 8 prefilled with the sentinel -> td [rows] (numpy).
        discount: the scalar of a single-task call; multitask: disc_tab (default: the distinct table)."""
        from tdmpc2_amd.native import _ptr

        zt, rw, tm = d(self.z(rows) if z is None else z), d(np.asarray(reward, np.float32)), d(np.asarray(terminated, np.float32))
        assert zt.shape == (rows, self.cfg.latent_dim) and rw.shape == tm.shape == (rows,)
        et = None if eps is None else d(eps)
        qi = None if pair is None else torch.tensor(pair, dtype=torch.int32, device=dev())
        tk = None if tasks is None else d(np.asarray(tasks, np.int32))
        tab = (self.disc_tab if disc_tab is None else disc_tab) if self.cfg.multitask else None
        tt, keep = self._tables(rows, tk, tab)
        out = torch.full((rows + 8,), vc.SENTINEL, device=dev())
        self._call(self.planner.lib.tdmpc2_plan_td_target_mt, rows, _ptr(zt), _ptr(rw), _ptr(tm),
                   C.c_float(0.0 if self.cfg.multitask else float(self.discount if discount is None else discount)), tt, _ptr(et), _ptr(qi),
                   C.c_uint64(seed), _ptr(out))
        res = out.cpu().numpy()
        assert (res[rows:] == np.float32(vc.SENTINEL)).all(), (self.tag, rows, res[rows:])
        return res[:rows]

    def pv(self, rows, target, reduce, tasks=None, pair=None, eps=None, seed=SEED, z=None):
        """tdmpc2_plan_policy_value_mt -> (action [rows, A], q [rows]) (numpy), both outputs eight sentinel rows longer."""
        from tdmpc2_amd.native import _ptr

        zt = d(self.z(rows) if z is None else z)
        assert zt.shape == (rows, self.cfg.latent_dim)
        et = None if eps is None else d(eps)
        qi = None if pair is None else torch.tensor(pair, dtype=torch.int32, device=dev())
        tk = None if tasks is None else d(np.asarray(tasks, np.int32))
        tt, keep = self._tables(rows, tk, None)
        act = torch.full((rows + 8, self.cfg.action_dim), vc.SENTINEL, device=dev())
        q = torch.full((rows + 8,), vc.SENTINEL, device=dev())
        self._call(self.planner.lib.tdmpc2_plan_policy_value_mt, rows, _ptr(zt), tt, int(bool(target)), int(reduce == "min"), _ptr(et), _ptr(qi),
                   C.c_uint64(seed), _ptr(act), _ptr(q))
        a, v = act.cpu().numpy(), q.cpu().numpy()
        assert (a[rows:] == np.float32(vc.SENTINEL)).all() and (v[rows:] == np.float32(vc.SENTINEL)).all(), (self.tag, rows)
        return a[:rows], v[:rows]

    def tasks(self, kind, rows):
        return vc.task_pattern(kind, rows, self.n_tasks) if self.cfg.multitask else None

    def disc_rows(self, tasks, discount=None):
        """The discount of every row as the library is given it: fp32."""
        return self.disc_np[tasks] if self.cfg.multitask else np.float32(self.discount if discount is None else discount)


def _handle(name, path, prec):
    key = (name, path, prec)
    if key not in _handles:
        _handles[key] = Handle(name, path, prec)
    _handles[key].seen = 0.0
    return _handles[key]


def _done(h, item):
    print(f"[{h.tag}] {item}: worst err / gate {h.seen:.3f}")
    assert h.planner.take_fault() == 0


def _note(item, h, ratio):
    key = (item, "layered" if h.layered else "fused", "fp32" if h.planner.precision == 1 else "split")
    _worst[key] = max(_worst.get(key, 0.0), float(ratio))


def _gated(item, h, got, v64, gate, what):
    with np.errstate(all="ignore"):
        ratio = np.atleast_1d(np.abs(got.astype(np.float64) - v64) / gate)
    i = int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)))
    _note(item, h, ratio[i] if np.isfinite(ratio[i]) else 1e30)
    h.seen = max(h.seen, float(ratio[i]))
    assert ratio[i] <= 1, f"[{h.tag}] {item} {what}: row {i} of {len(ratio)}: got {np.atleast_1d(got)[i]!r}, closed form {np.atleast_1d(v64)[i]!r}, err / gate {ratio[i]:.3f}"


def _row_cap(h):
    """The rows the layered workspace holds, AS THE LIBRARY REPORTS IT in its refusal of an oversized call."""
    from tdmpc2_amd.native import NativeError

    R = 1 << 14
    with pytest.raises(NativeError) as ex:
        h.pv(R, False, "avg", tasks=h.tasks("all0", R), pair=(0, 1), z=np.zeros((R, h.cfg.latent_dim), np.float32))
    m = re.search(r"workspace holds (\d+) rows", str(ex.value))
    assert m, str(ex.value)
    return int(m.group(1))


# ---------------------------------------------------------------- 2a. every ordered head pair, both reduces, both ensembles
@pytest.mark.parametrize("name,path,prec", RUNS)
def test_every_ordered_head_pair(name, path, prec):
    h = _handle(name, path, prec).bind("pin")
    cfg, R = h.cfg, 65
    rew, term = vc.row_inputs(R)
    tasks = h.tasks("mod7", R)
    for pair in vc.ordered_pairs(cfg.num_q):
        for target in (False, True):
            for red in ("min", "avg"):
                _, q = h.pv(R, target, red, tasks=tasks, pair=pair)
                v64, _, gate = vc.pinned_expect(cfg, target, pair, red)
                _gated("2a head pairs", h, q, np.full(R, v64), gate, f"pair {pair} target {target} {red}")
        td = h.td(R, rew, term, tasks=tasks, pair=pair)
        v64, _, gate = vc.pinned_expect(cfg, True, pair, "min", rew, term, h.disc_rows(tasks))
        _gated("2a head pairs", h, td, v64, gate, f"pair {pair} td_target")
    _done(h, "2a head pairs")


# ---------------------------------------------------------------- 2b. row counts
@pytest.mark.parametrize("name,path,prec", RUNS)
def test_row_counts_every_row(name, path, prec):
    """Every row of every count against the closed form of ITS reward / terminated / task; the eight rows behind the last stay untouched
    (Handle.td / Handle.pv).  Layered handles: also cap - 1 and cap rows, and cap + 1 is refused with the capacity named."""
    from tdmpc2_amd.native import NativeError

    h = _handle(name, path, prec).bind("pin")
    cfg = h.cfg
    counts = list(vc.ROW_COUNTS)
    if h.layered:
        cap = _row_cap(h)
        assert cap >= 257 and cap % 128 == 0
        counts += [cap - 1, cap]
    for R in counts:
        tasks = h.tasks("mod7", R)
        for big in (False, True):
            rew, term = vc.row_inputs(R, big)
            td = h.td(R, rew, term, tasks=tasks, pair=(0, 2))
            v64, _, gate = vc.pinned_expect(cfg, True, (0, 2), "min", rew, term, h.disc_rows(tasks))
            _gated("2b row counts", h, td, v64, gate, f"rows {R} big {big}")
        a, q = h.pv(R, False, "avg", tasks=tasks, pair=(1, 0))
        v64, _, gate = vc.pinned_expect(cfg, False, (1, 0), "avg")
        _gated("2b row counts", h, q, np.full(R, v64), gate, f"rows {R} policy_value")
        assert np.isfinite(a).all() and np.abs(a).max() <= 1
    if h.layered:
        R = cap + 1
        rew, term = vc.row_inputs(R)
        with pytest.raises(NativeError, match=f"error 1: the layered workspace holds {cap} rows"):
            h.td(R, rew, term, tasks=h.tasks("mod7", R), pair=(0, 2))
        with pytest.raises(NativeError, match=f"workspace holds {cap} rows"):
            h.pv(R, False, "avg", tasks=h.tasks("mod7", R), pair=(1, 0))
    _done(h, "2b row counts")


# ---------------------------------------------------------------- 2c. tail edges
@pytest.mark.parametrize("name,path,prec", RUNS)
def test_tail_edges(name, path, prec):
    """reward x terminated x discount of vc.tail_table on the target pairs (0, 2) -- hot100 and hot0, min = symexp(-10) -- and (1, 0):
    one row per call, and the 50 combinations of each discount together in one 64-row call.  Multitask handles take the four
    discounts from a table through the row's task.  terminated = 1 and discount = 0: td == reward, bit for bit where the reward is
    not a zero (reward + (+-0) q: the sum of two zeros takes its sign from q's, as in the reference; -0 + 0 = +0)."""
    h = _handle(name, path, prec).bind("pin")
    cfg = h.cfg
    mt = cfg.multitask
    tab = None
    if mt:
        t = np.full(h.n_tasks, 0.9, np.float32)
        t[:4] = vc.TAIL_DISCOUNTS
        tab = d(t)

    def check(rew, term, disc, dv, pair, what, R=None):
        n = len(rew)
        R = n if R is None else R
        idx = np.arange(R) % n
        rew, term, disc = rew[idx], term[idx], disc[idx]
        assert len(set(disc.tolist())) == 1
        assert disc[0] == np.float32(dv)
        tasks = np.full(R, vc.TAIL_DISCOUNTS.index(dv), np.int32) if mt else None
        td = h.td(R, rew, term, discount=dv, tasks=tasks, pair=pair, disc_tab=tab)
        v64, v32, gate = vc.pinned_expect(cfg, True, pair, "min", rew, term, disc)
        _gated("2c tail edges", h, td, v64, gate, what)
        exact = (term == 1) | (disc == 0)
        assert np.array_equal(td[exact], rew[exact]), (h.tag, what)
        nz = exact & (rew != 0)
        assert np.array_equal(td[nz].view(np.uint32), rew[nz].view(np.uint32)), (h.tag, what)

    for pair in ((0, 2), (1, 0)):
        q32 = vc.pinned_expect(cfg, True, pair, "min")[1]
        rew, term, disc = vc.tail_table(q32)
        for dv in vc.TAIL_DISCOUNTS:
            m = disc == np.float32(dv)
            check(rew[m], term[m], disc[m], dv, pair, f"pair {pair} discount {dv} together", R=64)
            if pair == (0, 2):
                for i in np.nonzero(m)[0]:
                    check(rew[i:i + 1], term[i:i + 1], disc[i:i + 1], dv, pair, f"pair {pair} reward {rew[i]!r} terminated {term[i]!r} discount {dv}")
    _done(h, "2c tail edges")


# ---------------------------------------------------------------- 2d. non-finite inputs
@pytest.mark.parametrize("name,path,prec", RUNS)
def test_non_finite_inputs_poison_exactly_their_row(name, path, prec):
    h = _handle(name, path, prec).bind("pin")
    cfg, R = h.cfg, 130
    rows = [0, 63, 64, R - 1]
    keep = np.ones(R, bool)
    keep[rows] = False
    tasks = h.tasks("mod7", R)
    rew, term = vc.row_inputs(R)
    for pair in ((0, 2), (2, 1)):   # min = the pinned value of target head 2, far from 0: inf x q has a sign
        clean = h.td(R, rew, term, tasks=tasks, pair=pair)
        assert np.isfinite(clean).all()
        for which in (0, 1):
            for v in (np.nan, np.inf, -np.inf):
                r, t = rew.copy(), term.copy()
                (r, t)[which][rows] = v
                got = h.td(R, r, t, tasks=tasks, pair=pair)
                q32 = vc.head_values(cfg, np.float32)[1]
                want = vc.td_from(q32[pair[0]], q32[pair[1]], r, t, h.disc_rows(tasks), "min", np.float32)
                assert not np.isfinite(want[rows]).any()
                assert np.array_equal(got[rows], want[rows], equal_nan=True), (h.tag, pair, which, v, got[rows], want[rows])
                assert np.array_equal(got[keep].view(np.uint32), clean[keep].view(np.uint32)), (h.tag, pair, which, v)
    assert h.planner.take_fault() == 0


# ---------------------------------------------------------------- 2e. multitask tables
@pytest.mark.parametrize("name,path,prec", MT_RUNS)
def test_multitask_tables_row_by_row(name, path, prec):
    """A different discount for every task: td[row] = reward[row] + disc[task[row]] (1 - terminated[row]) q in closed form, so a
    discount, reward or terminated taken from another row or task changes the number.  policy_value's action: exactly zero in the
    dimensions the row's own task masks, nonzero somewhere in the others."""
    h = _handle(name, path, prec).bind("pin")
    cfg = h.cfg
    mask = h.mask.cpu().numpy()
    assert (mask.sum(-1) < cfg.action_dim).any() and (mask.sum(-1) > 0).all()   # some task masks something, none masks all
    for kind in vc.TASK_PATTERNS:
        for R in (63, 64, 65, 130):
            tasks = h.tasks(kind, R)
            rew, term = vc.row_inputs(R)
            td = h.td(R, rew, term, tasks=tasks, pair=(0, 2))
            v64, _, gate = vc.pinned_expect(cfg, True, (0, 2), "min", rew, term, h.disc_rows(tasks))
            _gated("2e multitask tables", h, td, v64, gate, f"{kind} rows {R}")
            a, q = h.pv(R, True, "min", tasks=tasks, pair=(2, 1))
            v64, _, gate = vc.pinned_expect(cfg, True, (2, 1), "min")
            _gated("2e multitask tables", h, q, np.full(R, v64), gate, f"{kind} rows {R} policy_value")
            m = mask[tasks]
            assert not (a * (1 - m)).any(), (h.tag, kind, R)
            assert (np.abs(a * m).sum(-1) > 0).all(), (h.tag, kind, R)
    _done(h, "2e multitask tables")


# ---------------------------------------------------------------- 2f. the task_rows regrow (layered multitask)
@pytest.mark.parametrize("name,path,prec", [r for r in MT_RUNS if r[1] != 1])
def test_task_rows_regrow(name, path, prec):
    """5 rows, 257, 5 again on one handle (the row -> task copy grows at the second call), the case's own weights, noise and heads
    given: both 5-row results equal bit for bit, equal to a fresh handle's, and the 257-row result to another fresh handle's."""
    def run(h, R):
        tasks = h.tasks("mod7", R)
        rew, term = vc.row_inputs(R)
        eps = vc.chain_eps(R, h.cfg.action_dim)
        a, q = h.pv(R, False, "avg", tasks=tasks, pair=(0, 1), eps=eps)
        return h.td(R, rew, term, tasks=tasks, pair=(1, 2), eps=eps), a, q

    bits = lambda xs: [x.view(np.uint32) for x in xs]
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))
    one, five, big = (Handle(name, path, prec).bind(None) for _ in range(3))
    first, grown, again = run(one, 5), run(one, 257), run(one, 5)
    assert all(np.isfinite(x).all() for x in first + grown)
    assert same(first, again) and same(first, run(five, 5)) and same(grown, run(big, 257))
    assert np.ptp(grown[0]) > 0
    for h in (one, five, big):
        assert h.planner.take_fault() == 0
        h.planner.close()


# ---------------------------------------------------------------- 2g. the in-library head draw
def _identify(cfg, q):
    """The unordered pair whose mean the 8 returned values are (test_value_edges.py: the means are 100 gates apart)."""
    import itertools

    hits = []
    for pair in itertools.combinations(range(cfg.num_q), 2):
        v64, _, gate = vc.pinned_expect(cfg, False, pair, "avg")
        if (np.abs(q.astype(np.float64) - v64) <= gate).all():
            hits.append(pair)
    return hits


def _draw_seq(h):
    """The pair each of 200 calls (seed, call = k) draws, identified from the returned mean; once per handle."""
    key = (h.name, h.planner.path, h.planner.precision)
    if key not in _draws:
        h.bind("pin")
        tasks = h.tasks("mod7", 8)
        seq = []
        for k in range(200):
            h.planner.set_call_counter(k)
            _, q = h.pv(8, False, "avg", tasks=tasks, pair=None, seed=SEED)
            hits = _identify(h.cfg, q)
            assert len(hits) == 1, (h.tag, k, q, hits)   # (two equal heads would return one head's value: no pair's mean)
            seq.append(hits[0])
        assert h.planner.call_counter() == 200
        _draws[key] = seq
    return _draws[key]


@pytest.mark.parametrize("name,path,prec", FULL_RUNS)
def test_in_library_head_draw(name, path, prec):
    """qidx = None: 200 calls under (seed, call = k), 8 rows, avg.  Each returns the mean of exactly one pair of two DIFFERENT heads and
    all num_q choose 2 pairs occur (a uniform draw misses one with probability about 10 x 0.9^200; the run is deterministic)."""
    h = _handle(name, path, prec)
    seq = _draw_seq(h)
    assert len(set(seq)) == h.cfg.num_q * (h.cfg.num_q - 1) // 2, (h.tag, sorted(set(seq)))
    assert h.planner.take_fault() == 0


@pytest.mark.parametrize("name,a,b", [("mt5", (1, 1), (2, 1)), ("mt5", (1, 2), (2, 2)), ("mt5", (1, 1), (1, 2)), ("mt5", (2, 1), (2, 2)),
                                      ("c1", (1, 1), (1, 2)), ("small_mt", (2, 1), (2, 2)), ("tiny_mt", (0, 1), (0, 2))])
def test_in_library_head_draw_agrees(name, a, b):
    """The same pair at every k on the fused and the layered family (they implement the draw twice) and in the two arithmetics."""
    sa, sb = _draw_seq(_handle(name, *a)), _draw_seq(_handle(name, *b))
    assert sa == sb, (name, a, b, [k for k in range(200) if sa[k] != sb[k]][:5])


# ---------------------------------------------------------------- 3. the case's own weights against the fp64 oracle
def _chain_oracle(h, rows, kind):
    key = (h.name, rows, kind)
    if key not in _oracle:
        _oracle[key] = vc.oracle_chain(h.cfg, h.c["sd"], h.z(rows), vc.chain_eps(rows, h.cfg.action_dim), h.tasks(kind, rows))
    return _oracle[key]


@pytest.mark.parametrize("name,path,prec", FULL_RUNS)
def test_whole_chain_against_the_fp64_oracle(name, path, prec):
    """pi, both heads and the tail on the case's own weights: 1, 63, 64, 65, 129 rows, noise with saturated rows, every ordered head
    pair at 65 rows on c1 and mt5 (the fixture's pair and its reverse elsewhere), td_target and policy_value over both reduces
    and both ensembles, two task patterns and the distinct discount table on multitask handles; the action against the oracle's."""
    h = _handle(name, path, prec).bind(None)
    cfg = h.cfg
    fixture = tuple(int(i) for i in cases.td_batch(cfg)["qidx"])
    for kind in (("mod", "mod7") if cfg.multitask else (None,)):
        for R in (1, 63, 64, 65, 129):
            o32, o64 = _chain_oracle(h, R, kind)
            eps, tasks = vc.chain_eps(R, cfg.action_dim), h.tasks(kind, R)
            rew, term = vc.row_inputs(R)
            pairs = vc.ordered_pairs(cfg.num_q) if (R == 65 and name in ("c1", "mt5")) else [fixture, fixture[::-1]]
            a_gate = np.maximum(2e-5, 2 * np.abs(o32[0] - o64[0]))
            for pair in pairs:
                td = h.td(R, rew, term, tasks=tasks, pair=pair, eps=eps)
                v64, gate = vc.chain_expect(o32, o64, True, pair, "min", rew, term, h.disc_rows(tasks))
                _gated("3 whole chain", h, td, v64, gate, f"{kind} rows {R} pair {pair} td_target")
                for target in (False, True):
                    for red in ("min", "avg"):
                        a, q = h.pv(R, target, red, tasks=tasks, pair=pair, eps=eps)
                        v64, gate = vc.chain_expect(o32, o64, target, pair, red)
                        _gated("3 whole chain", h, q, v64, gate, f"{kind} rows {R} pair {pair} target {target} {red}")
                        _gated("3 action", h, a.reshape(-1), o64[0].reshape(-1), a_gate.reshape(-1), f"{kind} rows {R} pair {pair}")
    _done(h, "3 whole chain")
