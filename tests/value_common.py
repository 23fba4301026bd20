"""Shared by tests/test_value_edges.py (CPU) and tests/test_gpu_value_edges.py (-m gpu): the tail of TDMPC2._td_target / update_pi
(reference tdmpc2/tdmpc2.py:239-254, 208-225) restated in numpy, the pinned head rows of both ensembles, the input tables and the
two gates.  Nothing here comes from a HIP result."""
import itertools

import numpy as np

from tests import model_common as mc

PIN_FLOOR = 1e-5     # pinned heads: the project's loss-stage floor (mc.EDGE_FLOOR)
CHAIN_FLOOR = 1e-4   # the case's own weights: the layer code's gate (mc.RTOL)
GATES = {"pinned": "max(1e-5 max(1, |reward|, |discount (1 - terminated) q64|), 2 |td_from fp32 - td_from fp64|)",
         "unpinned": "max(1e-4 max(1, |reward|, |discount (1 - terminated) q64|), 2 |oracle fp32 - oracle fp64|); "
                     "action: max(2e-5, 2 |oracle fp32 - oracle fp64|)"}
SENTINEL = -7.25
ROW_COUNTS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
TERM_CYCLE = (0.0, 1.0, 0.3, 0.0, 0.0, 1.0, 0.75)

# One logits row per head (names of mc.edge_logit_rows), a different value on every head and a different row on the same head of
# the two ensembles.  Values: n1 2.13, twomax -9.96, n10 90.6, off+-300 -178.7, zero 0, hot0 / hot100 -+22025.5 (symexp(-+10)).
ONLINE_ROWS = ("n1", "twomax", "off+300", "n10", "zero")
TARGET_ROWS = ("hot100", "zero", "hot0", "off-300", "n10")
# regression heads (num_bins 0: the output is the value; 1: symexp of it, math.py:76-79): the one output column of every head
ONLINE_REG = (0.75, -2.4, -5.2, 4.5, 0.0)
TARGET_REG = (10.0, 0.0, -10.0, -5.2, 4.5)

# combinations at which the REFERENCE's own fp32 leaves the pinned gate (tests/test_value_edges.py measures it), with the measured
# err / gate: not asked of the library either.  At most 2 % of a table.
REMOVED = {}


def two_hot_inv_rows(logits, cfg):
    """mc.two_hot_inv_rows with the regression heads of math.py:76-79: logits [..., max(bins, 1)] -> [...]."""
    if cfg.num_bins == 0:
        return logits[..., 0]
    if cfg.num_bins == 1:
        return mc.symexp(logits[..., 0])
    return mc.two_hot_inv_rows(logits, cfg)


def head_rows(cfg):
    """(online [num_q, cols], target [num_q, cols]) fp32 logits, cols = max(num_bins, 1)."""
    nq = cfg.num_q
    if cfg.num_bins <= 1:
        return (np.array(ONLINE_REG[:nq], np.float32)[:, None], np.array(TARGET_REG[:nq], np.float32)[:, None])
    rows = mc.edge_logit_rows(cfg)
    return np.stack([rows[n] for n in ONLINE_ROWS[:nq]]), np.stack([rows[n] for n in TARGET_ROWS[:nq]])


def head_values(cfg, dtype):
    """(online [num_q], target [num_q]): two_hot_inv of the pinned rows evaluated in `dtype` from the fp32 logits."""
    return tuple(two_hot_inv_rows(r.astype(dtype), cfg) for r in head_rows(cfg))


def pin_value_heads(sd, cfg, online_rows, target_rows):
    """mc.pin_heads for the Q heads with DIFFERENT rows on the online (`_Qs`, `_detach_Qs`) and the target ensemble."""
    out = mc.pin_heads(sd, cfg, q_rows=online_rows)
    tgt = mc.pin_heads({k: v for k, v in sd.items() if k.startswith("_target_Qs_params.2.")}, cfg, q_rows=target_rows)
    out.update(tgt)
    return out


def ordered_pairs(nq):
    return [(a, b) for a in range(nq) for b in range(nq) if a != b]


def reduce_of(q_a, q_b, reduce):
    """world_model.py:213-216 on two heads: Q.min(0) | Q.sum(0) / 2."""
    return np.minimum(q_a, q_b) if reduce == "min" else (q_a + q_b) / 2


def td_from(q_a, q_b, reward, terminated, discount, reduce, dtype):
    """reward + discount (1 - terminated) (min | mean)(q_a, q_b) (tdmpc2.py:239-254), evaluated in `dtype` from fp32 inputs in the
    reference's order of operations; reward None: the bare reduce (what policy_value returns)."""
    c = lambda v: np.asarray(v, np.float32).astype(dtype)
    with np.errstate(all="ignore"):
        q = reduce_of(c(q_a), c(q_b), reduce)
        if reward is None:
            return q
        return c(reward) + c(discount) * (1 - c(terminated)) * q


def term_scale(q64, reward, terminated, discount):
    """max(1, |reward|, |discount (1 - terminated) q64|): the largest term of the sum, in fp64 (reward None: max(1, |q64|))."""
    c = lambda v: np.asarray(v, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        if reward is None:
            return np.maximum(1.0, np.abs(q64))
        return np.maximum(1.0, np.maximum(np.abs(c(reward)), np.abs(c(discount) * (1 - c(terminated)) * q64)))


def pinned_gate(v64, v32, scale):
    """mc.edge_gate with the floor on the largest TERM: reward ~ -discount q cancels, and the reference's fp32 loses the same digits."""
    return np.maximum(PIN_FLOOR * scale, 2.0 * np.abs(np.asarray(v32, np.float64) - v64))


def chain_gate(o64, o32, scale):
    return np.maximum(CHAIN_FLOOR * scale, 2.0 * np.abs(np.asarray(o32, np.float64) - o64))


def pinned_expect(cfg, target, pair, reduce, reward=None, terminated=None, discount=None):
    """(v64, v32, gate) of a call on pinned heads: heads `pair` of the online / target ensemble."""
    q64, q32 = head_values(cfg, np.float64)[int(target)], head_values(cfg, np.float32)[int(target)]
    a, b = pair
    v64 = td_from(q64[a], q64[b], reward, terminated, discount, reduce, np.float64)
    v32 = td_from(q32[a], q32[b], reward, terminated, discount, reduce, np.float32)
    scale = term_scale(reduce_of(q64[a], q64[b], reduce), reward, terminated, discount)
    if reward is not None:
        v64, v32, scale = (np.broadcast_to(x, np.shape(reward)) for x in (v64, v32, scale))
    with np.errstate(all="ignore"):
        return v64, v32, pinned_gate(v64, v32, scale)


def separation(cfg):
    """Worst (smallest) |difference| / (100 x the larger pinned gate) over the pairs of unordered-pair means, per ensemble, and
    whether the num_q values are pairwise different: ((ratio online, ratio target), distinct)."""
    ratios, distinct = [], True
    for target in (False, True):
        q64 = head_values(cfg, np.float64)[int(target)]
        distinct &= len(set(q64.tolist())) == len(q64)
        means = [pinned_expect(cfg, target, p, "avg") for p in itertools.combinations(range(cfg.num_q), 2)]
        worst = np.inf
        for (a, _, ga), (b, _, gb) in itertools.combinations(means, 2):
            worst = min(worst, abs(a - b) / (100.0 * max(ga, gb)))
        ratios.append(worst)
    return tuple(ratios), distinct


# ---------------------------------------------------------------- inputs
def row_inputs(rows, big=False):
    """reward distinct per row (a seeded normal, times 1e3 with `big`), terminated cycling through TERM_CYCLE."""
    reward = np.random.default_rng(77).standard_normal(rows).astype(np.float32) * np.float32(1e3 if big else 1.0)
    assert len(set(reward.tolist())) == rows
    return reward, np.resize(np.array(TERM_CYCLE, np.float32), rows)


TAIL_REWARDS = (0.0, -0.0, 1e-8, -1e-8, 1.0, -2.5, 1e6, -1e6, 3e38, "cancel")   # "cancel": reward = -discount q32
TAIL_TERMINATED = (0.0, 1.0, 0.3, 1.0 - 2.0 ** -24, 2.0)
TAIL_DISCOUNTS = (0.0, 0.99, 1.0, 0.5)


def tail_table(q32):
    """Every (reward, terminated, discount) of the tail edges for a reduce value q32 (fp32 scalar): three fp32 arrays [200]."""
    r, t, d = [], [], []
    for disc in TAIL_DISCOUNTS:
        for rew in TAIL_REWARDS:
            for term in TAIL_TERMINATED:
                r.append(-np.float32(disc) * np.float32(q32) if rew == "cancel" else np.float32(rew))
                t.append(term)
                d.append(disc)
    return np.array(r, np.float32), np.array(t, np.float32), np.array(d, np.float32)


def distinct_discounts(n_tasks):
    """A different discount for every task (the cases' own tables hold two values)."""
    return (np.float32(0.90) + np.float32(0.01) * np.arange(n_tasks, dtype=np.float32)).astype(np.float32)


TASK_PATTERNS = ("all0", "alllast", "mod", "mod7", "blocks64", "lastonly")


def task_pattern(kind, rows, n):
    r = np.arange(rows)
    t = {"all0": np.zeros(rows), "alllast": np.full(rows, n - 1), "mod": r % n, "mod7": (7 * r) % n,
         "blocks64": (r // 64 + 1) % n, "lastonly": np.where(r == rows - 1, n - 1, 0)}[kind]
    return t.astype(np.int32)


def chain_eps(rows, A):
    """pi_eps: a seeded normal, rows 0..3 overwritten with 0, +5, -5 and a mixed-sign +-5 row (saturated tanh, actions at +-1)."""
    eps = np.random.default_rng(100 + rows).standard_normal((rows, A)).astype(np.float32)
    special = [np.zeros(A), np.full(A, 5.0), np.full(A, -5.0), np.where(np.arange(A) % 2 == 0, 5.0, -5.0)]
    for i, s in enumerate(special[:rows]):
        eps[i] = s
    return eps


# ---------------------------------------------------------------- the fp32 / fp64 oracle on the case's own weights
def oracle_chain(cfg, sd, z, eps, task):
    """dtype -> (action [R, A], q [2 (online, target), num_q, R]) from oracle.planner_oracle: OracleModel.pi, then every head of both
    ensembles the way OracleModel.Q_pair evaluates them (ensemble_forward, two_hot_inv); numpy fp64 arrays of both evaluations."""
    import torch
    from oracle import planner_oracle as po

    out = {}
    tk = None if task is None else torch.as_tensor(np.asarray(task, np.int64))
    for dt in (torch.float32, torch.float64):
        m = po.OracleModel(cfg, {k: torch.as_tensor(v) for k, v in sd.items()}, dtype=dt)
        z2 = torch.as_tensor(z).to(dt)
        a = m.pi(z2, tk, torch.as_tensor(eps).to(dt))
        x = torch.cat([m.task_emb(z2, tk) if cfg.multitask else z2, a], -1)
        q = [po.two_hot_inv(po.ensemble_forward(m.sd, p, x), cfg)[..., 0] for p in ("_Qs.params", "_target_Qs_params")]
        out[dt] = (a.numpy().astype(np.float64), torch.stack(q).numpy().astype(np.float64))
    return out[torch.float32], out[torch.float64]


def chain_expect(o32, o64, target, pair, reduce, reward=None, terminated=None, discount=None):
    """(v64, gate) of a call on the case's own weights from oracle_chain's two evaluations.  The fp32 oracle value is its fp32 Q
    through the tail in fp32 (torch and numpy agree bit for bit on it: tests/test_value_edges.py)."""
    a, b = pair
    q32, q64 = o32[1][int(target)], o64[1][int(target)]
    c = lambda v: None if v is None else np.asarray(v, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        r64 = reduce_of(q64[a], q64[b], reduce)   # (the fp64 oracle's Q is no fp32 number: td_from's cast does not apply)
        v64 = r64 if reward is None else c(reward) + c(discount) * (1 - c(terminated)) * r64
    v32 = td_from(q32[a].astype(np.float32), q32[b].astype(np.float32), reward, terminated, discount, reduce, np.float32)
    return v64, chain_gate(v64, v32, term_scale(r64, reward, terminated, discount))
