"""Shared by tools/make_update_golden.py (generator), tests/test_update_golden.py (CPU) and tests/test_gpu_update.py (-m gpu): the
case table of tests/golden/update_steps.npz, its seeded inputs, its key layout and the two gates.  Nothing here comes from a HIP
result, and nothing here reads the reference tree.

The fixture is K iterations of the reference's own `TDMPC2._update` on one batch per case (oracle/ref_runner.py:
run_reference_updates), in fp64 and in fp32, plus one fp64 run per deliberately wrong control.  Keys, per case id `c`:
  c.obs [H+1, B, od], c.action [H, B, A], c.reward [H, B, 1], c.terminated [H, B, 1] (episodic), c.task [B] (multitask)     fp32 / int64
  c.td_pi_eps [K, H, B, A], c.td_qidx [K, 2], c.pi_eps [K, H+1, B, A], c.qidx [K, 2]                                        fp32 / int32
  c.info64, c.info32 [K, len(info_keys)]    the info dicts of the verbatim fp64 / fp32 run (fp64 arrays; columns: info_keys(cfg))
  c.td64 [K, H, B, 1] fp64, c.td32 [K, H, B, 1] fp32    `_update`'s own td_targets
  c.term_logit64 [K, B, 1]                  termination_pred[-1] of the fp64 run (episodic)
  c.<control>.info64, c.<control>.td64      the fp64 run of a control
and `scale0`, the running scale every run starts from."""
import os

import numpy as np

from tests import optim_common as oc
from tests import value_common as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "update_steps.npz")
SIZE_CAP = 400 * 1024
MARGIN, FLOOR = oc.MARGIN, oc.FLOOR  # e <= MARGIN * max(e_ref32, FLOOR)
K = 4
SCALE0 = 7.5
SEED = 4200
SENSITIVITY = 10.0  # every control moves some gated key of some case by this many bounds

# id: the model of oracle/cases.py, config overrides, B, the factor on the output layers of `_Qs` and of the target copy
CASES = {
    "tiny-B33": dict(model="tiny", over={}, B=33, q_scale=None),            # odd batch, more than one 32-row block
    "tiny_mt-B12": dict(model="tiny_mt", over={}, B=12, q_scale=None),      # task-embedding group and its remainder, masks, discounts
    "small_ep-B9": dict(model="small_ep_fire", over={}, B=9, q_scale=None),  # termination loss, (1 - terminated), rate / f1
    "tiny_wideq-B12": dict(model="tiny", over={}, B=12, q_scale=4.0),       # RunningScale's percentile path: p95 - p5 of q[0] > 1
    "tiny-H1-B1": dict(model="tiny", over=dict(horizon=1), B=1, q_scale=None),  # one step, one row
}
CONTROLS = ("enc_lr", "pi_eps", "no_emb_leak", "no_soft_update", "soft_update_first", "stale_pi_td", "soft_update_before_step")
LOSS_KEYS = ("consistency_loss", "reward_loss", "value_loss", "termination_loss", "total_loss", "grad_norm")
STAT_KEYS = ("termination_rate", "termination_f1")  # discrete: compared for equality
PI_KEYS = ("pi_loss", "pi_grad_norm", "pi_entropy", "pi_scaled_entropy", "pi_scale")
PIN_KEYS = ("td_pi_eps", "td_qidx", "pi_eps", "qidx")


def info_keys(cfg):
    """The keys of `_update`'s info dict in the reference's order (tdmpc2.py:320-330)."""
    return LOSS_KEYS + (STAT_KEYS if cfg.episodic else ()) + PI_KEYS


def controls_of(cfg):
    return tuple(c for c in CONTROLS if c != "no_emb_leak" or cfg.multitask)


def build(case_id):
    """(cfg, state dict of numpy arrays) of a case: the model of oracle/cases.py with dropout 0 and batch_size B, as
    tests/test_gpu_pi_grad.py: _agent makes it."""
    from oracle import cases
    from tdmpc2_amd.config import named_config

    spec = CASES[case_id]
    name = spec["model"]
    cfg_name, overrides, E, eval_mode, head_std = cases.CASES[name]
    c = cases.build_custom(named_config(cfg_name, **overrides, **spec["over"]), E, eval_mode, head_std, name=name)
    cfg = c["cfg"].replace(batch_size=spec["B"], buffer_size=200, dropout=0.0)
    sd = {k: np.asarray(v) for k, v in c["sd"].items()}
    if spec["q_scale"] is not None:
        for k in list(sd):
            if k.startswith(("_Qs.params.2.", "_target_Qs_params.2.", "_detach_Qs_params.2.")):
                sd[k] = (sd[k] * np.float32(spec["q_scale"])).astype(np.float32)
    return cfg, sd


def inputs(case_id, cfg):
    """The batch and the pins of a case from numpy.random.default_rng: obs ~ N(0, 1), action ~ U(-1, 1), reward ~ N(0, 1),
    terminated ~ Bernoulli(0.2) (episodic), task = arange(B) % n_tasks (multitask); per iteration two noise tensors and two ordered
    pairs of different Q heads, the pairs cycling so that they differ between iterations, one has its first index above its second and
    one uses num_q - 1."""
    rng = np.random.default_rng(SEED + list(CASES).index(case_id))
    H, B, A, od, nq = cfg.horizon, CASES[case_id]["B"], cfg.action_dim, cfg.obs_shape["state"][0], cfg.num_q
    batch = {"obs": rng.standard_normal((H + 1, B, od)).astype(np.float32),
             "action": rng.uniform(-1, 1, (H, B, A)).astype(np.float32),
             "reward": rng.standard_normal((H, B, 1)).astype(np.float32)}
    if cfg.episodic:
        batch["terminated"] = (rng.random((H, B, 1)) < 0.2).astype(np.float32)
    if cfg.multitask:
        batch["task"] = (np.arange(B) % len(cfg.tasks)).astype(np.int64)
    pairs = [(a, b) for a in range(nq) for b in range(nq) if a != b]
    td_pairs = [pairs[(1, 3, 5, 2, 0, 4)[k % 6] % len(pairs)] for k in range(K)]  # num_q 3: (0, 2), (1, 2), (2, 1), (1, 0)
    pi_pairs = [pairs[(5, 4, 3, 0, 2, 1)[k % 6] % len(pairs)] for k in range(K)]  # num_q 3: (2, 1), (2, 0), (1, 2), (0, 1)
    pins = {"td_pi_eps": rng.standard_normal((K, H, B, A)).astype(np.float32), "td_qidx": np.asarray(td_pairs, np.int32),
            "pi_eps": rng.standard_normal((K, H + 1, B, A)).astype(np.float32), "qidx": np.asarray(pi_pairs, np.int32)}
    return batch, pins


def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def batch_of(g, case_id):
    return {k: g.get(f"{case_id}.{k}") for k in ("obs", "action", "reward", "terminated", "task")}


def pins_of(g, case_id):
    return {k: g[f"{case_id}.{k}"] for k in PIN_KEYS}


# ---------------------------------------------------------------- the gates
def info_bounds(g, case_id, keys):
    """{key: bound on |x - ref64| / |ref64|} = MARGIN * max(max over the K iterations of the verbatim fp32 run's own error, FLOOR);
    None for a key that is compared for equality: the discrete termination statistics and a key whose fp64 value is 0 throughout."""
    i64, i32 = g[f"{case_id}.info64"], g[f"{case_id}.info32"]
    out = {}
    for j, k in enumerate(keys):
        if k in STAT_KEYS or not i64[:, j].any():
            out[k] = None
            continue
        out[k] = MARGIN * max(float((np.abs(i32[:, j] - i64[:, j]) / np.abs(i64[:, j])).max()), FLOOR)
    return out


def td_gate(g, case_id):
    """value_common.chain_gate per element of the TD target [K, H, B, 1]: max(1e-4 max(1, |reward|, |discount (1 - terminated) q64|),
    2 |ref32 - ref64|) -- the second term of the target is td64 - reward."""
    td64, td32 = g[f"{case_id}.td64"], g[f"{case_id}.td32"]
    reward = g[f"{case_id}.reward"].astype(np.float64)[None]
    scale = np.maximum(1.0, np.maximum(np.abs(reward), np.abs(td64 - reward)))
    return vc.chain_gate(td64, td32, scale)


def info_ratios(got, g, case_id, keys):
    """got [K, len(keys)] against the fp64 run -> ({key: worst e / max(e_ref32, FLOOR)}, failures).  Gate: ratio <= MARGIN;
    equality keys: |got - ref64| <= 1e-6."""
    i64 = g[f"{case_id}.info64"]
    bounds = info_bounds(g, case_id, keys)
    worst, fails = {}, []
    for j, k in enumerate(keys):
        for it in range(got.shape[0]):
            x, r = float(got[it, j]), float(i64[it, j])
            if bounds[k] is None:
                if not abs(x - r) <= 1e-6:
                    fails.append((it, k, x, r))
                continue
            e = abs(x - r) / abs(r)
            worst[k] = max(worst.get(k, 0.0), e / (bounds[k] / MARGIN))
            if not e <= bounds[k]:
                fails.append((it, k, x, r, e, bounds[k]))
    return worst, fails


def control_margin(g, case_id, control, keys):
    """How far a control's fp64 run lies from the verbatim fp64 run, in bounds: (worst ratio, where).  `stale_pi_td` is measured on
    the TD target with the TD gate, every other control on the info keys."""
    if control == "stale_pi_td":
        r = np.abs(g[f"{case_id}.{control}.td64"] - g[f"{case_id}.td64"]) / td_gate(g, case_id)
        return float(r.max()), "td_targets"
    i64, c64 = g[f"{case_id}.info64"], g[f"{case_id}.{control}.info64"]
    bounds = info_bounds(g, case_id, keys)
    best, where = 0.0, None
    for j, k in enumerate(keys):
        if bounds[k] is None:
            continue
        r = float((np.abs(c64[:, j] - i64[:, j]) / np.abs(i64[:, j])).max()) / bounds[k]
        if r > best:
            best, where = r, k
    return best, where
