"""CPU: the edge inputs of tests/test_gpu_model_edges.py (tests/model_common.py: edge_targets, edge_logit_rows, TERM_XS / TERM_YS)
before any kernel sees them.  The numpy restatement the GPU file gates against equals the reference's own soft_ce / two_hot_inv /
binary_cross_entropy_with_logits in fp64 to 1e-12 on every one of them, and the gate admits the reference: its fp32 result lies
inside max(1e-5 max(1, |v|), 2 |restatement fp32 - restatement fp64|) on every input.  An input at which the reference alone
left the gate would be listed in model_common.EDGE_REMOVED with its measured value, not gated more loosely; none is (worst
reference err / gate measured here: 0.53, row "off+300" at the target below symexp(9.8))."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import model_common as mc

CFG = SimpleNamespace(num_bins=101, vmin=-10.0, vmax=10.0, bin_size=20.0 / 100)


def _rows_and_targets():
    t = mc.edge_targets(CFG)
    return [(name, np.repeat(r[None], len(t), 0), t) for name, r in mc.edge_logit_rows(CFG).items()]


def test_edge_table_is_what_the_issue_lists():
    t, rows = mc.edge_targets(CFG), mc.edge_logit_rows(CFG)
    assert t.dtype == np.float32 and len(t) == 48 and len(t) % 8 == 0
    top = np.float32(mc.symexp(10.0))
    for v in (0.0, 1e-8, 1e-30, 22025.4, 22026.5, 22027.0, 1e6, 3e38, np.inf, top, np.nextafter(top, np.float32(0))):
        assert np.float32(v) in t and np.float32(-v) in t, v
    assert np.signbit(t[1]) and not np.signbit(t[0])   # -0 and +0 are both there
    assert len({x.tobytes() for x in t}) == 47          # distinct bit patterns (symexp(0) = 0 comes twice: as +0 and as k = 50)
    assert all(r.dtype == np.float32 and r.shape == (101,) and np.isfinite(r).all() for r in rows.values())
    assert np.argmax(rows["twomax"]) == 40 and rows["twomax"][40] == rows["twomax"][41]
    assert not mc.EDGE_REMOVED and len(mc.edge_pairs(CFG)) == 14 * 48
    # clamp, last bin and wrap are reached: the restatement's own index / weight at the top and bottom targets
    x = np.clip(mc.symlog(t.astype(np.float64)), CFG.vmin, CFG.vmax)
    u = (x - CFG.vmin) / CFG.bin_size
    assert (u == 100).sum() >= 5 and (u == 0).sum() >= 5 and ((u > 99) & (u < 100)).any() and ((u > 0) & (u < 1)).any()


def test_restatement_equals_the_reference_in_fp64_on_every_edge_input():
    from oracle import ref_runner

    if not ref_runner.available():
        pytest.skip("reference tree not present")
    import torch
    import torch.nn.functional as F
    ref_runner._import_reference()
    from common import math as rmath

    for name, lg, t in _rows_and_targets():
        lg64, t64 = lg.astype(np.float64), t.astype(np.float64)
        want = rmath.soft_ce(torch.as_tensor(lg64), torch.as_tensor(t64)[:, None], CFG)[:, 0].numpy()
        got = mc.soft_ce_rows(lg64, t64, CFG)
        assert (np.abs(got - want) <= 1e-12 * np.maximum(1, np.abs(want))).all(), name
        wq = rmath.two_hot_inv(torch.as_tensor(lg64[:1]), CFG)[0, 0].item()
        assert abs(mc.two_hot_inv_rows(lg64[0], CFG) - wq) <= 1e-12 * max(1, abs(wq)), name
    x = np.repeat(np.array(mc.TERM_XS, np.float32).astype(np.float64), len(mc.TERM_YS))
    y = np.tile(np.array(mc.TERM_YS, np.float32).astype(np.float64), len(mc.TERM_XS))
    wb = F.binary_cross_entropy_with_logits(torch.as_tensor(x), torch.as_tensor(y), reduction="none").numpy()
    assert (np.abs(mc.bce_logits(x, y) - wb) <= 1e-12 * np.maximum(1, np.abs(wb))).all()


def test_gate_admits_the_reference_fp32_on_every_edge_input():
    """The admission condition: whatever the gate asks of the library, the reference's own fp32 meets."""
    from oracle import ref_runner

    if not ref_runner.available():
        pytest.skip("reference tree not present")
    import torch
    import torch.nn.functional as F
    ref_runner._import_reference()
    from common import math as rmath

    pairs = set(mc.edge_pairs(CFG))
    worst = (0.0, None)
    for name, lg, t in _rows_and_targets():
        with np.errstate(all="ignore"):
            v64 = mc.soft_ce_rows(lg.astype(np.float64), t.astype(np.float64), CFG)
            v32 = mc.soft_ce_rows(lg, t, CFG)
        assert v32.dtype == np.float32 and np.isfinite(v64).all()
        r32 = rmath.soft_ce(torch.as_tensor(lg), torch.as_tensor(t)[:, None], CFG)[:, 0].numpy()
        ratio = np.abs(r32 - v64) / mc.edge_gate(v64, v32)
        q64, q32 = mc.two_hot_inv_rows(lg[0].astype(np.float64), CFG), mc.two_hot_inv_rows(lg[0], CFG)
        rq = rmath.two_hot_inv(torch.as_tensor(lg[:1]), CFG)[0, 0].item()
        qr = abs(rq - q64) / mc.edge_gate(q64, q32)
        rel = lambda v: (np.abs(v - v64) / np.maximum(1, np.abs(v64))).max()
        print(f"[{name}] reference fp32: soft_ce worst err / gate {ratio.max():.3f} (target {t[ratio.argmax()]!r}), two_hot_inv {qr:.3f}; "
              f"worst relative error {rel(r32):.2e}, of the fp32 restatement {rel(v32):.2e}")
        if name == mc.UNGATED_ROW:
            continue
        for i in range(len(t)):
            if (name, i) in pairs:
                assert ratio[i] <= 1, (name, i, t[i], ratio[i])
                worst = max(worst, (float(ratio[i]), (name, i)))
        assert qr <= 1, name
    print("worst admitted:", worst)
    x = np.repeat(np.array(mc.TERM_XS, np.float32), len(mc.TERM_YS))
    y = np.tile(np.array(mc.TERM_YS, np.float32), len(mc.TERM_XS))
    v64, v32 = mc.bce_logits(x.astype(np.float64), y.astype(np.float64)), mc.bce_logits(x, y)
    r32 = F.binary_cross_entropy_with_logits(torch.as_tensor(x), torch.as_tensor(y), reduction="none").numpy()
    assert (np.abs(r32 - v64) <= mc.edge_gate(v64, v32)).all()


def test_pin_heads_gives_the_oracle_the_pinned_logits():
    """pin_heads through the project's fp64 oracle model: every row's logits are the bias, bit for bit, and the fresh model of
    the reference (world_model.py:32: zero last layers) gives log(101) on every soft-CE row."""
    import torch
    from oracle import cases
    from oracle import planner_oracle as po

    c = cases.build_case("small_ep_fire")
    cfg = c["cfg"]
    nb = cfg.num_bins
    rr = np.arange(nb, dtype=np.float32)
    qr = np.stack([(i + 1) * 1000 + rr for i in range(cfg.num_q)])
    sd = mc.pin_heads(c["sd"], cfg, rr, qr, 7.25)
    assert sd["_Qs.params.2.bias"].shape == torch.as_tensor(c["sd"]["_Qs.params.2.bias"]).shape
    assert not sd["_reward.2.weight"].any() and not sd["_Qs.params.2.weight"].any() and not sd["_target_Qs_params.2.weight"].any()
    assert np.array_equal(np.asarray(c["sd"]["_reward.2.bias"]), np.asarray(cases.build_case("small_ep_fire")["sd"]["_reward.2.bias"]))  # a copy
    model = po.OracleModel(cfg, sd)
    inp = mc.inputs(cfg, 4)
    z, a = torch.as_tensor(inp["z0"]), torch.as_tensor(inp["actions"][0])
    assert torch.equal(model.reward(z, a, None), torch.as_tensor(rr).expand(4, nb))
    for prefix in ("_Qs.params", "_target_Qs_params"):
        assert torch.equal(po.ensemble_forward(model.sd, prefix, torch.cat([z, a], -1)), torch.as_tensor(qr)[:, None].expand(-1, 4, -1))
    assert torch.equal(po.mlp_forward(model.sd, "_termination", z), torch.full((4, 1), 7.25))
    fresh = mc.pin_heads(c["sd"], cfg, np.zeros(nb), np.zeros((cfg.num_q, nb)))
    assert not fresh["_reward.2.bias"].any() and not fresh["_Qs.params.2.bias"].any()
    t = mc.edge_targets(cfg).astype(np.float64)
    got = mc.soft_ce_rows(np.zeros((len(t), nb)), t, cfg)
    assert np.abs(got - np.log(101)).max() <= 1e-12
