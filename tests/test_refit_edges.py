"""CPU: the harness of tests/test_gpu_refit_edges.py proved before the kernel meets it (tests/refit_common.py).  The fp64
reference equals oracle.planner_oracle.refit run in fp64 wherever torch's top-k order is the contract's; the oracle's own fp32
stays inside every gate on every tie-free case; on the tie cases torch.topk's order is stated and sets are compared; the port of
the kernel's branch decisions puts every geometry where its test needs it; the crafted picks keep their distance; and nine
mistakes made IN THE REFERENCE each leave a gate by a wide factor.
TDMPC2_REFIT_EDGES_JSON=<file>: the figures are merged into that file (profiles/refit_edges.json)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import refit_common as rc

MUTATION_FACTOR = 10.0


def record(section, worst):
    """Merge {item: figure} into the JSON file TDMPC2_REFIT_EDGES_JSON names (no-op without it)."""
    path = os.environ.get("TDMPC2_REFIT_EDGES_JSON")
    if not path:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc["gate"] = ("value, elite_idx, prev_mean: bit-exact;  score: 2 (2 u |arg| + 2 expf_ulp 2^-23 + the same averaged over S + (K + 2) u) "
                   "relative + FLT_MIN;  mean: 2 (u (2 K + 4) sum |s a| + sum ds |a - m|);  std: inside "
                   "[clamp sqrt(s2 - g), clamp sqrt(s2 + g)] widened by 2^-23, times the mask;  action: 2^-23 (|a| + |std0 eps|);  "
                   "u = 2^-24  (tests/refit_common.py)")

    def clean(v):
        if isinstance(v, dict):
            return {k: clean(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [clean(x) for x in v]
        return v if isinstance(v, (bool, str)) else min(float(v), 1e30)

    doc.setdefault(section, {}).update({k: clean(v) for k, v in worst.items()})
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)


CFG = SimpleNamespace(num_elites=0, **rc.CFG)
# the geometries the CPU harness walks: every sort width, every K class, the three action shapes (the full grid runs on the GPU)
GEOMS = [(64, 1, 1, 1), (64, 64, 3, 6), (192, 3, 3, 6), (192, 61, 5, 61), (512, 64, 3, 6), (512, 61, 1, 1), (1024, 64, 5, 61),
         (1024, 1024, 3, 6), (512, 3, 3, 17)]


def _oracle(value, actions, K, dtype, mask=None):
    from oracle import planner_oracle as po

    cfg = SimpleNamespace(**{**vars(CFG), "num_elites": K})
    if dtype == torch.float64:  # the config's scalars as the fp32 bits the kernel is given
        cfg.temperature, cfg.min_std, cfg.max_std = (float(np.float32(x)) for x in (cfg.temperature, cfg.min_std, cfg.max_std))
        value = rc.nan_to_num(value)  # (in fp64 torch's nan_to_num would map inf to DBL_MAX; the fp32 run below does its own)
    v = torch.as_tensor(value).to(dtype).unsqueeze(1)
    m = None if mask is None else torch.as_tensor(mask).to(dtype).unsqueeze(0)
    v, idx, score, _, mean, std = po.refit(cfg, v, torch.as_tensor(actions).to(dtype), m)
    return dict(value=v.squeeze(1).numpy(), elite_idx=idx.numpy(), score=score.squeeze(1).numpy(), mean=mean.numpy(), std=std.numpy())


def _mask(A, seed=0):
    m = np.ones(A, np.float32)
    m[np.random.default_rng(seed).choice(A, max(A // 3, 1), replace=False)] = 0.0
    return m


def test_branch_port_puts_the_geometries_where_the_tests_need_them():
    assert [rc.sort_width(n) for n in rc.GEOMETRY_N] == [64, 256, 512, 1024]
    assert rc.refit_lds_bytes(512, 64, 3, 6) == ((1024 + 192 + 72 + 48) * 4 + 64 + 64 * 18 * 4, True)
    # H A = 5 x 61 at K = 64: 78 080 B of elite actions, unstaged in k_refit (48 KiB) and too large for the 32-row tile as well
    assert rc.branches(1024, 64, 5, 61) == dict(sorted=True, staged=False, in_launch=False)
    assert rc.branches(1024, 64, 5, 61, in_launch=True) == dict(sorted=True, staged=False, in_launch=False)
    assert rc.branches(512, 61, 5, 61)["staged"] is False and rc.branches(512, 3, 5, 61)["staged"] is True
    # the counting path: the sort width beyond the rollout kernels' 512 threads, in-launch only
    assert rc.branches(1024, 64, 3, 6, in_launch=True) == dict(sorted=False, staged=True, in_launch=True)
    assert rc.branches(512, 64, 3, 6, in_launch=True) == dict(sorted=True, staged=True, in_launch=True)
    assert rc.branches(1024, 1024, 3, 6)["staged"] is False and rc.branches(1024, 1024, 1, 1)["staged"] is True
    assert rc.fold_budget(6) == 32 * 2128 and rc.fold_budget(38) == 32 * (4 * 560 + 16)


def test_reference_equals_the_oracle_in_fp64():
    for N, K, H, A in GEOMS:
        names, vals, acts = rc.plans_of(N, K, H, A)
        mask = _mask(A) if A == 17 else None
        for name, v, a in zip(names, vals, acts):
            if name.split("/")[0] in rc.TIE_PATTERNS:
                continue
            ref = rc.refit_ref(v, a, K, mask=mask, **rc.CFG)
            o = _oracle(v, a, K, torch.float64, mask)
            assert np.array_equal(o["elite_idx"], ref["elite_idx"]), (N, K, name)
            assert np.array_equal(o["value"].astype(np.float32), ref["value"]), (N, K, name)
            for k in ("score", "mean", "std"):
                assert np.abs(o[k] - ref[k]).max() <= 1e-12 * max(1.0, np.abs(ref[k]).max()), (N, K, name, k)


def test_oracle_fp32_stays_inside_every_gate_on_tie_free_cases():
    worst = {}
    for N, K, H, A in GEOMS:
        names, vals, acts = rc.plans_of(N, K, H, A)
        mask = _mask(A) if A == 17 else None
        for name, v, a in zip(names, vals, acts):
            if name.split("/")[0] in rc.TIE_PATTERNS:
                continue
            ch = rc.check(rc.refit_ref(v, a, K, mask=mask, **rc.CFG), _oracle(v, a, K, torch.float32, mask))
            worst[f"N{N} K{K} H{H} A{A} {name}"] = rc.worst(ch)
    top = max(worst, key=worst.get)
    print("oracle fp32, worst err / gate:", worst[top], top)
    record("cpu_oracle_fp32", {"worst": worst[top], "worst_case": top, "cases": len(worst)})
    assert worst[top] <= 0.5, (top, worst[top])  # well under 1


def test_what_torch_topk_returns_on_ties():
    """torch.topk leaves the order among equal values open (its CPU kernel is a partial sort).  Where it happens to return the
    contract's order everything is compared; else the SET where the tied values all fit among the elites, and in every case the
    elite VALUES.  The kernel is held to the contract, not to torch."""
    stated = {"contract order": 0, "same set, other order": 0, "other set": 0}
    for N, K, H, A in GEOMS:
        names, vals, acts = rc.plans_of(N, K, H, A)
        for name, v, a in zip(names, vals, acts):
            if name.split("/")[0] not in rc.TIE_PATTERNS:
                continue
            ref = rc.refit_ref(v, a, K, **rc.CFG)
            o = _oracle(v, a, K, torch.float32)
            assert np.array_equal(np.sort(ref["value"][o["elite_idx"]])[::-1], ref["value"][ref["elite_idx"]]), (N, K, name)
            if np.array_equal(o["elite_idx"], ref["elite_idx"]):
                stated["contract order"] += 1
                assert rc.worst(rc.check(ref, o)) <= 0.5, (N, K, name)
            elif set(o["elite_idx"].tolist()) == set(ref["elite_idx"].tolist()):
                stated["same set, other order"] += 1
                ch = rc.check(ref, dict(o, elite_idx=ref["elite_idx"], score=np.sort(o["score"])[::-1]))
                assert max(ch["mean"], ch["std"]) <= 0.5, (N, K, name, ch)  # equal scores within a tie: the sums do not care
            else:
                stated["other set"] += 1
    print("torch.topk on the tie cases:", stated)
    record("cpu_torch_topk_on_ties", stated)
    assert sum(stated.values()) > 0


def _pick_geoms():
    return [(64, 3, 6), (61, 3, 6), (1, 3, 6), (64, 1, 1)]


def test_crafted_picks_keep_their_distance():
    least = np.inf
    for K, H, A in _pick_geoms():
        N = 512
        acts = rc.action_pattern("random", H, N, A, np.random.default_rng(K))
        for name, c in rc.pick_cases(K, H, N, A).items():
            assert (c["gumbel_exp"] > 0).all()
            ref = rc.refit_ref(c["value"], acts, K, gumbel_exp=c["gumbel_exp"], final_eps=c["final_eps"], last=True, **rc.CFG)
            if ref["pick_tied"]:
                assert name == "all_tied" and ref["pick"] == 0 and ref["elite_idx"][0] == 0
                continue
            assert name != "all_tied" or K == 1
            least = min(least, ref["pick_margin"] / max(ref["pick_gate"], 1e-300))
            assert ref["pick_margin"] >= 100.0 * ref["pick_gate"], (K, name, ref["pick_margin"], ref["pick_gate"])
            if name == "underflow" and K > 3:
                assert ref["pick"] < 3 and (ref["score"][3:] < 2.0 ** -160).all()
            if name == "eps_past_one":
                want, _, _, _ = rc.action_of(ref, ref["std"][0])
                assert (np.abs(want) == 1.0).all()
    print("least pick margin / gate:", least)
    record("cpu_pick", {"least_margin_over_gate": least})


def _mutation_case(mut):
    """(kwargs of refit_ref) on which the mistake shows."""
    rng = np.random.default_rng(11)
    N, K, H, A = 192, 61, 3, 6
    acts = rc.action_pattern("random", H, N, A, rng)
    kw = dict(value=rc.value_pattern("normal", N, K, rng), actions=acts, K=K)
    if mut == "tie_reversed":
        kw["value"] = rc.value_pattern("tie_block", N, K, rng)
    elif mut == "negzero_below":
        kw["value"] = rc.value_pattern("zero_mix", N, K, rng)
    elif mut == "inf_kept":
        kw["value"] = rc.value_pattern("inf", N, K, rng)
    elif mut == "padding_eligible":
        kw["Nvalid"] = 150
        kw["value"][150:] = 50.0  # whatever the padding rows evaluated to
    elif mut == "clamp_after_mask":
        kw["mask"] = _mask(A)
    elif mut == "pick_from_step_1":
        kw.update(gumbel_exp=rng.exponential(size=K).astype(np.float32) + 1e-3, final_eps=rng.standard_normal(A).astype(np.float32), last=True)
    return kw


def test_mutations_of_the_reference_leave_their_gates():
    out = {}
    for mut in rc.MUTATIONS:
        kw = _mutation_case(mut)
        ref = rc.refit_ref(**kw, **rc.CFG)
        assert rc.worst(rc.check(ref, rc.as_got(ref))) <= 0.5  # the reference rounded to fp32 is inside its own gates
        ch = rc.check(ref, rc.as_got(rc.refit_ref(**kw, **rc.CFG, mut=mut)))
        out[mut] = rc.worst(ch)
    print({k: (round(v, 1) if np.isfinite(v) else v) for k, v in out.items()})
    record("cpu_reference_mutations_err_over_gate", out)
    weak = {k: v for k, v in out.items() if v < MUTATION_FACTOR}
    assert not weak, weak
