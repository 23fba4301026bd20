"""CPU: the split arithmetic's scale records and packed bytes, restated (tests/scale_common.py) and held against what the suite
already pins; and the staggered checkpoints of tests/test_gpu_scale_edges.py, shown to tell the records apart.

a. The recorded digests of tests/golden/packed_digests.json (minted from the library) are re-derived in numpy for every row and for
   the weight sets plain, perturbed, zero_last, ln_gain and kw_clamps; `nonfinite` is left to the GPU test (NaN payloads).
b. What the bytes mean: |hi + lo - W 2^kw| <= max(2^-22 |W 2^kw|, 2^-25) for finite elements below the f16 maximum (hi rounds to 11
   bits: |v - hi| <= 2^-11 |v|, exact in fp32; lo rounds that residual to 11 bits, 2^-11 of it, or to the f16 subnormal grid of
   2^-24, half a step), padding exactly zero, max|W| 2^kw in [2^13, 2^14) unless kw is clamped, B 2^ka < 2^15.
   Beyond the kw clamp (the kw_clamps set): |W| = 1e20 gives kw = -40, and 1e20 x 2^-40 = 9.1e7 is past the f16 maximum: that
   element packs to hi = +Inf, lo = -Inf (lo = v - Inf), its decode is NaN; its neighbours of ordinary size pack to 0 or to f16
   subnormals with the bound above.  This is a limit of the split arithmetic, pinned here, not a bug to fix silently.
   At the other clamp, a matrix of 1e-30 takes kw = 40 and packs to all zeros: 1e-30 x 2^40 = 1.1e-18 is below half the smallest
   f16 subnormal.
c. Separation: on every staggered handle and entry point, every record the entry point reads is slipped by one exponent, up and
   down (the fp64 oracle with that layer's weight times 2 or 0.5, the bias untouched); the oracle must move by at least 10 gates of
   that entry point at the test's own inputs.  The minimum per handle and entry point is printed."""
import json
import os

import numpy as np
import pytest

from tests import refresh_common as rc
from tests import scale_common as sc

LABELS = ("plain", "perturbed", "zero_last", "ln_gain", "kw_clamps")
HANDLES = sc.FUSED + sc.LAYERED
_cases, _sets, _scen = {}, {}, {}


def _recorded():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", rc.PACKED_DIGESTS)) as f:
        return json.load(f)["rows"]


def _weight_sets(name):
    from oracle import cases

    if name not in _sets:
        _cases[name] = cases.build_case(name)
        _sets[name] = {label: sc.as_numpy(sd) for label, sd in sc.packed_inputs_cpu(_cases[name])}
    return _cases[name], _sets[name]


def scenario(name):
    if name not in _scen:
        _scen[name] = sc.Scenario(name)
    return _scen[name]


# ---------------------------------------------------------------- a. the recorded digests, re-derived
@pytest.mark.parametrize("name,path,prec", rc.CASES, ids=rc.IDS)
def test_recorded_digests_are_rederived(name, path, prec, request):
    rec = _recorded()[request.node.callspec.id]
    c, sets = _weight_sets(name)
    for label in LABELS:
        assert rc.digest(sets[label]) == rec[label]["input"], f"{label}: the INPUT tensors differ from the recorded ones"
    for label in LABELS:
        got = sc.owner_digests(sc.restated_segments(sets[label], c["cfg"], path, prec == 2))
        assert got == rec[label]["owners"], (label, sorted(o for o in rec[label]["owners"] if got.get(o) != rec[label]["owners"][o]))


# ---------------------------------------------------------------- b. what the bytes mean
def _check_slab(seg, rec, W, cfg, path, split, where):
    """The decode bound, exact zero padding and the range of the scaled maximum for one weight segment; returns the number of
    elements beyond the f16 maximum."""
    P, CT, KB = sc.packed_matrix(W, cfg, seg.owner, seg.layer, path, split)
    if not split:
        assert np.array_equal(sc.decode(seg, None), P.astype(np.float64)), where
        return 0
    kw = rec["kw"]
    hi, lo = sc.unfragment(np.frombuffer(seg.data, np.float16).reshape(CT, KB, 2, 64, 8), True)
    v = P.astype(np.float64) * 2.0 ** kw
    pad = np.ones(P.shape, bool)
    nz, nt, na = sc.layer_geometry(cfg, seg.owner, seg.layer, path, split)[:3]
    pad[:W.shape[0], :nz + na] = False
    assert not hi[pad].view(np.uint16).any() and not lo[pad].view(np.uint16).any(), f"{where}: padding is not zero"
    ok = np.isfinite(v) & (np.abs(v) < sc.F16_MAX)
    with np.errstate(all="ignore"):
        err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - v)
    bound = np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25)
    worst = float(np.max(err[ok] / bound[ok]))
    assert worst <= 1.0, f"{where}: |hi + lo - W 2^kw| is {worst:.3f} x max(2^-22 |W 2^kw|, 2^-25)"
    m = sc._finite_max(W)
    if m > 0 and abs(14 - sc._exponent(m)) <= sc.KW_CLAMP:
        assert 2.0 ** 13 <= float(m) * 2.0 ** kw < 2.0 ** 14, (where, float(m), kw)
    return int((~ok).sum())


@pytest.mark.parametrize("name,path,prec", rc.CASES, ids=rc.IDS)
def test_meaning_of_the_packed_bytes(name, path, prec):
    c, sets = _weight_sets(name)
    cfg, split = c["cfg"], prec == 2
    for label in LABELS:
        sd = sets[label]
        recs = sc.records(sd, cfg) if split else None
        beyond = 0
        for seg in sc.restated_segments(sd, cfg, path, split):
            if seg.kind != "weight":
                continue
            rec = recs[seg.owner][seg.member][seg.layer] if split else None
            W = sc.member(sd, seg.owner, seg.layer, "weight", seg.member)
            beyond += _check_slab(seg, rec, W, cfg, path, split, f"{label} {seg.owner} member {seg.member} layer {seg.layer}")
            if split and seg.layer < 2:   # B 2^ka < 2^15: the hi piece of a hidden activation cannot round to Inf
                g, b = (np.uint32(rec[k]).view(np.float32) for k in ("gmax", "bmax"))
                B = np.float32(np.sqrt(np.float32(W.shape[0] - 1))) * g + b
                assert float(B) * 2.0 ** rec["ka"] < 2.0 ** 15 and rec["ka"] <= sc.ACT_LOG2, (label, seg.owner, seg.member, seg.layer, float(B), rec["ka"])
        assert beyond == (1 if (split and label == "kw_clamps") else 0), (label, beyond)


@pytest.mark.parametrize("name,path,prec", [r for r in rc.CASES if r[2] == 2], ids=[i for i, r in zip(rc.IDS, rc.CASES) if r[2] == 2])
def test_beyond_the_kw_clamp(name, path, prec):
    """The kw_clamps set, element by element: see the module docstring, b."""
    c, sets = _weight_sets(name)
    cfg, sd = c["cfg"], sets["kw_clamps"]
    recs = sc.records(sd, cfg)
    segs = {(s.owner, s.member, s.layer): s for s in sc.restated_segments(sd, cfg, path, True) if s.kind == "weight"}
    # |W| = 1e20 on Q head 1, layer 0, row 2, source column 3 (a latent column: packed column 3)
    r = recs["q"][1][0]
    assert r["kw"] == -40 and 14 - sc._exponent(np.float32(1e20)) < -40
    seg = segs[("q", 1, 0)]
    hi, lo = sc.unfragment(np.frombuffer(seg.data, np.float16).reshape(*seg.shape, 2, 64, 8), True)
    assert hi[2, 3] == np.inf and lo[2, 3] == -np.inf and np.isnan(sc.decode(seg, r)[2, 3])
    others = np.ones(hi.shape, bool)
    others[2, 3] = False
    assert np.isfinite(hi[others]).all() and np.isfinite(lo[others]).all()
    assert np.abs(hi[others].astype(np.float64)).max() < 2.0 ** -14   # weights of ordinary size: zeros and f16 subnormals
    assert recs["q"][0][0]["kw"] != -40 and recs["q"][2][0]["kw"] != -40    # the other heads keep their own records
    # 1e-30 everywhere: kw = 40, every half zero
    r = recs["reward"][0][1]
    assert r["kw"] == 40 and not np.frombuffer(segs[("reward", 0, 1)].data, np.uint16).any()
    # 3e4 on pi layer 1: inside the clamp, kw = 14 - 15 = -1, the scaled maximum in [2^13, 2^14)
    assert recs["pi"][0][1]["kw"] == -1
    # the dynamics head times 1e-30: clamped to 40 as well, the scaled maximum far below 2^13, halves zero or subnormal
    r = recs["dynamics"][0][2]
    assert r["kw"] == 40 and float(np.uint32(r["maxbits"]).view(np.float32)) * 2.0 ** 40 < 2.0 ** -14


def test_decode_bound_is_attained_and_never_passed():
    """The derived bound on random values of every size the f16 halves can hold: the ratio reaches 1 and never exceeds it."""
    rng = np.random.default_rng(0)
    v = (rng.standard_normal(1 << 21) * np.exp2(rng.uniform(-30, 15.9, 1 << 21))).astype(np.float32)
    v = v[np.abs(v) < sc.F16_MAX]
    hi, lo = sc.split_planes(v, 0)
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - v.astype(np.float64))
    ratio = err / np.maximum(2.0 ** -22 * np.abs(v.astype(np.float64)), 2.0 ** -25)
    assert 0.9 < ratio.max() <= 1.0, ratio.max()


def test_fragment_order_round_trip():
    P = np.arange(64 * 48, dtype=np.float32).reshape(64, 48)
    slab = sc.split_slab(P, 2, 3, 0)
    assert slab.shape == (2, 3, 2, 64, 8)
    ct, kb, lane, e = 1, 2, 37, 5
    both = lambda hi, lo: hi.astype(np.float32) + lo.astype(np.float32)   # (3071 needs both halves)
    assert both(slab[ct, kb, 0, lane, e], slab[ct, kb, 1, lane, e]) == P[32 * ct + (lane & 31), 16 * kb + 8 * (lane >> 5) + e]
    assert np.array_equal(both(*sc.unfragment(slab, True)), P)
    f = sc.fp32_slab(P, 2, 6)
    assert f[ct, 4, lane, 3] == P[32 * ct + (lane & 31), 8 * 4 + 4 * (lane >> 5) + 3]
    assert np.array_equal(sc.unfragment(f, False), P)


# ---------------------------------------------------------------- the staggered checkpoints
@pytest.mark.parametrize("name", HANDLES)
def test_staggered_records_differ(name):
    s = scenario(name)
    recs = sc.records(s.sd, s.cfg)
    assert sc.stagger_violations(recs, s.cfg) == []
    assert sc.stagger_violations(sc.records(s.base_sd, s.cfg), s.cfg)   # ... which the fixture's own records do not meet
    for net in recs:   # no record sits on a clamp, and the restated rule follows the plan's arithmetic
        for hd, (rs, base) in enumerate(zip(recs[net], sc.records(s.base_sd, s.cfg)[net])):
            p = s.plan[(net, hd)]
            for l in range(3):
                assert abs(rs[l]["kw"]) < sc.KW_CLAMP and rs[l]["ka"] > sc.KA_FLOOR
                assert rs[l]["kw"] == base[l]["kw"] - p["s"][l] + (p["g"][l - 1] if l else 0)


def test_a_difference_is_named():
    """The report of the GPU test's byte comparison, on a restatement with one bit of one half flipped."""
    s = scenario("small_ep")
    want = sc.restated_segments(s.sd, s.cfg, 2, True)
    got = [(w.owner, w.data) for w in want]
    i = next(k for k, w in enumerate(want) if (w.owner, w.member, w.layer, w.kind) == ("q", 1, 1, "weight"))
    raw = bytearray(got[i][1])
    raw[2 * (1024 + 512 + 8 * 37 + 5)] ^= 1   # ct 0, kb 1, lo plane, lane 37, e 5
    got[i] = ("q", bytes(raw))
    msg = sc.first_difference(want, got)
    assert "owner q member 1 layer 1 kind weight" in msg and "row 5, packed column 29, lo" in msg, msg


# ---------------------------------------------------------------- c. separation
@pytest.mark.parametrize("entry", sc.ENTRY_POINTS)
@pytest.mark.parametrize("name", HANDLES)
def test_a_slipped_record_moves_the_oracle(name, entry):
    s = scenario(name)
    floor = s.fp32_ratio(entry)
    worst, where = np.inf, None
    for net, hd in s.reads(entry):
        for layer in range(3):
            for up in (True, False):
                sep = s.separation(entry, net, hd, layer, up)
                if sep < worst:
                    worst, where = sep, (net, hd, layer, "up" if up else "down")
    print(f"[{name}] {entry}: minimum separation {worst:.1f} gates at {where}; oracle fp32 error / gate floor {floor:.3f}")
    # the oracle's own fp32 error leaves the gate at its floor: 2 x it (1.5 x for the value entries) stays below the floor
    assert floor <= (1 / sc.VALUE_FACTOR if entry in ("estimate_value", "plan") else 1.0), (name, entry, floor)
    assert worst >= 10, (name, entry, where, worst)
