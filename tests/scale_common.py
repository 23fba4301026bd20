"""Shared by tests/test_scale_edges.py (CPU) and tests/test_gpu_scale_edges.py (-m gpu): the weight packer of the split and the fp32
arithmetic restated in numpy from the comments of tdmpc2_amd/csrc/refresh_kernels.cuh (scale rule, source-column map, fragment
order, hi / lo split, padded bias, LayerNorm vectors, scale records, encoder owner, segment order), a decoder of a packed slab,
and `stagger`: a checkpoint rescaled by powers of two so that every scale record of a handle differs from its neighbours.
Nothing here comes from a HIP result, and nothing here touches a torch device.

The scale rule (k_rf_scales), per net, ensemble member and layer:
  kw = clamp(14 - exponent(max finite |W|), -40, 40), exponent(m) the e of m = f 2^e with f in [0.5, 1); 14 when the maximum is 0
  ka = clamp(min(5, 15 - exponent(B)), -24, .), B = sqrt(width - 1) max|g| + max|b| in fp32, for LayerNorm + Mish layers; else 5
  oscale = 2^-(kw + ka_in), ka_in = 5 for layer 0 and the previous layer's ka otherwise
The 32-byte record is `<ffIifiII`: wscale = 2^kw, oscale, bits of max|W|, kw, ascale = 2^ka, ka, bits of max|g|, bits of max|b|."""
import collections
import struct

import numpy as np

from tests import refresh_common as rc

PREFIX = {"dynamics": "_dynamics", "reward": "_reward", "pi": "_pi", "termination": "_termination", "q": "_Qs.params",
          "target_q": "_target_Qs_params"}
TAKES_ACTION = ("dynamics", "reward", "q", "target_q")
ACT_LOG2 = 5
RECORD = "<ffIifiII"
RECORD_NAMES = ("wscale", "oscale", "maxbits", "kw", "ascale", "ka", "gmax", "bmax")
KW_CLAMP, KA_FLOOR = 40, -24
F16_MAX = 65504.0

Segment = collections.namedtuple("Segment", "owner member layer kind data shape")   # shape: (CT, KB) of a weight slab, else None


def as_numpy(sd):
    """The checkpoint as fp32 numpy arrays (torch CPU tensors are accepted)."""
    return {k: np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in sd.items()}


def nets_of(sd, cfg):
    """Net names in the blob's order (rc.NET_ORDER) that this checkpoint holds."""
    return [n for n in rc.NET_ORDER if f"{PREFIX[n]}.0.weight" in sd and (n != "termination" or cfg.episodic)]


def heads_of(cfg, net):
    return int(cfg.num_q) if net in ("q", "target_q") else 1


def member(sd, net, layer, name, hd):
    """One tensor of one ensemble member: `name` in weight | bias | ln.weight | ln.bias; None where the layer has none."""
    v = sd.get(f"{PREFIX[net]}.{layer}.{name}")
    if v is None:
        return None
    return v[hd] if net in ("q", "target_q") else v


# ---------------------------------------------------------------- scale rule
def _finite_max(v):
    a = np.abs(np.asarray(v, np.float32)).ravel()
    a = a[np.isfinite(a)]
    return np.float32(a.max()) if a.size else np.float32(0)


def _exponent(m):
    """e of m = f 2^e, f in [0.5, 1) (frexpf), for m > 0."""
    return int(np.frexp(np.float32(m))[1])


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def layer_record(W, g, beta, mish, ka_in):
    """The record of one layer as a dict of RECORD_NAMES.  g / beta None: a layer without LayerNorm."""
    m = _finite_max(W)
    kw = int(np.clip(14 - _exponent(m), -KW_CLAMP, KW_CLAMP)) if m > 0 else 14
    ka, gmax, bmax = ACT_LOG2, np.float32(0), np.float32(0)
    if g is not None:
        gmax, bmax = _finite_max(g), _finite_max(beta)
        if mish:
            width = W.shape[0]
            bound = np.float32(np.sqrt(np.float32(max(width - 1, 1)))) * gmax + bmax   # fp32, as the kernel computes it
            if bound > 0:
                ka = min(ka, 15 - _exponent(bound))
            ka = max(ka, KA_FLOOR)
    return dict(wscale=float(np.ldexp(np.float32(1), kw)), oscale=float(np.ldexp(np.float32(1), -(kw + ka_in))), maxbits=_bits(m), kw=kw,
                ascale=float(np.ldexp(np.float32(1), ka)), ka=ka, gmax=_bits(gmax), bmax=_bits(bmax))


def records(sd, cfg):
    """{net: [member][layer] -> record dict} of every net of the checkpoint."""
    sd = as_numpy(sd)
    out = {}
    for net in nets_of(sd, cfg):
        out[net] = []
        for hd in range(heads_of(cfg, net)):
            recs, ka_in = [], ACT_LOG2
            for l in range(3):
                r = layer_record(member(sd, net, l, "weight", hd), member(sd, net, l, "ln.weight", hd), member(sd, net, l, "ln.bias", hd),
                                 mish=l < 2, ka_in=ka_in)
                recs.append(r)
                ka_in = r["ka"]
            out[net].append(recs)
    return out


def pack_record(r):
    return struct.pack(RECORD, *(r[n] for n in RECORD_NAMES))


def unpack_records(data):
    return [dict(zip(RECORD_NAMES, struct.unpack_from(RECORD, data, 32 * l))) for l in range(3)]


# ---------------------------------------------------------------- slabs
def layer_geometry(cfg, net, layer, path, split):
    """(nz, nt, na, Kp, KB) of a stored layer.  The packed contraction axis is [z or hidden (nz) | action (na) | zeros]: the fused
    family (path 1) pads the action columns to 16, the layered family (path 2) the whole row to 32."""
    nz = cfg.latent_dim if layer == 0 else cfg.mlp_dim
    nt = int(cfg.task_dim) if layer == 0 else 0
    na = cfg.action_dim if (layer == 0 and net in TAKES_ACTION) else 0
    Kp = -(-(nz + na) // 32) * 32 if path == 2 else nz + -(-na // 16) * 16
    return nz, nt, na, Kp, Kp // (16 if split else 8)


def packed_matrix(W, cfg, net, layer, path, split):
    """[32 CT][Kp] fp32: source columns [z | task | a] mapped to [z | a], rows beyond `out` and padded columns zero."""
    nz, nt, na, Kp, KB = layer_geometry(cfg, net, layer, path, split)
    out = W.shape[0]
    assert W.shape[1] == nz + nt + na, (net, layer, W.shape)
    CT = -(-out // 32)
    P = np.zeros((CT * 32, Kp), np.float32)
    P[:out, :nz] = W[:, :nz]
    P[:out, nz:nz + na] = W[:, nz + nt:]
    return P, CT, KB


def split_planes(P, kw):
    """(hi, lo) f16 of P 2^kw: hi by round-to-nearest-even, lo the rounded residual, both computed from the fp32 product."""
    with np.errstate(all="ignore"):
        v = P * np.ldexp(np.float32(1), kw)
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def split_slab(P, CT, KB, kw):
    """[ct][kb][hi / lo][lane][8] f16, row = 32 ct + (lane & 31), k = 16 kb + 8 (lane >> 5) + e."""
    frag = lambda h: h.reshape(CT, 32, KB, 2, 8).transpose(0, 2, 3, 1, 4).reshape(CT, KB, 64, 8)
    hi, lo = split_planes(P, kw)
    return np.ascontiguousarray(np.stack([frag(hi), frag(lo)], axis=2))


def fp32_slab(P, CT, KB):
    """[ct][kb][lane][4] fp32, row = 32 ct + (lane & 31), k = 8 kb + 4 (lane >> 5) + r."""
    return np.ascontiguousarray(P.reshape(CT, 32, KB, 2, 4).transpose(0, 2, 3, 1, 4).reshape(CT, KB, 64, 4))


def unfragment(slab, split):
    """Inverse of the fragment order: split [CT][KB][2][64][8] f16 -> (hi, lo) [32 CT][16 KB]; fp32 [CT][KB][64][4] -> [32 CT][8 KB]."""
    if not split:
        CT, KB = slab.shape[:2]
        return slab.reshape(CT, KB, 2, 32, 4).transpose(0, 3, 1, 2, 4).reshape(CT * 32, KB * 8)
    CT, KB = slab.shape[:2]
    un = lambda x: x.reshape(CT, KB, 2, 32, 8).transpose(0, 3, 1, 2, 4).reshape(CT * 32, KB * 16)
    return un(slab[:, :, 0]), un(slab[:, :, 1])


def decode(segment, record):
    """The [32 CT][in-packed] matrix a split weight segment stands for, (hi + lo) 2^-kw in fp64; fp32 segments (record None): as stored."""
    CT, KB = segment.shape
    if record is None:
        return unfragment(np.frombuffer(segment.data, np.float32).reshape(CT, KB, 64, 4), False).astype(np.float64)
    hi, lo = unfragment(np.frombuffer(segment.data, np.float16).reshape(CT, KB, 2, 64, 8), True)
    with np.errstate(all="ignore"):
        return (hi.astype(np.float64) + lo.astype(np.float64)) * 2.0 ** -record["kw"]


# ---------------------------------------------------------------- blob assembly
def _f32(v):
    return np.ascontiguousarray(v, np.float32).tobytes()


def _padded(v, n):
    out = np.zeros(n, np.float32)
    out[:len(v)] = v
    return out.tobytes()


def restated_segments(sd, cfg, path, split):
    """[Segment] of the packed blob in its canonical order: per net (rc.NET_ORDER) and ensemble member the three layers' weight slab,
    bias padded to 32 CT, LayerNorm gain and bias (padded to a multiple of 4), task-embedding columns wemb[row][c] (multitask, layer
    0), then -- split -- the three records; then the state encoder, per layer the transposed matrix [in][out] and three vectors."""
    sd = as_numpy(sd)
    recs = records(sd, cfg) if split else None
    out = []
    for net in nets_of(sd, cfg):
        for hd in range(heads_of(cfg, net)):
            for l in range(3):
                W = member(sd, net, l, "weight", hd)
                P, CT, KB = packed_matrix(W, cfg, net, l, path, split)
                slab = split_slab(P, CT, KB, recs[net][hd][l]["kw"]) if split else fp32_slab(P, CT, KB)
                out.append(Segment(net, hd, l, "weight", slab.tobytes(), (CT, KB)))
                out.append(Segment(net, hd, l, "bias", _padded(member(sd, net, l, "bias", hd), CT * 32), None))
                g = member(sd, net, l, "ln.weight", hd)
                if g is not None:
                    n4 = -(-W.shape[0] // 4) * 4
                    out.append(Segment(net, hd, l, "ln.weight", _padded(g, n4), None))
                    out.append(Segment(net, hd, l, "ln.bias", _padded(member(sd, net, l, "ln.bias", hd), n4), None))
                nz, nt = layer_geometry(cfg, net, l, path, split)[:2]
                if nt > 0:
                    out.append(Segment(net, hd, l, "wemb", _f32(W[:, nz:nz + nt]), None))
            if split:
                out.append(Segment(net, hd, None, "records", b"".join(pack_record(r) for r in recs[net][hd]), None))
    l = 0
    while f"_encoder.state.{l}.weight" in sd:
        p = f"_encoder.state.{l}."
        out.append(Segment("encoder", 0, l, "weight^T", _f32(sd[p + "weight"].T), None))
        for n in ("bias", "ln.weight", "ln.bias"):
            out.append(Segment("encoder", 0, l, n, _f32(sd[p + n]), None))
        l += 1
    return out


def owner_digests(segments):
    import hashlib

    hs = {}
    for s in segments:
        hs.setdefault(s.owner, hashlib.sha256()).update(s.data)
    return {o: h.hexdigest() for o, h in hs.items()}


ELEMENT = {"weight": np.uint16, "records": np.uint32}


def first_difference(want, got):
    """None when the blob's segments `got` ([(owner, bytes)], rc.blob_segments) equal the restated ones; else a sentence naming owner,
    member, layer, segment kind and the first differing element."""
    return _first_difference(want, got, False)


def _first_difference(want, got, nan_ok):
    if len(want) != len(got):
        return f"{len(got)} segments, restated {len(want)}"
    for i, (w, (owner, data)) in enumerate(zip(want, got)):
        where = f"segment {i}: owner {w.owner} member {w.member} layer {w.layer} kind {w.kind}"
        if owner != w.owner or len(data) != len(w.data):
            return f"{where}: the blob has owner {owner}, {len(data)} bytes; restated {len(w.data)} bytes"
        if data == w.data:
            continue
        split_w = w.kind == "weight" and w.shape is not None and len(w.data) == w.shape[0] * w.shape[1] * 2048
        ut, ft = (np.uint16, np.float16) if split_w else (np.uint32, np.float32)
        a, b = np.frombuffer(w.data, ut), np.frombuffer(data, ut)
        bad = a != b
        if nan_ok and w.kind != "records":
            fa, fb = np.frombuffer(w.data, ft), np.frombuffer(data, ft)
            bad &= ~(np.isnan(fa) & np.isnan(fb))
        if not bad.any():
            continue
        j = int(np.argmax(bad))
        what = f"element {j}"
        if split_w:
            ct, kb, plane, lane, e = np.unravel_index(j, (w.shape[0], w.shape[1], 2, 64, 8))
            what += f" (row {32 * ct + (lane & 31)}, packed column {16 * kb + 8 * (lane >> 5) + e}, {'lo' if plane else 'hi'})"
        elif w.kind == "records":
            what += f" (layer {j // 8}, field {RECORD_NAMES[j % 8]})"
        return f"{where}: {what}: restated 0x{int(a[j]):x}, the blob holds 0x{int(b[j]):x}"
    return None


def first_difference_nan(want, got):
    """first_difference where two NaNs at the same position count as equal, whatever their payloads."""
    return _first_difference(want, got, True)


def packed_inputs_cpu(c):
    """rc.packed_inputs on the CPU.  There rc.device_sd shares memory with the case's arrays (a device copy does not), so every
    weight set starts from a clone; the recorded `input` digests say that these are the tensors the GPU test binds."""
    fresh = lambda: {k: v.clone() for k, v in rc.device_sd(c, "cpu").items()}
    yield "plain", fresh()
    sd = fresh()
    rc.perturb(sd, 1)
    yield "perturbed", sd
    for variant in rc.EDGE_VARIANTS:
        sd = fresh()
        rc.edge_weights(sd, variant)
        yield variant, sd


# ---------------------------------------------------------------- staggering
# A plan maps (net, member) to dict(s=(s0, s1, s2), g=(g0, g1)).  Layer l's weight AND bias are multiplied by 2^s_l (a hidden layer's
# LayerNorm undoes it up to its epsilon; the pre-activation mix of weight and bias is the fixture's); a hidden layer's LayerNorm gain
# AND bias by 2^g_l and the next layer's weight by 2^-g_l, so the next pre-activation keeps its size.  Then
#   kw_l = kw_l(fixture) - s_l + g_(l-1),   ka_l = min(5, 15 - exponent(2^g_l B_l(fixture))),   oscale exponent = -(kw_l + ka_(l-1)).
S_HIDDEN = tuple(range(0, 16))
S_LAST = (0, -1, -2, 1, -3, -4, -5, -6, 2)   # a head's logits times 4 and more put the fp32 oracle's error above the gates' floors
S_LAST_TERMINATION = (3, 4, 2, 5, 1)   # the termination logits spread out (as in the small_ep_fire case), so that few rows sit at the threshold
KA_PAIRS = ((5, 3), (4, 2), (3, 1), (2, 5), (1, 4))   # (ka of layer 0, ka of layer 1): different within a pair, different between pairs


def launch_groups(cfg, nets):
    """Sets of (net, member) whose same-layer records one launch can hold: the rollout's nets, each ensemble, and the nets of a value
    tail (pi then the heads); plus every online head with its target twin (a read from the other ensemble)."""
    nq = int(cfg.num_q)
    groups = [[(n, 0) for n in ("dynamics", "reward", "pi", "termination") if n in nets]]
    for ens in ("q", "target_q"):
        if ens in nets:
            groups.append([(ens, h) for h in range(nq)] + [("pi", 0)])
    if "q" in nets and "target_q" in nets:
        groups += [[("q", h), ("target_q", h)] for h in range(nq)]
    return groups


def ka_targets(cfg, nets, ka_min=1):
    """(ka0, ka1) per (net, member): the pairs of KA_PAIRS no lower than ka_min, so that dynamics / reward and any two heads differ."""
    pairs = [p for p in KA_PAIRS if min(p) >= ka_min] or [(5, 4), (4, 5)]
    out, single = {}, {"dynamics": 0, "reward": 1, "pi": 2, "termination": 3}
    for n in nets:
        for h in range(heads_of(cfg, n)):
            i = single[n] if n in single else h + (1 if n == "target_q" else 0)
            out[(n, h)] = pairs[i % len(pairs)]
    return out


def stagger_plan(sd, cfg, ka_min=1):
    """Greedy: per (net, member) the gains that give ka_targets, then the smallest weight shifts for which the oscale exponent of
    every layer differs from every record of the same net placed so far and from the same-layer records of its launch groups."""
    sd = as_numpy(sd)
    nets = nets_of(sd, cfg)
    base, targets, groups = records(sd, cfg), ka_targets(cfg, nets, ka_min), launch_groups(cfg, nets)
    peers = {}
    for grp in groups:
        for m in grp:
            peers.setdefault(m, set()).update(x for x in grp if x != m)
    members = [(net, hd) for net in nets for hd in range(heads_of(cfg, net))]
    gains, kas = {}, {}
    for key in members:
        net, hd = key
        b, g = base[net][hd], []
        for l in (0, 1):
            t = targets[key][l]
            bound = np.float32(np.sqrt(np.float32(sd[f"{PREFIX[net]}.{l}.weight"].shape[-2] - 1))) * np.uint32(b[l]["gmax"]).view(np.float32) \
                + np.uint32(b[l]["bmax"]).view(np.float32)
            g.append(0 if t == ACT_LOG2 else 15 - t - _exponent(bound))
            assert g[-1] > 0 or t == ACT_LOG2, (net, hd, l, t, bound)
        gains[key], kas[key] = g, (ACT_LOG2, targets[key][0], targets[key][1])
    placed = {key: {} for key in members}   # placed[(net, member)][layer] = oscale exponent
    shifts = {key: {} for key in members}
    for layers in ((2,), (0, 1)):   # the last layers first: they have the fewest shifts to choose from
        for key in members:
            net, hd = key
            for l in layers:
                avoid = {e for k2 in members if k2[0] == net for e in placed[k2].values()}
                avoid |= {placed[p][l] for p in peers.get(key, ()) if l in placed[p]}
                for cand in (S_HIDDEN if l < 2 else S_LAST_TERMINATION if net == "termination" else S_LAST):
                    e = -(base[net][hd][l]["kw"] - cand + (gains[key][l - 1] if l else 0) + kas[key][l])
                    if e not in avoid:
                        break
                else:
                    raise AssertionError(f"no shift left for {key} layer {l}")
                shifts[key][l], placed[key][l] = cand, e
    return {key: dict(s=tuple(shifts[key][l] for l in range(3)), g=tuple(gains[key])) for key in members}


def stagger(sd, cfg, plan):
    """The checkpoint (numpy, fp32) rescaled by `plan`; every factor is a power of two, so each product is exact."""
    out = {k: v.copy() for k, v in as_numpy(sd).items()}
    p2 = lambda e: np.ldexp(np.float32(1), int(e))
    for (net, hd), p in plan.items():
        sel = (hd,) if net in ("q", "target_q") else ()
        t = lambda l, n: out[f"{PREFIX[net]}.{l}.{n}"]
        for l in range(3):
            t(l, "weight")[sel] *= p2(p["s"][l] - (p["g"][l - 1] if l else 0))
            t(l, "bias")[sel] *= p2(p["s"][l])
            if l < 2:
                t(l, "ln.weight")[sel] *= p2(p["g"][l])
                t(l, "ln.bias")[sel] *= p2(p["g"][l])
    return out


def stagger_violations(recs, cfg):
    """The conditions a staggered checkpoint's records must meet, as a list of sentences (empty: all hold)."""
    bad = []
    ex = {(n, h): [int(round(np.log2(r["oscale"]))) for r in recs[n][h]] for n in recs for h in range(len(recs[n]))}
    ka = {(n, h): [r["ka"] for r in recs[n][h]] for n in recs for h in range(len(recs[n]))}
    for n in recs:   # pairwise distinct within each net, over members and layers
        flat = [e for h in range(len(recs[n])) for e in ex[(n, h)]]
        if len(set(flat)) != len(flat):
            bad.append(f"{n}: oscale exponents repeat within the net: {flat}")
    for grp in launch_groups(cfg, list(recs)):   # same-layer records of nets that can share a launch
        for l in range(3):
            es = [ex[m][l] for m in grp]
            if len(set(es)) != len(es):
                bad.append(f"layer {l} of {grp}: oscale exponents {es}")
    if len({k for v in ka.values() for k in v[:2]}) < 3:
        bad.append("ka takes fewer than three values on the handle")
    for m, v in ka.items():
        if v[0] == v[1]:
            bad.append(f"{m}: ka of the two hidden layers equal ({v[0]})")
    pairs = [(("dynamics", 0), ("reward", 0))] if "dynamics" in recs and "reward" in recs else []
    for ens in ("q", "target_q"):
        if ens in recs:
            pairs += [((ens, a), (ens, b)) for a in range(len(recs[ens])) for b in range(a)]
    for a, b in pairs:
        for l in (0, 1):
            if ka[a][l] == ka[b][l]:
                bad.append(f"ka of layer {l} equal on {a} and {b} ({ka[a][l]})")
    return bad


# ---------------------------------------------------------------- a slipped record, as the fp64 oracle sees it
def slipped(sd, net, hd, layer, up):
    """A kernel that takes a neighbour's oscale for this record scales the layer's accumulator by a power of two: the oracle's model of
    a slip by ONE exponent is that layer's weight times 2 (up) or 0.5, the bias untouched."""
    out = dict(sd)
    k = f"{PREFIX[net]}.{layer}.weight"
    w = np.array(as_numpy({k: sd[k]})[k], np.float32, copy=True)
    w[(hd,) if net in ("q", "target_q") else ()] *= np.float32(2.0 if up else 0.5)
    out[k] = w
    return out


# ---------------------------------------------------------------- entry points on a staggered checkpoint: inputs, oracle, gates
# Every gate below is the one the entry point's existing whole-chain test uses against the oracle, imported where it is a function:
#   estimate_value, plan   tests/test_gpu_adversarial.py's bar: worst |v - v64| / max(1, |v64|) < max(1e-4, 1.5 x the fp32 oracle's worst).
#                          That file writes the bar inline (`hip < max(1e-4, 1.5 * ref)`), so VALUE_FLOOR / VALUE_FACTOR restate it; its
#                          second conjunct, hip < 3 ref + 1e-6, belongs to the heavy-tailed weights of that file and is not part of the
#                          gate here.  The action gate of policy_value is the expression of test_gpu_value_edges.py's whole-chain test.
#   td_target, policy_value  value_common.chain_expect (chain_gate), the action max(2e-5, 2 |oracle fp32 - oracle fp64|)
#   policy_loss            policy_loss_common.tol on the per-row fields the oracle has (action, q)
#   model_rollout / losses model_common.tol per field (item 6 of tests/test_gpu_model_edges.py)
FUSED = ("c1", "mt5", "c1_ep")
LAYERED = ("small", "small_ep", "small_mt")
FUSED_SHAPE = dict(num_samples=128, num_elites=16)   # the smallest plan the fused family's two-cluster route is tested at
ENTRY_POINTS = ("estimate_value", "plan", "td_target", "policy_value", "policy_loss", "model_rollout", "model_losses")
VALUE_FLOOR, VALUE_FACTOR = 1e-4, 1.5
CHAIN_T, CHAIN_B = 5, 26     # 130 rows: two 64-row tiles and a tail; policy_loss sees them as [T, B]
MODEL_B = 43                 # H B = 129 rows at H = 3
PLAN_SEPARATION_ITERS = 1


def head_pairs(nq):
    """qidx pairs that between them use every head."""
    return {2: [(0, 1), (1, 0)], 3: [(0, 2), (1, 0)], 5: [(0, 2), (1, 0), (3, 4)]}[int(nq)]


def _t(sd):
    import torch

    return {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}


class Scenario:
    """One handle's staggered checkpoint and the seeded inputs of every entry point; `raw(kind, sd, dtype)` evaluates the oracle
    (oracle/planner_oracle.py) and `expect(entry)` gives {key: (fp64 value, gate)}."""

    def __init__(self, name, ka_min=1, custom=None):
        """custom: (config name, overrides, plans) -- a layered shape outside oracle.cases, the head pairs going round over its plans."""
        from oracle import cases
        from tdmpc2_amd import synth
        from tdmpc2_amd.config import named_config
        from tests import model_common as mc
        from tests import value_common as vc

        if custom is None:
            cfg_name, over, _, _, head_std = cases.CASES[name]
            over = dict(over, **(FUSED_SHAPE if name in FUSED else {}))
        else:
            (cfg_name, over, n_plans), head_std = custom, 0.06
        cfg = named_config(cfg_name, **over)
        self.name, self.path = name, 1 if name in FUSED else 2
        self.pairs = head_pairs(cfg.num_q)
        self.E = E = len(self.pairs) if custom is None else n_plans
        self.c = c = cases.build_custom(cfg, E, False, head_std, name=name)
        self.cfg, self.I = cfg, c["iterations"]
        self.base_sd = as_numpy(c["sd"])
        self.plan = stagger_plan(self.base_sd, cfg, ka_min)
        self.sd = stagger(self.base_sd, cfg, self.plan)
        H, N, A, nq = cfg.horizon, cfg.num_samples, cfg.action_dim, cfg.num_q
        rng = np.random.default_rng(7)
        self.n_tasks = len(cfg.tasks) if cfg.multitask else 0
        masks = self.sd["_action_masks"].astype(np.float32) if cfg.multitask else None
        # estimate_value: one qidx pair per plan
        self.v_actions = rng.uniform(-1, 1, (E, H, N, A)).astype(np.float32)
        if cfg.multitask:
            self.v_actions *= masks[np.array(c["tasks"])][:, None, None, :]
        self.v_eps = rng.standard_normal((E, N, A)).astype(np.float32)
        self.v_qidx = np.array([self.pairs[e % len(self.pairs)] for e in range(E)], np.int32)
        # plan: the case's tape with the head pairs going round over plans and iterations
        c["tape"]["qidx"] = np.array([[self.pairs[(e + it) % len(self.pairs)] for it in range(self.I)] for e in range(E)], np.int32)
        self.p_actions = rng.uniform(-1, 1, (E, PLAN_SEPARATION_ITERS, H, N, A)).astype(np.float32)
        if cfg.multitask:
            self.p_actions *= masks[np.array(c["tasks"])][:, None, None, None, :]
        # td_target / policy_value / policy_loss: CHAIN_T x CHAIN_B rows
        R = CHAIN_T * CHAIN_B
        self.R = R
        self.ch_z = synth.make_latents(cfg, R, seed=R)
        self.ch_eps = vc.chain_eps(R, A)
        self.ch_rew, self.ch_term = vc.row_inputs(R)
        self.ch_tasks_b = vc.task_pattern("mod7", CHAIN_B, self.n_tasks) if cfg.multitask else None
        self.ch_tasks = np.tile(self.ch_tasks_b, CHAIN_T) if cfg.multitask else None
        self.disc_np = vc.distinct_discounts(self.n_tasks) if cfg.multitask else None
        self.discount = None if cfg.multitask else float(c["discounts"][0])
        self.ch_pairs = vc.ordered_pairs(nq)
        self.pl_qidx = self.pairs[-1]
        # model_rollout / model_losses
        mi = mc.inputs(cfg, MODEL_B)
        self.m_z0, self.m_act = mi["z0"], mi["actions"]
        self.m_tasks = None if mi["tasks"] is None else np.asarray(mi["tasks"], np.int64)
        self.m_next = synth.make_latents(cfg, H * MODEL_B, seed=21).reshape(H, MODEL_B, cfg.latent_dim)
        self.m_rew = rng.standard_normal((H, MODEL_B)).astype(np.float32)
        self.m_td = (3 * rng.standard_normal((H, MODEL_B))).astype(np.float32)
        self.m_term = (rng.random((H, MODEL_B)) < 0.3).astype(np.float32)
        self._raw, self._slipped = {}, {}
        if cfg.episodic:
            # estimate_value reads the termination net through `sigmoid(.) > 0.5` alone: with the fixture's bias it never fires and
            # the net's records would be invisible.  Move the bias so that half of estimate_value's sample rows terminate within the
            # horizon (fp64 oracle: the median over the rows of the largest logit along the rollout).
            self.sd["_termination.2.bias"] = (self.sd["_termination.2.bias"] - np.float32(np.median(self._value_term_logits().max(1)))).astype(np.float32)

    def _value_term_logits(self):
        """[E, H, N] termination logits along estimate_value's rollouts, fp64 oracle."""
        import torch
        from oracle import planner_oracle as po

        cfg, dt = self.cfg, torch.float64
        m = po.OracleModel(cfg, _t(self.sd), dtype=dt)
        out = []
        for e in range(self.E):
            z, row = torch.as_tensor(self.c["z0"][e:e + 1]).to(dt).repeat(cfg.num_samples, 1), []
            for t in range(cfg.horizon):
                z = m.next(z, torch.as_tensor(self.v_actions[e, t]).to(dt), None)
                row.append(po.mlp_forward(m.sd, "_termination", z)[..., 0].numpy())
            out.append(np.stack(row))
        return np.stack(out)

    # ---- which records an entry point reads: [(net, member)]
    def reads(self, entry):
        nq, ep = range(int(self.cfg.num_q)), [("termination", 0)] if self.cfg.episodic else []
        q, tq = [("q", h) for h in nq], [("target_q", h) for h in nq]
        roll = [("dynamics", 0), ("reward", 0)] + ep
        if entry == "estimate_value":
            return roll + [("pi", 0)] + q
        if entry == "plan":
            used = {int(h) for e in range(self.E) for it in range(PLAN_SEPARATION_ITERS) for h in self.c["tape"]["qidx"][e, it]}
            return roll + [("pi", 0)] + [("q", h) for h in sorted(used)]
        if entry == "td_target":
            return [("pi", 0)] + tq
        if entry == "policy_value":
            return [("pi", 0)] + q + tq
        if entry == "policy_loss":
            return [("pi", 0)] + [("q", h) for h in self.pl_qidx]
        return roll + q + (tq if entry == "model_rollout" else [])     # model_rollout: online and use_target; model_losses: online

    KIND = {"estimate_value": "value", "plan": "planvalue", "td_target": "chain", "policy_value": "chain", "policy_loss": "chain",
            "model_rollout": "model", "model_losses": "model"}

    # ---- the oracle
    def value_of(self, sd, dt, actions, eps, qidx, envs=None):
        """po.estimate_value per plan -> [len(envs), N] (fp64 numpy)."""
        import torch
        from oracle import planner_oracle as po

        c, cfg = self.c, self.cfg
        m = po.OracleModel(cfg, _t(sd), dtype=dt)
        out = []
        for i, e in enumerate(range(self.E) if envs is None else envs):
            task = None if c["tasks"] is None else c["tasks"][e]
            disc = c["discounts"][e]
            disc = disc.to(dt) if torch.is_tensor(disc) and dt == torch.float64 else disc
            z = torch.as_tensor(c["z0"][e:e + 1]).to(dt).repeat(cfg.num_samples, 1)
            v = po.estimate_value(m, z, torch.as_tensor(actions[i]).to(dt), task, disc, torch.as_tensor(eps[i]).to(dt), torch.as_tensor(qidx[i]))
            out.append(v.squeeze(1).numpy().astype(np.float64))
        return np.stack(out)

    def _chain(self, sd, dt):
        """value_common.oracle_chain: (action [R, A], q [2, num_q, R]) of the evaluation in `dt`."""
        import torch
        from tests import value_common as vc

        o32, o64 = vc.oracle_chain(self.cfg, sd, self.ch_z, self.ch_eps, self.ch_tasks)
        return o64 if dt == torch.float64 else o32

    def _model(self, sd, dt):
        """The open-loop rollout and every head on it: zs [H+1, B, L], reward_logits [H, B, bins], q_logits / tq_logits [nq, H, B, bins],
        term_logit [H+1, B] (episodic)."""
        import torch
        from oracle import planner_oracle as po

        cfg = self.cfg
        m = po.OracleModel(cfg, _t(sd), dtype=dt)
        tk = None if self.m_tasks is None else torch.as_tensor(self.m_tasks)
        z, act = torch.as_tensor(self.m_z0).to(dt), torch.as_tensor(self.m_act).to(dt)
        zs, rl, ql, tl = [z], [], [], []
        for t in range(cfg.horizon):
            x = torch.cat([m.task_emb(z, tk) if cfg.multitask else z, act[t]], -1)
            rl.append(m.reward(z, act[t], tk))
            ql.append(po.ensemble_forward(m.sd, "_Qs.params", x))
            tl.append(po.ensemble_forward(m.sd, "_target_Qs_params", x))
            z = m.next(z, act[t], tk)
            zs.append(z)
        n = lambda x: x.numpy().astype(np.float64)
        out = dict(zs=n(torch.stack(zs)), reward_logits=n(torch.stack(rl)), q_logits=n(torch.stack(ql, 1)), tq_logits=n(torch.stack(tl, 1)))
        if cfg.episodic:
            out["term_logit"] = n(po.mlp_forward(m.sd, "_termination", torch.stack(zs))[..., 0])
        return out

    def raw(self, kind, sd=None, dt64=True):
        import torch

        dt = torch.float64 if dt64 else torch.float32
        key = (kind, dt64) if sd is None else None
        if key in self._raw:
            return self._raw[key]
        s = self.sd if sd is None else sd
        if kind == "value":
            out = self.value_of(s, dt, self.v_actions, self.v_eps, self.v_qidx)
        elif kind == "planvalue":
            tp = self.c["tape"]
            out = np.stack([self.value_of(s, dt, self.p_actions[:, it], tp["pi_eps"][:, it], tp["qidx"][:, it]) for it in range(PLAN_SEPARATION_ITERS)], 1)
        elif kind == "chain":
            out = self._chain(s, dt)
        else:
            out = self._model(s, dt)
        if key is not None:
            self._raw[key] = out
        return out

    # ---- expectations: {key: (v64, gate)} from the two evaluations
    @staticmethod
    def value_fields(v64, v32, key="value"):
        scale = np.maximum(1.0, np.abs(v64))
        ref = float(np.max(np.abs(v32 - v64) / scale))
        return {key: (v64, max(VALUE_FLOOR, VALUE_FACTOR * ref) * scale)}, ref

    def model_losses_of(self, o, dtype):
        from types import SimpleNamespace
        from tests import model_common as mc

        cfg = self.cfg
        ns = SimpleNamespace(num_bins=cfg.num_bins, vmin=cfg.vmin, vmax=cfg.vmax, rho=cfg.rho, episodic=cfg.episodic, consistency_coef=20.0,
                             reward_coef=0.1, value_coef=0.1, termination_coef=1.0)
        a = lambda v: np.asarray(v).astype(dtype)
        tl = a(o["term_logit"]) if cfg.episodic else np.zeros(o["zs"].shape[:2], dtype)
        with np.errstate(all="ignore"):
            return mc.losses_from(ns, a(o["zs"]), a(o["reward_logits"]), a(o["q_logits"]), tl, a(self.m_next), a(self.m_rew), a(self.m_td), a(self.m_term))

    def derive(self, entry, o64, o32):
        """{key: (v64, gate)} of `entry` from the raw oracle outputs of its kind."""
        from tests import model_common as mc
        from tests import policy_loss_common as pc
        from tests import value_common as vc

        if entry in ("estimate_value", "plan"):
            return self.value_fields(o64, o32)[0]
        out = {}
        if entry in ("td_target", "policy_value"):
            disc = self.disc_np[self.ch_tasks] if self.cfg.multitask else np.float32(self.discount)
            for pair in self.ch_pairs:
                if entry == "td_target":
                    out[("td", pair)] = vc.chain_expect(o32, o64, True, pair, "min", self.ch_rew, self.ch_term, disc)
                else:
                    for target in (False, True):
                        for red in ("min", "avg"):
                            out[("q", target, red, pair)] = vc.chain_expect(o32, o64, target, pair, red)
            if entry == "policy_value":
                out[("action",)] = (o64[0], np.maximum(2e-5, 2 * np.abs(o32[0] - o64[0])))
            return out
        if entry == "policy_loss":
            a, b = self.pl_qidx
            q64, q32 = (vc.reduce_of(o[1][0][a], o[1][0][b], "avg") for o in (o64, o32))
            out["q"] = (q64, pc.tol(q64, np.abs(q32 - q64).max()))
            out["action"] = (o64[0], pc.tol(o64[0], np.abs(o32[0] - o64[0]).max()))
            return out
        fields = ["zs", "reward_logits", "q_logits", "tq_logits"] + (["term_logit"] if self.cfg.episodic else [])
        if entry == "model_rollout":
            for k in fields:
                out[k] = (o64[k], mc.tol(o64[k], np.abs(o32[k] - o64[k]).max()))
            return out
        for k in fields:   # the rollout outputs a model_losses call returns with `want` (online heads)
            if k != "tq_logits":
                out[k] = (o64[k], mc.tol(o64[k], np.abs(o32[k] - o64[k]).max()))
        (l64, s64), (l32, s32) = self.model_losses_of(o64, np.float64), self.model_losses_of(o32, np.float32)
        out["losses"] = (l64, mc.tol(l64, np.abs(l32 - l64).max()))
        out["step_means"] = (s64, mc.tol(s64, np.abs(s32 - s64).max()))
        return out

    def expect(self, entry):
        kind = self.KIND[entry]
        return self.derive(entry, self.raw(kind), self.raw(kind, dt64=False))

    def fp32_ratio(self, entry):
        """Worst |oracle fp32 - oracle fp64| / floor of the gate: the gate sits at its floor where 2 x (1.5 x for values) this is <= 1."""
        kind = self.KIND[entry]
        o64, o32 = self.raw(kind), self.raw(kind, dt64=False)
        if entry in ("estimate_value", "plan"):
            return self.value_fields(o64, o32)[1] / VALUE_FLOOR
        exp = self.derive(entry, o64, o32)
        mine = self.derive(entry, o64, o64)   # the same gates with a zero fp32 term: the floors
        return max(float(np.max(exp[k][1] / mine[k][1])) for k in exp)

    def separation(self, entry, net, hd, layer, up):
        """How far, in gates, the fp64 oracle of `entry` moves when record (net, hd, layer) slips one exponent."""
        kind = self.KIND[entry]
        base = self.expect(entry)
        key = (kind, net, hd, layer, up)   # td_target, policy_value and policy_loss share one evaluation, the two model entries another
        if key not in self._slipped:
            self._slipped[key] = self.raw(kind, slipped(self.sd, net, hd, layer, up))
        moved = self.derive(entry, self._slipped[key], self.raw(kind, dt64=False))
        with np.errstate(all="ignore"):
            return max(float(np.nanmax(np.abs(moved[k][0] - base[k][0]) / base[k][1])) for k in base)
