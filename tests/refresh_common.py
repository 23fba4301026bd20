"""Shared by the weight-refresh tests (tests/test_gpu_refresh.py, tests/test_refresh_golden.py) and tools/make_soft_update_golden.py:
the seeded inputs of the soft-update fixture, the gate of a lerped element, a reader of the packed blob's segment table, and
the weight sets and per-owner digests of the packed-bytes fixture (tools/make_packed_digests.py)."""
import hashlib
import struct

import numpy as np

GOLDEN = "soft_update_tiny.npz"
STEPS, TAU = 3, 0.01
Q_KEYS = [f"{l}.{n}" for l in range(3) for n in ("weight", "bias", "ln.weight", "ln.bias") if not (l == 2 and n.startswith("ln"))]

# |out - ref64| <= 2^-23 (|t| + |o|): three roundings of either lerp form, fused multiply-add or not.  With d = o - t (one
# rounding, |d| <= |t| + |o|), w d or d (1 - w) (one more, the factor at most 1) and the final sum (|result| <= max(|t|, |o|)),
# each rounding contributes at most 2^-24 of a quantity bounded by |t| + |o|; 1 - w itself adds a relative 2^-24 to a product
# bounded by |d|.  Four terms of 2^-24 (|t| + |o|) at the very most, of which the sum's is at most half: below 2^-23 (|t| + |o|).
GATE = 2.0 ** -23
# the fixture stores the reference's fp64 result as its distance from the reference's fp32 result, in units of the gate and in
# fp16 (fp64 tensors would not fit the repository's size limit): reproduced to within 2^-33 (|t| + |o|) -- the tool checks it --
# by which the tests tighten the gate
TAIL_ERR = 2.0 ** -33


def tiny_inputs():
    """Online Q tensors of the three steps and the initial target tensors of the `tiny` case: the case's own ensembles, the target
    moved off the online one and the online one moved between the steps as an optimiser would (numpy draws: the same on every host)."""
    from oracle import cases

    sd = cases.build_case("tiny")["sd"]
    rng = np.random.default_rng(20240607)
    target = {k: (np.asarray(sd[f"_target_Qs_params.{k}"], np.float32)
                  + np.float32(0.05) * rng.standard_normal(sd[f"_target_Qs_params.{k}"].shape).astype(np.float32)) for k in Q_KEYS}
    online, cur = [], {k: np.asarray(sd[f"_Qs.params.{k}"], np.float32).copy() for k in Q_KEYS}
    for _ in range(STEPS):
        cur = {k: v + np.float32(0.01) * rng.standard_normal(v.shape).astype(np.float32) for k, v in cur.items()}
        online.append(cur)
    return target, online


def digest(arrays):
    h = hashlib.sha256()
    for k in sorted(arrays):
        h.update(k.encode())
        h.update(np.ascontiguousarray(arrays[k], np.float32).tobytes())
    return h.hexdigest()


def scale_of(t, o):
    """|t| + |o| in fp64: what the gate is relative to."""
    return np.abs(np.asarray(t, np.float64)) + np.abs(np.asarray(o, np.float64))


def encode64(ref64, t32, s):
    """The fp64 result as its distance from the fp32 record in units of the gate, GATE (|t| + |o|), in fp16."""
    return ((ref64 - t32.astype(np.float64)) / np.maximum(GATE * s, 1e-300)).astype(np.float16)


def decode64(t32, r16, s):
    return t32.astype(np.float64) + r16.astype(np.float64) * (GATE * s)


def lerp64(t, o, tau):
    """torch.lerp's form in fp64 on fp32 inputs (numpy)."""
    t, o = np.asarray(t, np.float64), np.asarray(o, np.float64)
    return t + tau * (o - t) if abs(tau) < 0.5 else o - (o - t) * (1.0 - tau)


def gate_excess(out, ref64, t, o, slack=0.0):
    """max over the elements of |out - ref64| - (GATE - slack) (|t| + |o|); the gate holds when this is <= 0."""
    s = np.abs(np.asarray(t, np.float64)) + np.abs(np.asarray(o, np.float64))
    return float(np.max(np.abs(np.asarray(out, np.float64) - ref64) - (GATE - slack) * s))


# ---------------------------------------------------------------- packed blob (tdmpc2_plan_export_packed)
HDR_BYTES = 192  # struct PackHdr: magic 8, version 4, abi 4, cfg 104, has_target 4, enc_layers 4, enc_in 24, enc_out 24, nseg 8, data_bytes 8
NET_ORDER = ("dynamics", "reward", "pi", "termination", "q", "target_q")


def blob_segments(blob, cfg, split, has_target=True, enc_layers=2):
    """[(owner, bytes)] of the blob's segments in its canonical order; owner is a net name or 'encoder'."""
    nseg, data_bytes = struct.unpack_from("<QQ", blob, HDR_BYTES - 16)
    sizes = struct.unpack_from(f"<{nseg}Q", blob, HDR_BYTES)
    assert HDR_BYTES + 8 * nseg + sum(sizes) == len(blob) and sum(sizes) == data_bytes
    owners = []
    for net in NET_ORDER:
        if (net == "termination" and not cfg.episodic) or (net == "target_q" and not has_target):
            continue
        heads = int(cfg.num_q) if net in ("q", "target_q") else 1
        for _ in range(heads):
            for layer in range(3):
                ln = layer < 2 or net == "dynamics"
                owners += [net] * (2 + (2 if ln else 0) + (1 if layer == 0 and cfg.task_dim > 0 else 0))
            if split:
                owners.append(net)
    owners += ["encoder"] * (4 * enc_layers)
    assert len(owners) == nseg, (len(owners), nseg)
    out, pos = [], HDR_BYTES + 8 * nseg
    for o, n in zip(owners, sizes):
        out.append((o, blob[pos:pos + n]))
        pos += n
    return out


# ---------------------------------------------------------------- weight sets of the blob tests and of packed_digests.json
# (case, path, precision): fused split / fp32 (heads of 101 and 2 A columns, action padding), fused multitask (wemb), layered
# episodic (GBK row padding, termination net), layered fp32 multitask
CASES = [("c1", 1, 2), ("c1", 1, 1), ("mt5", 1, 2), ("small_ep", 2, 2), ("small_mt", 2, 1)]
IDS = ["c1-split", "c1-fp32", "mt5", "small_ep", "small_mt"]
EDGE_VARIANTS = ("zero_last", "ln_gain", "kw_clamps", "nonfinite")
PACKED_DIGESTS = "packed_digests.json"


def device_sd(c, device):
    """The case's checkpoint as contiguous fp32 device tensors: what a trainer holds (and a refresh reads in place)."""
    import torch

    return {k: torch.as_tensor(np.asarray(v)).to(device, torch.float32).contiguous() for k, v in c["sd"].items()
            if k.startswith(("_dynamics.", "_reward.", "_pi.", "_Qs.params.", "_termination.", "_target_Qs_params.", "_encoder.state."))}


def perturb(sd, seed, scale=0.02):
    import torch

    g = torch.Generator(device="cpu").manual_seed(seed)
    for k in sorted(sd):
        sd[k].add_((scale * torch.randn(sd[k].shape, generator=g)).to(sd[k].device))


def edge_weights(sd, variant):
    import torch

    with torch.no_grad():
        if variant == "zero_last":       # maxbits = 0: what a fresh model's zero-initialised heads give
            sd["_reward.2.weight"].zero_()
            sd["_Qs.params.2.weight"].zero_()
            sd["_target_Qs_params.2.weight"].zero_()
        elif variant == "ln_gain":       # ka leaves 5
            sd["_dynamics.0.ln.weight"][3] = 1e3
            sd["_Qs.params.1.ln.weight"][1, 7] = -1e3
            sd["_pi.1.ln.bias"][2] = 4e4
        elif variant == "kw_clamps":     # kw near and beyond its clamps
            sd["_pi.1.weight"][5, 9] = 3e4
            sd["_reward.1.weight"].fill_(1e-30)
            sd["_Qs.params.0.weight"][1, 2, 3] = 1e20
            sd["_dynamics.2.weight"].mul_(1e-30)
        elif variant == "nonfinite":     # the scan of max|W| skips them
            sd["_dynamics.1.weight"][4, 4] = float("nan")
            sd["_reward.0.weight"][0, 1] = float("inf")
            sd["_Qs.params.1.weight"][2, 1, 1] = float("-inf")
            sd["_pi.0.ln.weight"][0] = float("nan")


def packed_inputs(c, device):
    """(label, state dict) of the six weight sets the packed-bytes fixture records: the case's own, a seeded perturbation of
    them, and the four edge variants."""
    yield "plain", device_sd(c, device)
    sd = device_sd(c, device)
    perturb(sd, 1)
    yield "perturbed", sd
    for variant in EDGE_VARIANTS:
        sd = device_sd(c, device)
        edge_weights(sd, variant)
        yield variant, sd


def sd_digest(sd):
    return digest({k: v.detach().cpu().numpy() for k, v in sd.items()})


def owner_digests(blob, cfg, split):
    """{owner: SHA-256 over that owner's segments, in the blob's order}."""
    hs = {}
    for o, seg in blob_segments(blob, cfg, split):
        hs.setdefault(o, hashlib.sha256()).update(seg)
    return {o: h.hexdigest() for o, h in hs.items()}
