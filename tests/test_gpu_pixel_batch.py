"""-m gpu: the pixel encoder's MFMA batch route (pixel_batch_kernels.cuh, tdmpc2_plan_encode_pix_batch) against the fp64
reference of tests/pixel_common.py, held to the same gate as pixel_kernels.cuh in tests/test_gpu_pixel_edges.py (err / gz <= 1,
nothing loosened).  Layer-under-test probes, the shape sweep, tiled images (a row may not depend on its slot: tiles straddle
images on every layer), chunk edges, all 49 shifts, fp32 observations past expf's underflow, re-binding after a reservation, the
refusals, and agreement with encode_pix on the spread route (both inside the gate; bit_equal per case is recorded, not asserted,
and so is where the two routes part: by layer 0's tap column, and layers 1..3 behind a one-hot layer 0).
TDMPC2_PIXEL_BATCH_JSON=<file>: the worst err / gate per item and bit_equal per case are merged into that file
(profiles/pixel_batch_edges.json)."""
import json
import os

import pytest
import torch

from tests import pixel_common as pc

pytestmark = pytest.mark.gpu

_worst, _bits = {}, {}
ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = 1, 2, 4


def record(sections):
    """Merge {section: {item: value}} into the JSON file TDMPC2_PIXEL_BATCH_JSON names (no-op without it)."""
    path = os.environ.get("TDMPC2_PIXEL_BATCH_JSON")
    if not path:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc["gate"] = "pc.ref_of(case)['gz'] as tests/test_gpu_pixel_edges.py applies it (tests/pixel_common.py)"
    for section, items in sections.items():
        doc.setdefault(section, {}).update(items)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module", autouse=True)
def _dump():
    yield
    record({"mi355x_worst_err_over_gate": {k: float(v) for k, v in _worst.items()}, "bit_equal_to_encode_pix": dict(_bits)})


def _dev():
    return torch.device("cuda", 0)


def _planner(C, max_envs, multitask=False):
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.native import NativePlanner

    cfg = named_config("mt5" if multitask else "c1")
    if not multitask:
        cfg.latent_dim, cfg.num_channels, cfg.obs = 16 * C, C, "rgb"
    return NativePlanner(cfg, cfg.iterations, _dev(), max_envs=max_envs)


def _bind(p, case):
    p.bind_pixel_encoder({k: v.to(_dev()) for k, v in pc.state_dict(case["Ws"], case["Bs"]).items()})


def _inputs(case, n=None):
    m = len(case["obs"])
    idx = torch.arange(m if n is None else n) % m
    obs = case["obs"][idx].contiguous().to(_dev())
    shift = torch.tensor(case["shifts"], dtype=torch.int32)[idx].contiguous().to(_dev())
    return obs, shift


def _encode(p, case, n=None, planning=False):
    """z [n, 16 C] of the case's images tiled to n rows (image i % m in row i), as a CPU tensor."""
    obs, shift = _inputs(case, n)
    z = (p.encode_pix if planning else p.encode_pix_batch)(obs, shift)
    torch.cuda.synchronize()
    return z.cpu()


def _gate(item, z, case, probe=False):
    """Rows of the case's images against the reference; rows beyond them repeat them bit for bit."""
    ref, n = pc.ref_of(case), len(case["obs"])
    m = min(n, len(z))
    if probe:
        assert ref["g"][3].max().item() <= pc.G_MAX
    assert torch.isfinite(z).all(), item
    for i in range(n, len(z)):
        assert torch.equal(z[i], z[i % n]), (item, i)
    ratio = float(((z[:m].double() - ref["z"][:m]).abs() / ref["gz"][:m]).max())
    print(f"{item}: worst err / gate {ratio:.4f}")
    _worst[item] = max(_worst.get(item, 0.0), ratio)
    assert ratio <= 1.0, (item, ratio)


@pytest.mark.parametrize("fp32", [False, True], ids=["u8", "fp32"])
@pytest.mark.parametrize("L", [0, 1, 2, 3])
def test_layer_under_test_probes(L, fp32):
    p = _planner(pc.PROBE_C, 4)
    for i in range(len(pc.PROBE_RC[L])):
        case = pc.probe_case(L, i, fp32)
        _bind(p, case)
        p.reserve_pix_batch(4)
        _gate(f"probe L{L} {'fp32' if fp32 else 'u8'}", _encode(p, case), case, probe=True)


@pytest.mark.parametrize("C,cin", pc.SWEEP + [(32, 9)])
def test_shape_sweep(C, cin):
    case = pc.stack_case(C, cin)
    p = _planner(C, 1)
    _bind(p, case)
    p.reserve_pix_batch(3)
    _gate(f"sweep C{C} cin{cin} n3", _encode(p, case, 3), case)


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_a_row_does_not_depend_on_its_slot(n):
    # n = 1 leaves layer 3's tile half empty; 3 and 5 make tiles straddle images on every layer; rows past the case's images
    # (n = 5 of the probe's 4) must equal their source rows bit for bit
    for case, name in ((pc.stack_case(32, 9), "C32 cin9"), (pc.probe_case(0, 1), "probe L0 #1")):
        p = _planner(case["C"], 1)
        _bind(p, case)
        p.reserve_pix_batch(8)
        z = _encode(p, case, n)
        _gate(f"slots {name} n{n}", z, case)
        one = _encode(p, case, 1)
        assert torch.equal(z[0], one[0])


def test_chunk_edges():
    case = pc.stack_case(32, 9)
    small, big = _planner(32, 1), _planner(32, 1)
    _bind(small, case)
    _bind(big, case)
    small.reserve_pix_batch(4)
    big.reserve_pix_batch(16)
    for n in (4, 5, 9):
        a, b = _encode(small, case, n), _encode(big, case, n)
        _gate(f"chunk 4 n{n}", a, case)
        assert torch.equal(a, b), n  # passes of 4 against one pass
    before, bytes_before = _encode(small, case, 9), small.device_bytes
    small.reserve_pix_batch(2)  # re-reserving a smaller value changes nothing
    assert small.device_bytes == bytes_before and torch.equal(_encode(small, case, 9), before)
    small.reserve_pix_batch(16)  # a larger one grows the workspace; the bits stay
    assert small.device_bytes > bytes_before and torch.equal(_encode(small, case, 9), before)


def test_all_49_shifts():
    case = pc.shifts_case()
    assert sorted(set(case["shifts"])) == sorted(pc.ALL_SHIFTS) and len(case["shifts"]) == 49
    p = _planner(case["C"], 1)
    _bind(p, case)
    p.reserve_pix_batch(49)
    _gate("49 shifts", _encode(p, case), case)
    # shifts outside [0, 6] are clamped
    obs, shift = _inputs(case)
    wild = torch.where(shift == 0, shift - 5, torch.where(shift == 6, shift + 9, shift))
    assert torch.equal(p.encode_pix_batch(obs, wild).cpu(), p.encode_pix_batch(obs, shift).cpu())


def test_fp32_observations_fractional_negative_and_large():
    case = pc.stack_case(pc.PROBE_C, pc.PROBE_CIN, fp32=True)
    obs = case["obs"]
    assert (obs < 0).any() and (obs > 255).any() and (obs != obs.round()).any()
    p = _planner(case["C"], 1)
    _bind(p, case)
    p.reserve_pix_batch(5)
    _gate("fp32 fractional / negative / > 255", _encode(p, case), case)
    # 200 times the range: spreads past 100, expf underflows.  g leaves first order, so z is not gated; the readout is
    # (the checks of tests/test_gpu_pixel_edges.py)
    big = pc.large_case()
    ref = pc.ref_of(big)
    assert ref["spread"].max().item() > 100.0
    z = _encode(p, big).double()
    assert torch.isfinite(z).all()
    sums = z.reshape(len(z), -1, 8).sum(-1)
    assert (sums - 1.0).abs().max().item() <= 2.0 ** -22, (sums - 1.0).abs().max().item()
    grp, gg = ref["logits"].reshape(len(z), -1, 8), ref["g"][3].flatten(1).reshape(len(z), -1, 8)
    top = grp.max(-1, keepdim=True).values
    dead = (grp - top) < -(104.0 + gg + gg.max(-1, keepdim=True).values) * (1 + 2.0 ** -20)
    assert dead.any() and (z.reshape(grp.shape)[dead] == 0.0).all()
    srt = grp.sort(-1, descending=True)
    clear = (srt.values[..., 0] - srt.values[..., 1]) > 2.0 * gg.max(-1).values
    assert clear.sum().item() >= 16  # of 80 groups
    assert torch.equal(z.reshape(grp.shape).argmax(-1)[clear], srt.indices[..., 0][clear])


def test_rebinding_after_a_reservation():
    a16, b16, a3 = pc.stack_case(8, 16), pc.stack_case(8, 16, seed=1), pc.stack_case(8, 3, seed=1)
    p = _planner(8, 1)
    _bind(p, a16)
    p.reserve_pix_batch(5)
    for step, case in enumerate((a16, b16, a3, a16)):  # new weights after a training step, then cin 16 -> 3 -> 16
        _bind(p, case)
        _gate(f"re-bind step {step} cin{case['cin']}", _encode(p, case), case)


def test_refusals_leave_the_handle_usable():
    from tdmpc2_amd.native import NativeError

    case = pc.stack_case(8, 3, seed=1)
    p = _planner(8, 1)
    obs, shift = _inputs(case)
    z = torch.empty(len(obs), 16 * 8, device=_dev())
    call = lambda n, o, dt, cin: p.lib.tdmpc2_plan_encode_pix_batch(p._h, n, o.data_ptr(), dt, cin, shift.data_ptr(), z.data_ptr(), None)
    assert p.lib.tdmpc2_plan_pix_batch_reserve(p._h, 4, None) == ERR_STATE  # no encoder bound
    with pytest.raises(NativeError, match="no pixel encoder bound"):
        p.encode_pix_batch(obs, shift)
    _bind(p, case)
    assert call(len(obs), obs, 0, 3) == ERR_STATE and b"reserve" in p.lib.tdmpc2_last_error()  # bound, nothing reserved
    with pytest.raises(NativeError, match="reserve"):
        p.encode_pix_batch(obs, shift)
    with pytest.raises(ValueError):
        p.reserve_pix_batch(0)
    p.reserve_pix_batch(4)
    assert call(len(obs), obs, 0, 4) == ERR_INVALID and b"channels" in p.lib.tdmpc2_last_error()   # wrong Cin
    assert call(len(obs), obs, 0, 17) == ERR_INVALID
    assert call(len(obs), obs, 2, 3) == ERR_INVALID and b"obs_dtype" in p.lib.tdmpc2_last_error()  # wrong dtype
    assert call(0, obs, 0, 3) == ERR_INVALID
    with pytest.raises(ValueError):
        p.encode_pix_batch(obs.to(torch.float16), shift)
    with pytest.raises(ValueError):
        p.encode_pix_batch(obs[:, :2].contiguous(), shift)
    mt = _planner(8, 1, multitask=True)
    assert mt.lib.tdmpc2_plan_pix_batch_reserve(mt._h, 4, None) == ERR_UNSUPPORTED
    assert mt.lib.tdmpc2_plan_encode_pix_batch(mt._h, len(obs), obs.data_ptr(), 0, 3, shift.data_ptr(), z.data_ptr(), None) == ERR_UNSUPPORTED
    _gate("after refusals", _encode(p, case), case)  # the handle stays usable


AGREE = [("stack", 32, 9, False), ("stack", 8, 1, False), ("stack", 64, 16, False), ("stack", 40, 16, False), ("stack", 8, 3, True),
         ("probe", 0, 0, False), ("probe", 1, 1, True), ("probe", 3, 2, False), ("shifts", 0, 0, False)]


@pytest.mark.parametrize("kind,a,b,fp32", AGREE)
def test_agrees_with_encode_pix_on_the_spread_route(kind, a, b, fp32):
    case = pc.stack_case(a, b, fp32=fp32) if kind == "stack" else pc.probe_case(a, b, fp32) if kind == "probe" else pc.shifts_case()
    n = len(case["obs"])
    cus = torch.cuda.get_device_properties(_dev()).multi_processor_count
    assert n < max(cus // 2, 1)  # below pix_image_min_envs: encode_pix takes the spread route
    p = _planner(case["C"], n)
    _bind(p, case)
    p.reserve_pix_batch(n)
    name = f"{kind} {a} {b} {'fp32' if fp32 else 'u8'}"
    zb, zp = _encode(p, case), _encode(p, case, planning=True)
    _gate(f"agree batch {name}", zb, case)
    _gate(f"agree encode_pix {name}", zp, case)
    _bits[name] = bool(torch.equal(zb, zp))
    print(f"{name}: bit_equal {_bits[name]}, max |diff| {(zb - zp).abs().max().item():.3e}")
    # not asserted: bit_equal is false on most cases; test_where_the_two_routes_part below locates the difference


def _one_hot_stack(ky, kx, fp32):
    """Every layer one-hot (identity channel map): a logit IS one resampled, preprocessed input element + 0.5, read through layer
    0's tap (ky, kx) and the LAST tap of layers 1..3, which walks the final pixels over frame rows and columns 32 + k .. 56 + k: the
    half where the tap table's bilinear weights are not exactly 0 and 1, so that the form of the blend shows."""
    C, cin = pc.PROBE_C, pc.PROBE_CIN
    Ws, Bs = [], []
    for l in range(4):
        tap = (ky, kx) if l == 0 else (pc.KERNEL[l] - 1, pc.KERNEL[l] - 1)
        W, b = pc.one_hot_layer(l, cin if l == 0 else C, C, tap, False, 0.5 if l == 0 else 0.0)
        Ws.append(W)
        Bs.append(b)
    return dict(obs=pc._images(4, cin, 77, fp32), shifts=pc.SHIFTS4, Ws=Ws, Bs=Bs, C=C, cin=cin, stack=False)


def _probe_behind(L, i, l0tap):
    """pc.probe_case(L, i) (layer L >= 1 random, the others one-hot) with layer 0's one-hot tap set to l0tap."""
    base = pc.probe_case(L, i)
    W0, b0 = pc.one_hot_layer(0, base["cin"], base["C"], l0tap, bool(i % 2), 0.5)
    Ws, Bs = [W0] + [w.clone() for w in base["Ws"][1:]], [b0] + [b.clone() for b in base["Bs"][1:]]
    return dict(base, Ws=Ws, Bs=Bs)


def _agree(name, case):
    n = len(case["obs"])
    p = _planner(case["C"], n)
    _bind(p, case)
    p.reserve_pix_batch(n)
    zb, zp = _encode(p, case), _encode(p, case, planning=True)
    _gate(f"parting batch {name}", zb, case)
    _gate(f"parting encode_pix {name}", zp, case)
    return bool(torch.equal(zb, zp))


@pytest.mark.parametrize("fp32", [False, True], ids=["u8", "fp32"])
def test_where_the_two_routes_part_layer0_tap_column(fp32):
    # recorded, not asserted (it is a property of how pix_conv0 was compiled): with uint8 frames the copies of
    # pix_conv0's unrolled kx loop for kx = 0, 2, 4 blend with one fused chain, as the batch route does, and agree with it bit for
    # bit; the copies for kx = 1, 3, 5, 6 round two products on their own and differ in a few elements; with fp32 frames every
    # copy rounds all four products and every column differs
    bits = {}
    for kx in range(7):
        name = f"one-hot {'fp32' if fp32 else 'u8'} l0 tap (5, {kx})"
        bits[name] = _agree(name, _one_hot_stack(5, kx, fp32))
        print(f"{name}: bit_equal {bits[name]}")
    record({"bit_equal_to_encode_pix_by_layer0_tap": bits})


@pytest.mark.parametrize("L", [1, 2, 3])
def test_where_the_two_routes_part_layers_behind_layer0(L):
    # recorded, not asserted: layer L random behind a one-hot layer 0.  Through an even tap column (the fused copies, uint8) the
    # input elements of both routes are the same bits, and so is everything after them: layers 1..3, bias, ReLU and SimNorm repeat
    # k_pix_spread exactly.  Through an odd one the input differs and the difference is carried along.
    bits = {}
    for i in range(len(pc.PROBE_RC[L])):
        for tap in ((6, 2), (3, 4), (5, 1)):
            name = f"L{L} #{i} behind l0 tap {tap}"
            bits[name] = _agree(name, _probe_behind(L, i, tap))
            print(f"{name}: bit_equal {bits[name]}")
    record({"bit_equal_to_encode_pix_by_layer0_tap": bits})
