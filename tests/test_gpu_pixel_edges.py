"""-m gpu: pixel_kernels.cuh against the fp64 reference of tests/pixel_common.py (cases, gates and where they come from: there;
tests/test_pixel_edges.py proves them on the CPU).  Layer-under-test probes for every layer and both observation types, the
accepted shapes' edges on both routes with tiled images (a row may not depend on its slot), route agreement bit for bit, all 49
shifts on both routes, fp32 observations past expf's underflow, the workspace's last slot and re-binding.
TDMPC2_PIXEL_EDGES_JSON=<file>: the worst err / gate per item is merged into that file (profiles/pixel_edges.json)."""
import pytest
import torch

from tests import pixel_common as pc
from tests.test_pixel_edges import record

pytestmark = pytest.mark.gpu

_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_worst():
    yield
    record("mi355x_worst_err_over_gate", _worst)


def _dev():
    return torch.device("cuda", 0)


def _planner(C, max_envs):
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.native import NativePlanner

    cfg = named_config("c1")
    cfg.latent_dim, cfg.num_channels, cfg.obs = 16 * C, C, "rgb"
    return NativePlanner(cfg, cfg.iterations, _dev(), max_envs=max_envs)


def _bind(p, case):
    p.bind_pixel_encoder({k: v.to(_dev()) for k, v in pc.state_dict(case["Ws"], case["Bs"]).items()})


def _threshold():
    """The fewest images the per-image route takes (pixel_route.h: pix_image_min_envs of the device's compute units)."""
    cus = torch.cuda.get_device_properties(_dev()).multi_processor_count
    return max(cus // 2, 1)


def _encode(p, case, E=None):
    """z [E, 16 C] of the case's images tiled to E rows (image i % n in row i), as a CPU tensor."""
    n = len(case["obs"])
    idx = torch.arange(n if E is None else E) % n
    obs = case["obs"][idx].contiguous().to(_dev())
    shift = torch.tensor(case["shifts"], dtype=torch.int32)[idx].contiguous().to(_dev())
    z = p.encode_pix(obs, shift)
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
        _gate(f"probe L{L} {'fp32' if fp32 else 'u8'}", _encode(p, case), case, probe=True)


@pytest.mark.parametrize("cin", [1, 16])
@pytest.mark.parametrize("C", [8, 24, 40, 48, 64])
def test_shape_sweep_on_both_sides_of_the_threshold(C, cin):
    thr = _threshold()
    case = pc.stack_case(C, cin)
    p = _planner(C, thr)
    _bind(p, case)
    _gate(f"sweep C{C} cin{cin} E3 spread", _encode(p, case, 3), case)
    # E at the threshold: the per-image route where its LDS fits (C <= 40; C = 40 asks for 161 600 of 163 840 B), else the spread route
    _gate(f"sweep C{C} cin{cin} E at threshold {'image' if C <= 40 else 'spread'}", _encode(p, case, thr), case)


def test_routes_agree_bit_for_bit():
    thr = _threshold()
    case = pc.stack_case(32, 9)
    p = _planner(32, thr)
    _bind(p, case)
    below, at = _encode(p, case, thr - 1), _encode(p, case, thr)
    _gate("routes C32 cin9 spread", below, case)
    _gate("routes C32 cin9 image", at, case)
    assert torch.equal(below, at[:thr - 1])  # the work-item code is shared: the route changes where a layer's output lives, only


def test_all_49_shifts_on_both_routes():
    thr = _threshold()
    case = pc.shifts_case()
    assert sorted(set(case["shifts"])) == sorted(pc.ALL_SHIFTS) and len(case["shifts"]) == 49
    E = -(-max(thr, 49) // 49) * 49
    p = _planner(case["C"], E)
    _bind(p, case)
    if thr > 49:
        _gate("49 shifts spread", _encode(p, case), case)
    _gate("49 shifts image", _encode(p, case, E), case)


def test_fp32_observations_fractional_negative_and_large():
    case = pc.stack_case(pc.PROBE_C, pc.PROBE_CIN, fp32=True)
    obs = case["obs"]
    assert (obs < 0).any() and (obs > 255).any() and (obs != obs.round()).any()
    p = _planner(case["C"], 5)
    _bind(p, case)
    _gate("fp32 fractional / negative / > 255", _encode(p, case), case)
    # 200 times the range: spreads past 100, expf underflows.  g leaves first order, so z is not gated; the readout is.
    big = pc.large_case()
    ref = pc.ref_of(big)
    assert ref["spread"].max().item() > 100.0
    z = _encode(p, big).double()
    assert torch.isfinite(z).all()
    sums = z.reshape(len(z), -1, 8).sum(-1)
    assert (sums - 1.0).abs().max().item() <= 2.0 ** -22, (sums - 1.0).abs().max().item()
    grp, gg = ref["logits"].reshape(len(z), -1, 8), ref["g"][3].flatten(1).reshape(len(z), -1, 8)
    top = grp.max(-1, keepdim=True).values
    # below e^-104 < 2^-149 nothing is representable: wherever the reference's logit is that far down even after both gates, an exact 0
    dead = (grp - top) < -(104.0 + gg + gg.max(-1, keepdim=True).values) * (1 + 2.0 ** -20)
    assert dead.any() and (z.reshape(grp.shape)[dead] == 0.0).all()
    # the argmax, wherever the reference's runner-up is further away than the two logits' gates
    srt = grp.sort(-1, descending=True)
    clear = (srt.values[..., 0] - srt.values[..., 1]) > 2.0 * gg.max(-1).values
    assert clear.sum().item() >= 16  # of 80 groups
    assert torch.equal(z.reshape(grp.shape).argmax(-1)[clear], srt.indices[..., 0][clear])


def test_workspace_last_slot():
    case = pc.stack_case(64, 16)
    E = 3
    p = _planner(64, E)  # max_envs == E: image E - 1 owns the workspace's last slice
    _bind(p, case)
    one = _encode(p, dict(case, obs=case["obs"][:1], shifts=case["shifts"][:1]))
    z = _encode(p, case, E)
    _gate("workspace edge C64 E == max_envs", z, case)
    assert torch.equal(z[0], one[0])


def test_rebinding_weights_and_input_channels():
    a16, b16, a3 = pc.stack_case(8, 16), pc.stack_case(8, 16, seed=1), pc.stack_case(8, 3, seed=1)
    p = _planner(8, 5)
    for step, case in enumerate((a16, b16, a3, a16)):  # new weights after a training step, then cin 16 -> 3 -> 16
        _bind(p, case)
        z = _encode(p, case)
        _gate(f"re-bind step {step} cin{case['cin']}", z, case)
        fresh = _planner(8, 5)
        _bind(fresh, case)
        assert torch.equal(z, _encode(fresh, case)), step
