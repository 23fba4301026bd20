"""CPU: the harness of tests/test_gpu_pixel_edges.py proved before the kernel meets it (tests/pixel_common.py).  The fp64
reference equals tdmpc2_amd.layers.conv in fp64 on table-resampled input and agrees with the reference project's recorded
output; the pinned module's own fp32 stays inside every gate on every case (worst err / gate: profiles/pixel_edges.json,
written when TDMPC2_PIXEL_EDGES_JSON names a file); the probes read every row and column of the layer under test; the
conditioned weights move SimNorm off its uniform point; and seven mistakes made IN THE REFERENCE each leave the gate of their
case by at least a factor of 2."""
import json
import os

import numpy as np
import pytest
import torch

from tests import pixel_common as pc

MUTATION_FACTOR = 2.0


def record(section, worst):
    """Merge {item: worst err / gate} into the JSON file TDMPC2_PIXEL_EDGES_JSON names (no-op without it)."""
    path = os.environ.get("TDMPC2_PIXEL_EDGES_JSON")
    if not path:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc["gate"] = ("z: 2 z (g + sum_group z g) + 4 * 2^-22;  g_l = 2^-24 (K + 2) (|W| * |x| + |b|) + |W| * g_(l-1);  "
                   "g_x = 2^-24 (7 S / 255 + 0.5);  "
                   "stack cases: min(that, max(1e-5, 4 |module fp32 - fp64|))  (tests/pixel_common.py)")
    doc.setdefault(section, {}).update({k: float(v) for k, v in worst.items()})
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def cases():
    return pc.gated_cases()


def test_reference_equals_the_module_in_fp64(cases):
    for name in ("probe L0 #1 u8", "probe L2 #3 fp32", "stack C24 cin16", "stack C8 cin3 fp32", "shifts"):
        c = cases[name]
        ref = pc.ref_of(c)
        acts, z = pc.module_tail_fp64(c)
        for l in range(4):
            assert (acts[l] - ref["act"][l]).abs().max().item() <= 1e-12 * max(1.0, ref["act"][l].abs().max().item()), (name, l)
        assert (z - ref["z"]).abs().max().item() <= 1e-13, name


def test_reference_agrees_with_the_recorded_reference_output():
    from oracle import make_golden_host as mg
    from tests.helpers import GOLDEN_DIR

    g = np.load(f"{GOLDEN_DIR}/{mg.PIXEL_FILE}")
    st = {k: torch.as_tensor(np.asarray(v)).float() for k, v in mg.conv_state(g).items()}
    torch.manual_seed(mg.CONV_SEED)
    shift = torch.randint(0, 7, size=(2, 1, 1, 2), dtype=torch.float32).view(2, 2).int().tolist()  # the reference's draw
    c = dict(obs=mg.pixel_input(), shifts=shift, Ws=[st[f"{i}.weight"] for i in (2, 4, 6, 8)], Bs=[st[f"{i}.bias"] for i in (2, 4, 6, 8)])
    ref = pc.reference(c["obs"], c["shifts"], c["Ws"], c["Bs"])
    # default-init weights at C = 32: the composed worst-case gate is loose here (g ~ 0.08), so the recorded fp32 output is also
    # held to the 1e-5 that tests/test_gpu_pixel_encoder.py allows the kernel on this fixture
    assert pc.worst_ratio(g["conv"], ref) <= 1.0
    assert np.abs(g["conv"] - ref["z"].numpy()).max() <= 1e-5


def test_module_fp32_stays_inside_every_gate(cases):
    worst = {}
    for name, c in cases.items():
        ref = pc.ref_of(c)
        if not c["stack"]:
            assert ref["g"][3].max().item() <= pc.G_MAX, (name, ref["g"][3].max().item())
        worst[name] = pc.worst_ratio(pc.module_fp32(c).numpy(), ref)
    print("module fp32, worst err / gate:", max(worst.values()), max(worst, key=worst.get))
    record("cpu_module_fp32", worst)
    bad = {k: v for k, v in worst.items() if v > 1.0}
    assert not bad, bad


def test_readout_term_is_what_torch_fp32_softmax_shows(cases):
    """READOUT_R is the reference side's own figure: torch's fp32 softmax against fp64 on the fp32-rounded fp64 logits."""
    r = 0.0
    for c in cases.values():
        y32 = pc.ref_of(c)["logits"].float()
        r = max(r, (pc.simnorm64(y32.double()) - pc.simnorm64(y32).double()).abs().max().item())
    print("torch fp32 softmax vs fp64:", r)
    assert r <= pc.READOUT_R <= 4.0 * r, r


def test_conditioned_weights_leave_the_uniform_point(cases):
    for name, c in cases.items():
        if name.startswith("stack") or name == "shifts":
            s = pc.ref_of(c)["spread"]
            assert s.median().item() >= 1.0 and s.max().item() <= 30.0, (name, s.median().item(), s.max().item())
    big = pc.reference(**{k: pc.large_case()[k] for k in ("obs", "shifts", "Ws", "Bs")})
    assert big["spread"].max().item() > 100.0 and (big["z"] < 2.0 ** -150).any()


def test_probes_read_every_row_and_column_of_the_layer_under_test():
    for L in range(3):
        side, step = pc.OUT[L], pc.PROBE_STEP[L]
        rows = {r + step * o for r, _ in pc.PROBE_RC[L] for o in range(4)}
        cols = {c + step * o for _, c in pc.PROBE_RC[L] for o in range(4)}
        assert rows == cols == set(range(side)), L
        pix = {(r + step * oy, c + step * ox) for r, c in pc.PROBE_RC[L] for oy in range(4) for ox in range(4)}
        assert {(0, 0), (0, side - 1), (side - 1, 0), (side - 1, side - 1)} <= pix, L
    for L in range(4):
        assert {bool(i % 2) for i in range(len(pc.PROBE_RC[L]))} == {False, True}  # the identity and the twisted channel map
        for i, (r, c) in enumerate(pc.PROBE_RC[L]):
            case = pc.probe_case(L, i)
            ref = pc.ref_of(case)
            if L < 3:
                # the logits ARE layer L's output pixels (post-ReLU), read at stride PROBE_STEP from (r, c), channels permuted
                step, p = pc.PROBE_STEP[L], pc.perm(case["C"], bool(i % 2))
                src = ref["act"][L][:, :, r:r + 3 * step + 1:step, c:c + 3 * step + 1:step]
                for _ in range(L + 1, 4):
                    src = src[:, [p.index(co) for co in range(case["C"])]]
                assert torch.equal(ref["act"][3], src), (L, i)
                assert (ref["act"][3] > 0).float().mean().item() >= 0.9, (L, i)  # ReLU hides little of it


def _leaves(case, mutated):
    return ((mutated["z"] - pc.ref_of(case)["z"]).abs() / pc.ref_of(case)["gz"]).max().item()


def _mutated(case, mut=None, **over):
    c = dict(case, **over)
    return pc.reference(c["obs"], c["shifts"], c["Ws"], c["Bs"], mut)


def test_mutations_of_the_reference_leave_their_gates():
    out = {}
    # the corner output pixel (28, 28) of layer 0, one channel, replaced by its neighbour: the L0 probe that reads (28, 28)
    c = pc.probe_case(0, 7)
    out["corner (28, 28) of layer 0, one channel"] = _leaves(c, _mutated(c, {"corner0": 5}))
    # tap (6, 6) of layer 0 dropped for one output channel
    W0 = c["Ws"][0].clone()
    W0[2, :, 6, 6] = 0.0
    out["tap (6, 6) of layer 0, one channel"] = _leaves(c, _mutated(c, Ws=[W0] + c["Ws"][1:]))
    # dx and dy swapped on images with dx != dy
    c = pc.shifts_case()
    assert any(dx != dy for dx, dy in c["shifts"])
    out["dx and dy swapped"] = _leaves(c, _mutated(c, shifts=[(dy, dx) for dx, dy in c["shifts"]]))
    # the last input channel ignored at cin = 16
    c = pc.stack_case(8, 16)
    W0 = c["Ws"][0].clone()
    W0[:, 15] = 0.0
    out["last input channel ignored at cin 16"] = _leaves(c, _mutated(c, Ws=[W0] + c["Ws"][1:]))
    # two output channels of layer 2 swapped
    c = pc.probe_case(2, 1)
    W2, b2 = c["Ws"][2].clone(), c["Bs"][2].clone()
    W2[[3, 4]], b2[[3, 4]] = W2[[4, 3]], b2[[4, 3]]
    out["two output channels of layer 2 swapped"] = _leaves(c, _mutated(c, Ws=c["Ws"][:2] + [W2] + c["Ws"][3:], Bs=c["Bs"][:2] + [b2] + c["Bs"][3:]))
    # SimNorm groups offset by 4 features; - 0.5 omitted
    c = pc.stack_case(24, 1)
    out["SimNorm groups offset by 4"] = _leaves(c, _mutated(c, {"group_off": 4}))
    out["- 0.5 omitted"] = _leaves(c, _mutated(c, {"no_half": True}))
    print({k: round(v, 1) for k, v in out.items()})
    weak = {k: v for k, v in out.items() if v < MUTATION_FACTOR}
    assert not weak, weak
