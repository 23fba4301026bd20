"""CPU: tdmpc2_amd/csrc/pi_grad_route.h compiled with the host compiler (tests/pi_grad_common.py: SHIM): the grids cover every row and
every output element exactly once for every subset of NULL outputs, at B T of 1, 27 and 297 and at the case table; the host
constants are the published ones; the sums of the loss run in the published order, bit for bit against numpy; offsets past 2^32 stay
exact.  The same walk runs as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import pi_grad_common as pc

FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    return pc.build_route(tmp_path_factory.mktemp("pi_grad_route"))


def _ptr(a):
    return a.ctypes.data_as(FP)


def test_constants_and_descriptor(route):
    from tdmpc2_amd import native

    out = (C.c_int32 * 10)()
    route.constants(out)
    k = dict(zip(pc.CONSTANT_KEYS, out))
    assert (k["THREADS"], k["ROWS"], k["HEAD_LANES"], k["HEAD_ROWS"]) == (256, 4, 8, 32) and k["HEAD_LANES"] * k["HEAD_ROWS"] == k["THREADS"]
    assert (k["MAXT"], k["MAXA"], k["MAXBINS"], k["KINDS"]) == (16, 64, 4096, 2)
    assert k["DESC_BYTES"] == 44 == C.sizeof(native.PiGradDesc) == C.sizeof(pc.Desc) and k["GRID_BYTES"] == 24
    assert [f[0] for f in native.PiGradDesc._fields_] == [f[0] for f in pc.Desc._fields_]


def test_descriptor_refusals(route):
    case = pc.CASES["small"]
    assert route.check(C.byref(pc.desc_of(case))) == 0
    for over, code in ((dict(steps=0), 1), (dict(steps=17), 1), (dict(steps=16), 0), (dict(batch=0), 2), (dict(action_dim=0), 3),
                       (dict(action_dim=65), 3), (dict(action_dim=64), 0), (dict(num_bins=1), 4), (dict(num_bins=4097), 4),
                       (dict(num_bins=2), 0)):
        assert route.check(C.byref(pc.desc_of(case, **over))) == code, over


@pytest.mark.parametrize("T,B", pc.ROUTE_SIZES)
@pytest.mark.parametrize("A,NB", ((1, 2), (6, 101), (17, 65), (64, 129)))
def test_exact_cover_at_the_sizes(route, T, B, A, NB):
    d = pc.desc_of(dict(T=T, B=B, A=A, NB=NB))
    up = lambda a, b: -(-a // b)  # noqa: E731
    assert route.head_grid(C.byref(d)) == up(T * B, 32) and route.value_grid(C.byref(d)) == up(T * B, 4)
    for want, counts in ((1, (up(2 * T * B, 4), 0)), (2, (0, up(T * B, 256))), (3, (up(2 * T * B, 4), up(T * B, 256)))):
        out = (C.c_uint64 * 3)()
        route.bwd_grid(C.byref(d), want, out)
        assert list(out) == [0, counts[0], counts[0] + counts[1]], want
    assert route.cover(C.byref(d)) == 0  # every launch, every subset of loss_backward's outputs


@pytest.mark.parametrize("name", [c["name"] for c in pc.CASE_LIST] + list(pc.FIXTURE_CASES))
def test_exact_cover_at_the_case_table(route, name):
    case = pc.CASES.get(name) or pc.FIXTURE_CASES[name]
    assert route.cover(C.byref(pc.desc_of(case))) == 0


def test_steps_and_mask_rows(route):
    d = pc.desc_of(pc.CASES["odd"])  # T 9, B 33
    for unit, step in ((0, 0), (32, 0), (33, 1), (296, 8), (297, 0), (297 + 34, 1), (2 * 297 - 1, 8)):
        assert route.step_of(C.byref(d), unit) == step, unit
    assert [route.mask_row(C.byref(d), r) for r in (0, 32, 33, 296)] == [0, 32, 0, 32]


def test_offsets_past_2_32(route):
    d = pc.desc_of(dict(T=16, B=1 << 29, A=64, NB=101))  # 2^33 rows
    TB = 1 << 33
    assert route.head_grid(C.byref(d)) == TB // 32 and route.value_grid(C.byref(d)) == TB // 4
    out = (C.c_uint64 * 3)()
    route.bwd_grid(C.byref(d), 3, out)
    assert list(out) == [0, 2 * TB // 4, 2 * TB // 4 + TB // 256]
    assert route.step_of(C.byref(d), 2 * TB - 1) == 15 and route.step_of(C.byref(d), TB) == 0 and route.step_of(C.byref(d), TB - 1) == 15
    assert route.mask_row(C.byref(d), TB - 1) == (1 << 29) - 1 and route.mask_row(C.byref(d), 1 << 32) == 0


def test_host_constants(route):
    h = pc.hyper()
    for case in (pc.CASES["small"], pc.CASES["deep"]):
        d = pc.desc_of(case, h)
        T, B, NB = case["T"], case["B"], case["NB"]
        for t in range(T):
            w = h["rho"] ** t
            assert route.rho_pow(C.byref(d), t) == np.float32(w)
            assert route.coef_q(C.byref(d), t) == np.float32(-w / (2.0 * T * B))
            assert route.coef_se(C.byref(d), t) == np.float32(-h["entropy_coef"] * w / (T * B))
        bins = np.asarray([route.bin(C.byref(d), k) for k in range(NB)], np.float32)
        assert bins.tobytes() == pc.bins_of(h, NB, np.float32).tobytes()
        assert bins[0] == -10.0 and bins[-1] == 10.0 and (np.diff(bins) > 0).all()
    import torch

    # the table the planner's handle builds (torch.linspace in fp32, float step) to an ulp of the largest bin
    assert np.abs(pc.bins_of(h, 101, np.float32) - torch.linspace(-10, 10, 101).numpy()).max() <= 2.0 ** -20


@pytest.mark.parametrize("n", (1, 5, 255, 256, 257, 297, 1000, 4097))
def test_the_ordered_sum_matches_numpy_bit_for_bit(route, n):
    src = (np.random.default_rng(n).standard_normal(n) * 100).astype(np.float32)
    got = np.float32(route.ordered_sum(_ptr(src), n))
    assert got.tobytes() == np.float32(pc.ordered_sum_model(src)).tobytes()


@pytest.mark.parametrize("T,B", ((1, 1), (3, 9), (9, 33), (16, 5), (2, 300)))
@pytest.mark.parametrize("scale", pc.SCALES)
def test_the_loss_matches_numpy_bit_for_bit(route, T, B, scale):
    h = pc.hyper()
    rng = np.random.default_rng(T * 1000 + B)
    q = (np.sinh(rng.uniform(-9, 9, (T, B)))).astype(np.float32)
    ent, se = (rng.uniform(5, 90, (T, B)).astype(np.float32) for _ in range(2))
    d = pc.desc_of(dict(T=T, B=B, A=6, NB=101), h)
    losses, sm = np.zeros(3, np.float32), np.zeros(T, np.float32)
    route.loss_serial(C.byref(d), _ptr(q), _ptr(ent), _ptr(se), C.c_float(scale), _ptr(losses), _ptr(sm))
    want_l, want_sm = pc.loss_model(q, ent, se, h, scale)
    assert losses.tobytes() == want_l.tobytes() and sm.tobytes() == want_sm.tobytes()
    ref = -(h["entropy_coef"] * se.astype(np.float64) + q.astype(np.float64) / scale).mean(1)
    assert abs(losses[0] - (ref * h["rho"] ** np.arange(T)).mean()) <= 1e-5 * np.abs(ref).max()


def test_the_walk_as_a_program_under_the_sanitizers(tmp_path):
    exe = pc.build_walk(tmp_path, sanitize=True)
    res = subprocess.run([exe, pc.walk_input(str(tmp_path / "cases.bin"))], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "bad 0" in res.stdout and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
