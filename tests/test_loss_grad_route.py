"""CPU: tdmpc2_amd/csrc/loss_grad_route.h compiled with the host compiler (tests/loss_grad_common.py: SHIM): the decoded grids cover
every row and every output element exactly once at the case table, the workspace has the published size and every float of it is
written once, the step sums run in the published order, and offsets past 2^32 stay exact.  The same walk runs as a stand-alone
program under AddressSanitizer and UBSan."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

from tests import loss_grad_common as lc

CONS, REW, Q, TERM = range(4)  # LS_K_*


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    return lc.build_route(tmp_path_factory.mktemp("loss_route"))


def test_constants_and_descriptor(route):
    from tdmpc2_amd import native

    out = (C.c_int32 * 12)()
    route.constants(out)
    k = dict(zip(lc.CONSTANT_KEYS, out))
    assert (k["THREADS"], k["WAVES"], k["ROWS"], k["ELEMS"], k["MAXT"]) == (256, 4, 4, 1024, 8)
    assert (k["CONS"], k["REW"], k["TERM"], k["Q0"], k["KINDS"]) == (0, 1, 2, 3, 4)
    assert k["DESC_BYTES"] == 56 == C.sizeof(native.LossDesc) == C.sizeof(lc.Desc) and k["GRID_BYTES"] == 40
    assert [f[0] for f in native.LossDesc._fields_] == [f[0] for f in lc.Desc._fields_]


def _grid(route, d, backward, want):
    out = (C.c_uint64 * 5)()
    route.grid(C.byref(d), backward, want, out)
    return list(out)


@pytest.mark.parametrize("name", [c["name"] for c in lc.CASE_LIST] + ["fixture"])
def test_exact_cover_and_workspace(route, name):
    case = lc.FIXTURE_CASE if name == "fixture" else lc.CASES[name]
    d = lc.desc_of(case)
    T, B, L, NB, Qn, ep = case["T"], case["B"], case["L"], case["NB"], case["Q"], case["episodic"]
    assert route.check(C.byref(d)) == 0
    assert route.ws_floats(C.byref(d)) == (3 + Qn) * T * B
    up = lambda a, b: -(-a // b)  # noqa: E731
    fwd = [up(T * B, 4), up(T * B, 4), up(Qn * T * B, 4), up(T * B, 256) if ep else 0]
    assert _grid(route, d, 0, 0) == [0] + list(itertools.accumulate(fwd))
    assert route.cover(C.byref(d), 0, 0) == 0
    bwd = [up(T * B * L, 1024), up(T * B, 4), up(Qn * T * B, 4), up(T * B, 256) if ep else 0]
    for want in range(1, 16):
        if (want & 8) and not ep:
            continue
        counts = [n if (want >> k) & 1 else 0 for k, n in enumerate(bwd)]
        assert _grid(route, d, 1, want) == [0] + list(itertools.accumulate(counts)), want
        assert route.cover(C.byref(d), 1, want) == 0, want


def test_steps_targets_and_workspace_slots(route):
    case = lc.CASES["flag"]
    d = lc.desc_of(case)
    T, B, L, Qn = case["T"], case["B"], case["L"], case["Q"]
    step, target = C.c_int32(), C.c_uint64()
    for q, t, b in itertools.product(range(Qn), range(T), (0, 1, B - 1)):
        row = (q * T + t) * B + b
        route.unit_info(C.byref(d), Q, 1, row, C.byref(step), C.byref(target))
        assert (step.value, target.value) == (t, t * B + b)
        assert route.ws_index(C.byref(d), 3, row) == (3 + q) * T * B + t * B + b  # slot LS_Q0 + q of row t * B + b
    for t, b, col in itertools.product(range(T), (0, B - 1), (0, L - 1)):
        route.unit_info(C.byref(d), CONS, 1, (t * B + b) * L + col, C.byref(step), C.byref(target))
        assert step.value == t
        route.unit_info(C.byref(d), REW, 0, t * B + b, C.byref(step), C.byref(target))
        assert (step.value, target.value) == (t, t * B + b)


def test_per_step_constants_are_rounded_once(route):
    case = lc.CASES["five"]
    h = lc.hyper(case["NB"])
    d = lc.desc_of(case, h)
    T, B, L, Qn = case["T"], case["B"], case["L"], case["Q"]
    for t in range(T):
        w = h["rho"] ** t
        assert route.rho_pow(C.byref(d), t) == np.float32(w)
        assert route.coef(C.byref(d), CONS, t) == np.float32(h["consistency_coef"] * 2.0 * w / (T * B * L))
        assert route.coef(C.byref(d), REW, t) == np.float32(h["reward_coef"] * w / (T * B))
        assert route.coef(C.byref(d), Q, t) == np.float32(h["value_coef"] * w / (T * Qn * B))
        assert route.coef(C.byref(d), TERM, t) == np.float32(h["termination_coef"] / (T * B))


def test_summation_order(route):
    rng = np.random.default_rng(5)
    for n in (1, 2, 33, 255, 256, 257, 1000):
        src = (np.exp(rng.uniform(-8, 8, n)) * rng.choice((-1.0, 1.0), n)).astype(np.float32)
        got = route.ordered_sum(src.ctypes.data_as(C.POINTER(C.c_float)), n)
        assert np.float32(got).tobytes() == lc.ordered_sum_model(src).tobytes(), n
    # the order matters: a plain left-to-right sum of the same terms differs somewhere
    src = (np.exp(rng.uniform(-8, 8, 1000))).astype(np.float32)
    serial = np.float32(0)
    for v in src:
        serial = np.float32(serial + v)
    assert lc.ordered_sum_model(src).tobytes() != serial.tobytes()


def test_refusals_of_the_descriptor(route):
    case = lc.CASES["flag"]
    for over, code in ((dict(steps=0), 1), (dict(steps=9), 1), (dict(batch=0), 2), (dict(latent_dim=0), 2), (dict(num_q=0), 2),
                       (dict(num_bins=1), 3), (dict(num_bins=0), 3), (dict(steps=8), 0)):
        d = lc.desc_of(case, **over)
        assert route.check(C.byref(d)) == code, over


def test_offsets_past_2_32(route):
    big = lc.desc_of(dict(T=8, B=1 << 24, L=512, NB=101, Q=5, episodic=True))
    n = 8 * (1 << 24) * 512
    g = _grid(route, big, 1, 15)
    assert g[1] == n // 1024 and g[4] < 1 << 31
    kind, local = C.c_int32(), C.c_uint64()
    route.decode(C.byref(big), 1, 15, g[1] - 1, C.byref(kind), C.byref(local))
    assert kind.value == CONS and route.elem(local.value, 255, 3) == n - 1 > 1 << 32
    route.decode(C.byref(big), 1, 15, g[1], C.byref(kind), C.byref(local))
    assert (kind.value, local.value) == (REW, 0)
    assert route.ws_index(C.byref(big), 3 + 4, 8 * (1 << 24) - 1) == route.ws_floats(C.byref(big)) - 1 == 8 * 8 * (1 << 24) - 1
    huge = lc.desc_of(dict(T=8, B=(1 << 31) - 1, L=1, NB=2, Q=1 << 20, episodic=False))
    assert _grid(route, huge, 0, 0)[4] > 1 << 31  # what the entry points refuse as UNSUPPORTED


@pytest.mark.parametrize("sanitize", [False, True])
def test_walk_as_a_program(tmp_path, sanitize):
    exe = lc.build_walk(tmp_path, sanitize=sanitize)
    res = subprocess.run([exe, lc.walk_input(str(tmp_path / "cases.bin"))], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "bad 0" in res.stdout and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
