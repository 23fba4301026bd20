"""CPU test of the layered family's launch routes (tdmpc2_amd/csrc/layer_route.h, compiled with g++: tests/layer_route_model.py).

* the route table: for the benched geometries, the kernel instance and grid of every kind of layer launch -- values read off a GPU
  kernel trace (rocprofv3 --kernel-trace of one planning call per geometry) of the library before the routes moved into layer_route.h
  (the ordered launch lists: profiles/r7a_layer_route_launches.txt);
* the knob table: one entry per knob, every default inside its accepted range, and the values the measurement records used accepted.
(The dispatcher model of the launches that wait: tests/test_tile_order.py.)"""
import ctypes

import pytest

from tdmpc2_amd.config import named_config
from tests import layer_route_model as lrm


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return lrm.build(tmp_path_factory.mktemp("layer_route"))


# (config, E) -> layer label (layer_route_model.plan_launches) -> [(kernel, grid in workgroups, workgroup size)] of its first launch:
# the GEMM, and m_rows behind g_gemm_m unless every problem's epilogue ran inside the GEMM.  <net>.l<i>: layer i of the net on the
# per-layer tiles, "@t0" the first layer at t = 0 (the action columns only); "a|b": a few-row launch of two problems; pi_rows: the
# policy-prior rows (a pass of their own, or -- one few-row plan -- inside iteration 0's stage).
TABLE = {
    ("c3", 1): {
        "pi.l0": [("g_gemm_m", 256, 512), ("m_rows<256>", 512, 256)],
        "pi.l2": [("g_gemm_m", 64, 512), ("m_rows<256>", 128, 256)],
        "pi_rows.l0": [("g_gemm_m", 88, 512), ("m_rows<256>", 24, 256)],
        "pi_rows.l1": [("g_gemm_m", 112, 512), ("m_rows<256>", 24, 256)],
        "pi_rows.l2": [("g_gemm_m", 16, 512), ("m_rows<256>", 6, 256)],
        "dyn|rew.l0@t0": [("g_gemm_m", 64, 512)],
        "dyn|rew.l0": [("g_gemm_m", 224, 512), ("m_rows<256>", 1024, 256)],
        "dyn|rew.l1": [("g_gemm_m", 224, 512), ("m_rows<256>", 1024, 256)],
        "dyn.l2|rew.l2": [("g_gemm_m", 256, 512), ("m_rows<256>", 640, 256)],
        "q0|q1.l2": [("g_gemm_m", 128, 512), ("m_rows<256>", 128, 256)],
    },
    ("c3", 4): {
        "pi.l0": [("g_gemm_m", 256, 512), ("m_rows<512>", 256, 512)],
        "pi.l2": [("g_gemm_m", 256, 512), ("m_rows<512>", 256, 512)],
        "pi_rows.l0": [("g_gemm_m", 88, 512), ("m_rows<256>", 128, 256)],
        "pi_rows.l1": [("g_gemm_m", 112, 512), ("m_rows<256>", 128, 256)],
        "pi_rows.l2": [("g_gemm_m", 16, 512), ("m_rows<256>", 32, 256)],
        "dyn|rew.l0@t0": [("g_gemm_m", 256, 512)],
        "dyn|rew.l0": [("g_gemm_m", 256, 512)],
        "dyn|rew.l1": [("g_gemm_m", 256, 512)],
        "dyn.l2|rew.l2": [("g_gemm_m", 384, 512), ("m_rows<512>", 512, 512)],
        "q0|q1.l2": [("g_gemm_m", 256, 512), ("m_rows<512>", 256, 512)],
    },
    ("c3", 30): {
        "dyn.l0@t0": [("g_gemm_w<1, 0>", 448, 512)],
        "dyn.l0": [("g_gemm_w<1, 0>", 448, 512)],
        "dyn.l1": [("g_gemm_w<1, 0>", 448, 512)],
        "dyn.l2": [("g_gemm_s<2, 4, 2, 2, 0>", 360, 256)],
        "rew.l2": [("g_gemm_s<1, 1, 4, 3, 0>", 480, 256)],
        "q0.l2": [("g_gemm_s<1, 1, 4, 3, 0>", 480, 256)],
        "q1.l2": [("g_gemm_s<1, 1, 4, 0, 0>", 480, 256)],
        "pi.l0": [("g_gemm_w<1, 0>", 448, 512)],
        "pi.l2": [("g_gemm_s<1, 1, 4, 0, 0>", 480, 256)],
        "pi_rows.l0": [("g_gemm_m", 256, 512), ("m_rows<256>", 960, 256)],
        "pi_rows.l1": [("g_gemm_m", 256, 512), ("m_rows<256>", 960, 256)],
        "pi_rows.l2": [("g_gemm_m", 128, 512), ("m_rows<256>", 240, 256)],
    },
    ("c4", 1): {
        "pi.l0": [("g_gemm_m", 256, 512), ("m_rows<512>", 128, 512)],
        "pi.l2": [("g_gemm_m", 128, 512), ("m_rows<512>", 128, 512)],
        "pi_rows.l0": [("g_gemm_m", 256, 512), ("m_rows<256>", 24, 256)],
        "pi_rows.l1": [("g_gemm_m", 256, 512), ("m_rows<256>", 24, 256)],
        "pi_rows.l2": [("g_gemm_m", 16, 512), ("m_rows<256>", 6, 256)],
        "dyn|rew.l0@t0": [("g_gemm_m", 256, 512)],
        "dyn|rew.l0": [("g_gemm_m", 256, 512)],
        "dyn|rew.l1": [("g_gemm_m", 256, 512)],
        "dyn.l2|rew.l2": [("g_gemm_m", 256, 512), ("m_rows<512>", 256, 512)],
        "q0|q1.l2": [("g_gemm_m", 256, 512), ("m_rows<512>", 128, 512)],
    },
    ("c4", 2): {
        "dyn.l0@t0": [("g_gemm_s<2, 4, 2, 1, 0>", 256, 256)],
        "dyn.l0": [("g_gemm_w<1, 1>", 256, 512)],
        "dyn.l1": [("g_gemm_w<1, 1>", 256, 512)],
        "dyn.l2": [("g_gemm_w<2, 1>", 256, 512)],
        "rew.l2": [("g_gemm_s<1, 1, 4, 0, 0>", 64, 256)],
        "q0.l2": [("g_gemm_s<1, 1, 4, 0, 0>", 64, 256)],
        "q1.l2": [("g_gemm_s<1, 1, 4, 0, 0>", 64, 256)],
        "pi.l0": [("g_gemm_w<1, 1>", 256, 512)],
        "pi.l2": [("g_gemm_s<1, 1, 4, 0, 0>", 64, 256)],
        "pi_rows.l0": [("g_gemm_m", 256, 512), ("m_rows<256>", 64, 256)],
        "pi_rows.l1": [("g_gemm_m", 256, 512), ("m_rows<256>", 64, 256)],
        "pi_rows.l2": [("g_gemm_m", 16, 512), ("m_rows<256>", 16, 256)],
    },
    ("c4", 8): {
        "dyn.l0@t0": [("g_gemm_w<1, 0>", 512, 512)],
        "dyn.l0": [("g_gemm_w<1, 0>", 512, 512)],
        "dyn.l1": [("g_gemm_w<1, 0>", 512, 512)],
        "dyn.l2": [("g_gemm_w<2, 0>", 192, 512)],
        "rew.l2": [("g_gemm_s<1, 1, 4, 3, 0>", 256, 256)],
        "q0.l2": [("g_gemm_s<1, 1, 4, 3, 0>", 256, 256)],
        "q1.l2": [("g_gemm_s<1, 1, 4, 0, 0>", 256, 256)],
        "pi.l0": [("g_gemm_w<1, 0>", 512, 512)],
        "pi.l2": [("g_gemm_s<1, 1, 4, 0, 0>", 256, 256)],
        "pi_rows.l0": [("g_gemm_m", 256, 512), ("m_rows<256>", 256, 256)],
        "pi_rows.l1": [("g_gemm_m", 256, 512), ("m_rows<256>", 256, 256)],
        "pi_rows.l2": [("g_gemm_m", 32, 512), ("m_rows<256>", 64, 256)],
    },
    ("c4", 64): {
        "dyn.l0@t0": [("g_gemm_w<1, 0>", 4096, 512)],
        "dyn.l0": [("g_gemm_w<1, 0>", 4096, 512)],
        "dyn.l1": [("g_gemm_w<1, 0>", 4096, 512)],
        "dyn.l2": [("g_gemm_w<2, 0>", 1536, 512)],
        "rew.l2": [("g_gemm_s<1, 4, 4, 0, 0>", 512, 256)],
        "q0.l2": [("g_gemm_s<1, 4, 4, 0, 0>", 512, 256)],
        "q1.l2": [("g_gemm_s<1, 4, 4, 0, 0>", 512, 256)],
        "pi.l0": [("g_gemm_w<1, 0>", 4096, 512)],
        "pi.l2": [("g_gemm_s<1, 4, 4, 0, 0>", 512, 256)],
        "pi_rows.l0": [("g_gemm_s<2, 4, 2, 1, 0>", 256, 256)],
        "pi_rows.l1": [("g_gemm_s<2, 4, 2, 1, 0>", 256, 256)],
        "pi_rows.l2": [("g_gemm_s<1, 1, 4, 0, 0>", 64, 256)],
    },
}


@pytest.mark.parametrize("model,E", sorted(TABLE))
def test_the_routes_of_the_benched_geometries_are_the_traced_ones(lib, model, E):
    got = {}
    for label, kernel, grid, wg in lrm.kernel_list(lrm.plan_launches(lib, named_config(model), E)):
        launches = got.setdefault(label, [])
        if all(k.split("<")[0] != kernel.split("<")[0] for k, _, _ in launches):  # the first launch of the layer
            launches.append((kernel, grid, wg))
    assert {k: got.get(k) for k in TABLE[model, E]} == TABLE[model, E]


def _knobs(lib):
    spec = (ctypes.c_int * 3)()
    res = []
    for i in range(lib.knob_count()):
        lib.knob_spec(i, spec)
        res.append(tuple(spec))
    return res


def test_the_knob_table(lib):
    from tdmpc2_amd.native import EXPERT_KNOBS
    knobs = _knobs(lib)
    assert len(knobs) == len(EXPERT_KNOBS)  # LK_COUNT entries (the names: tests/test_abi.py)
    for name, (d, lo, hi) in zip(EXPERT_KNOBS, knobs):
        assert lo <= d <= hi, name
    k = dict(zip(EXPERT_KNOBS, knobs))
    # the values the code gives a meaning to, and those of the A/Bs on record (profiles/README.md, tools/)
    used = {"GEMM_W256_MIN": (-1, -100, 0, 128, 192, 100000), "GEMM_W_XCD_ROWS": (-1, 0, 1, 2, 4), "GEMM_XCD_ROWS": (-1, 0, 1, 2, 4),
            "GEMM_COL_PAD": (-1, 0, 1), "KSPLIT_AUTO_MIN": (-1, 0, 64), "GEMM_FILL_HEAD_PERMILLE": (200, 400, 750, 1000),
            "GEMM_FILL_PERMILLE": (0, 750, 1000), "GEMM_W_SPLIT_MAX": (1, 2, 3, 4), "MID_PARTS_MAX": (1, 2, 4, 8, 16, 32),
            "GEMM_WIDE_MIN": (0, 128, 256, 512), "GEMM_W_SPLIT_OVH": (0, 12000)}
    for name in EXPERT_KNOBS:
        if name not in used:  # the switches
            used[name] = (0, 1)
    for name, vals in used.items():
        d, lo, hi = k[name]
        assert all(lo <= v <= hi for v in vals), name


def test_the_few_row_path_takes_the_calls_that_fill_one_round(lib):
    """mid_ok: single plans of the 48M / 317M models (and four 48M plans) take the few-row path, 30 / 8 plans do not; and nothing
    without the handle's split arithmetic, its switch, the K-split mode or the buffers it needs."""
    for model, E, want in (("c3", 1, True), ("c3", 4, True), ("c3", 30, False), ("c4", 1, True), ("c4", 2, False), ("c4", 8, False)):
        cfg = named_config(model)
        h = lrm.Handle(lib, cfg, E)
        assert h.mid_ok(lrm._ru(E * cfg.num_samples, 128)) == want, (model, E)
    rows_p, maxct = 512, 56
    assert lib.mid_ok_c(1, 1, 2, 1, 1, 0, 256, maxct, rows_p)
    for off in range(6):
        args = [1, 1, 2, 1, 1, 0]
        args[off] = 1 - args[off] if off != 2 else 0
        assert not lib.mid_ok_c(*args, 256, maxct, rows_p), off
