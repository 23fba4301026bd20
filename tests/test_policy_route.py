"""CPU test of the policy prior's routes (tdmpc2_amd/csrc/policy_route.h, compiled with g++: tests/policy_route_model.py): for
every model size, single-task and multitask, several row counts and both forced routes -- every (row, output feature) of every
layer written exactly once, LDS within 160 KiB and within what each launch asks for, writes inside the workspace binding
allocates, the auto threshold -- and the argument checks of the policy entry points (no GPU needed)."""
import ctypes

import pytest

from tdmpc2_amd.config import MODEL_SIZE
from tests import policy_route_model as prm

MAX_ENVS = 512
ROWS = (1, 2, 8, 64, 256, MAX_ENVS)
LDS_MAX = 160 * 1024


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return prm.build(tmp_path_factory.mktemp("policy_route"))


def _dims(size, multitask):
    d = MODEL_SIZE[size]
    A, T = (6, 96) if multitask else (38, 0)
    L, M = d["latent_dim"], d["mlp_dim"]
    obs_dim = 39 if multitask else 223
    enc_w = max(obs_dim + T, d["enc_dim"], L)
    return L, M, A, T, enc_w


@pytest.mark.parametrize("multitask", [False, True])
@pytest.mark.parametrize("size", sorted(MODEL_SIZE))
def test_every_output_is_written_once(lib, size, multitask):
    L, M, A, T, enc_w = _dims(size, multitask)
    in0 = L + T
    maxw = max(in0, M, 2 * A)
    ws_x, ws_y = lib.ws_x(MAX_ENVS, M), lib.ws_y(MAX_ENVS, M, A)
    for E in ROWS:
        for mode in (prm.FORCE_ROW, prm.FORCE_SPREAD):
            r = prm.route(lib, E, in0, M, A, maxw, mode)
            assert r["kind"] == (prm.POL_ROW if mode == prm.FORCE_ROW else prm.POL_SPREAD), (size, E, mode)
            g = r["grids"]
            if r["kind"] == prm.POL_ROW:
                assert r["launches"] == 1 and g[0]["x"] == E and g[0]["y"] == 1
                assert g[0]["lds"] == lib.row_lds(maxw) <= LDS_MAX
                for width in (M, M, 2 * A):  # the three layers: features of every row, once
                    assert (prm.cover(lib, 1, g[0], E, width) == 1).all()
                assert (prm.cover(lib, 2, g[0], E, A) == 1).all()  # head: wave 0 of each row's workgroup
                continue
            assert r["launches"] == 6
            ins, outs = (in0, M, M), (M, M, 2 * A)
            for l in range(3):
                gg = g[2 * l]
                assert gg["R"] in (1, 2, 4, 8) and gg["in"] == ins[l] and gg["out"] == outs[l]
                assert gg["lds"] == lib.gemv_lds(gg["R"], ins[l]) <= LDS_MAX
                assert (prm.cover(lib, 0, gg, E, outs[l]) == 1).all(), (size, E, l)
                assert E * outs[l] <= ws_y  # the GEMV writes y [E, out]
                if l < 2:
                    ng = g[2 * l + 1]
                    assert ng["threads"] == 512 and ng["lds"] == 0 and ng["out"] == M
                    assert (prm.cover(lib, 1, ng, E, M) == 1).all()
                    assert E * M <= ws_x  # the norm writes x [E, M]
            assert g[5]["threads"] == 64 and (prm.cover(lib, 2, g[5], E, A) == 1).all()
        # acting on the row route with the encoder in the same launch: its LDS holds the widest layer of both
        r = prm.route(lib, E, in0, M, A, max(maxw, enc_w), prm.FORCE_ROW)
        if enc_w <= 1024:
            assert r["kind"] == prm.POL_ROW and r["grids"][0]["lds"] <= LDS_MAX


def test_rows_per_workgroup(lib):
    L, M, A, T, _ = _dims(317, True)
    for E, want in ((1, 1), (2, 2), (3, 4), (8, 8), (256, 8)):
        r = prm.route(lib, E, L + T, M, A, M, prm.FORCE_SPREAD)
        assert all(r["grids"][2 * l]["R"] == want for l in range(3)), (E, want)
        assert r["grids"][0]["y"] == (E + want - 1) // want


def test_auto_threshold(lib):
    """The row route for the 5M model at E = 1 (one launch, observation to action), the spread route for the wide models."""
    for multitask in (False, True):
        L, M, A, T, enc_w = _dims(5, multitask)
        assert prm.route(lib, 1, L + T, M, A, max(L + T, M, enc_w), prm.AUTO)["kind"] == prm.POL_ROW
        for size in (48, 317):
            L, M, A, T, _ = _dims(size, multitask)
            for E in ROWS:
                assert prm.route(lib, E, L + T, M, A, max(L + T, M), prm.AUTO)["kind"] == prm.POL_SPREAD, (size, E)


def test_policy_entry_points_reject_null_arguments():
    from tdmpc2_amd import native

    lib = ctypes.CDLL(native.lib_path())
    lib.tdmpc2_last_error.restype = ctypes.c_char_p
    vp, i32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    calls = {
        "tdmpc2_plan_bind_policy": ([vp, i32, vp, vp, vp, vp, i32, i32, vp], [None, 0, None, None, None, None, 512, 512, None]),
        "tdmpc2_plan_pi": ([vp, i32, vp, vp, vp, vp, u64, vp, vp], [None, 1, None, None, None, None, 0, None, None]),
        "tdmpc2_plan_act_pi": ([vp, i32, vp, i32, vp, vp, vp, i32, u64, vp, vp], [None, 1, None, 17, None, None, None, 0, 0, None, None]),
        "tdmpc2_plan_act_pi_pix": ([vp, i32, vp, i32, i32, vp, vp, i32, u64, vp, vp], [None, 1, None, 0, 9, None, None, 0, 0, None, None]),
    }
    for name, (argtypes, args) in calls.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, i32
        assert fn(*args) == 1, name  # TDMPC2_ERR_INVALID
        assert b"null" in lib.tdmpc2_last_error(), name


def test_policy_route_tuning_key_has_a_binding():
    """TDMPC2_TUNE_POLICY_ROUTE (= 9, after TDMPC2_TUNE_WAIT_US) <-> NativePlanner.set_policy_route; not in the expert-knob table."""
    import os
    import re

    from tdmpc2_amd import native

    hdr = open(os.path.join(prm.ROOT, "include", "tdmpc2_plan.h")).read()
    assert re.search(r"TDMPC2_TUNE_WAIT_US = 8,\s+TDMPC2_TUNE_POLICY_ROUTE = TDMPC2_TUNE_WAIT_US \+ 1,", hdr)
    assert native.TUNE_POLICY_ROUTE == 9 and native.TUNE_POLICY_ROUTE < native.TUNE_EXPERT
    src = open(native.__file__).read()
    body = src[src.index("def set_policy_route("):]
    body = body[:body.index("\n    def ", 10)]
    assert "tdmpc2_plan_set_tuning(self._h, TUNE_POLICY_ROUTE," in body
