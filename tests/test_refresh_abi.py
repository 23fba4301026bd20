"""CPU: ABI 14 -- tdmpc2_plan_refresh_weights / tdmpc2_plan_soft_update_target are declared in the header, bound in Python, listed
in INTEGRATION.md and exported, the table's layout matches the header's, and the refusals that come before the device is touched
return the header's codes."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tdmpc2_plan_refresh_weights", "tdmpc2_plan_soft_update_target")


def test_abi_14_everywhere():
    from tdmpc2_amd import native

    hdr = open(os.path.join(ROOT, "include", "tdmpc2_plan.h")).read()
    assert re.search(r"#define TDMPC2_PLAN_ABI_VERSION 14\b", hdr) and native.ABI_VERSION == 14
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, hdr) and sym in native.ABI_SYMBOLS and f"`{sym}" in doc, sym
    assert "typedef struct tdmpc2_weight_table" in hdr and "refresh_state_dict" in doc and "soft_update_target" in doc


def test_table_layout():
    from tdmpc2_amd import native

    p = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(native.WeightEntry) == 4 * p
    assert native.WeightTable.enc.offset == 18 * 4 * p and native.WeightTable.enc_layers.offset == 24 * 4 * p
    assert ctypes.sizeof(native.WeightTable) == 24 * 4 * p + 4 * 13 + 4  # 13 int32, padded to the pointers' alignment


@pytest.fixture(scope="module")
def lib():
    from tdmpc2_amd import native

    if not os.path.exists(native.lib_path()):
        pytest.skip("library not built")
    lib = ctypes.CDLL(native.lib_path())
    lib.tdmpc2_last_error.restype = ctypes.c_char_p
    return lib


def test_refusals_before_the_device(lib):
    from tdmpc2_amd import native

    vp = ctypes.c_void_p
    lib.tdmpc2_plan_refresh_weights.argtypes = [vp, ctypes.POINTER(native.WeightTable), vp]
    lib.tdmpc2_plan_soft_update_target.argtypes = [vp, ctypes.POINTER(native.WeightTable), ctypes.POINTER(vp * 4), ctypes.c_float, vp]
    tab, tgt = native.WeightTable(), (vp * 4 * 3)()
    assert lib.tdmpc2_plan_refresh_weights(None, ctypes.byref(tab), None) == 1 and b"null" in lib.tdmpc2_last_error()
    assert lib.tdmpc2_plan_soft_update_target(None, ctypes.byref(tab), tgt, 0.01, None) == 1 and b"null" in lib.tdmpc2_last_error()
    fake = vp(1)  # never dereferenced: the arguments below are refused first
    assert lib.tdmpc2_plan_refresh_weights(fake, None, None) == 1 and b"null" in lib.tdmpc2_last_error()
    assert lib.tdmpc2_plan_soft_update_target(fake, None, tgt, 0.01, None) == 1
    assert lib.tdmpc2_plan_soft_update_target(fake, ctypes.byref(tab), None, 0.01, None) == 1
    for tau in (-0.01, 1.5, float("nan"), float("inf")):
        assert lib.tdmpc2_plan_soft_update_target(fake, ctypes.byref(tab), tgt, tau, None) == 1, tau
        assert b"tau" in lib.tdmpc2_last_error()
