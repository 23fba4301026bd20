"""CPU: the optimiser step's additions to ABI 14 (include/tdmpc2_plan.h: tdmpc2_optim_*).  The version stays 14; every new symbol is
declared, bound, documented and exported; the structs match the header; every refusal returns TDMPC2_ERR_INVALID with its message
before a device is touched (no GPU here: a call that reached the device could not answer INVALID); tdmpc2_optim_layout agrees with
the Python model."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests import optim_common as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tdmpc2_optim_layout", "tdmpc2_optim_create", "tdmpc2_optim_destroy", "tdmpc2_optim_step", "tdmpc2_optim_get_step",
           "tdmpc2_optim_set_step")
OK, INVALID, UNSUPPORTED, HIP, STATE = range(5)
P = 256  # a non-null pointer that is never dereferenced: every call below is refused first


@pytest.fixture(scope="module")
def lib():
    from tdmpc2_amd import native

    return native.load_library()


def test_version_symbols_and_documentation(lib):
    from tdmpc2_amd import native

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tdmpc2_plan.h")).read(), flags=re.S)
    assert re.search(r"#define\s+TDMPC2_PLAN_ABI_VERSION\s+14\b", hdr) and native.ABI_VERSION == 14
    declared = set(re.findall(r"\b(tdmpc2_[a-z_]+)\s*\(", hdr))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert s in declared and s in native.ABI_SYMBOLS and hasattr(lib, s), s
        assert f"`{s}" in doc, s
    assert {s for s in declared if s.startswith("tdmpc2_optim_")} == set(SYMBOLS)


def test_structs_match_the_header(tmp_path):
    from tdmpc2_amd import native

    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tdmpc2_plan.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(tdmpc2_optim_seg), offsetof(tdmpc2_optim_seg, count),\n'
                   '         offsetof(tdmpc2_optim_seg, group), sizeof(tdmpc2_optim_cfg), offsetof(tdmpc2_optim_cfg, beta1),\n'
                   '         offsetof(tdmpc2_optim_cfg, lr), offsetof(tdmpc2_optim_cfg, segs));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S, G = native.OptimSeg, native.OptimCfg
    assert got == [C.sizeof(S), S.count.offset, S.group.offset, C.sizeof(G), G.beta1.offset, G.lr.offset, G.segs.offset]
    assert got[0] == 24 and got[3] == 48


def _cfg(segs=((P, 5, 0), (P, 64, 1)), lrs=(3e-4, 1e-4), **over):
    from tdmpc2_amd import native

    h = dict(beta1=0.9, beta2=0.999, eps=1e-8, max_norm=20.0)
    h.update({k: v for k, v in over.items() if k in h})
    cfg, keep = native.optim_cfg(list(segs), list(lrs), h["beta1"], h["beta2"], h["eps"], h["max_norm"])
    for k in ("n_segs", "n_groups"):
        if k in over:
            setattr(cfg, k, over[k])
    if over.get("null_lr"):
        cfg.lr = None
    if over.get("null_segs"):
        cfg.segs = None
    return cfg, keep


NAN = float("nan")
BAD_CFGS = ((dict(null_lr=True), "null lr or segs"), (dict(null_segs=True), "null lr or segs"), (dict(n_segs=0), "at least 1"),
            (dict(n_segs=-1), "at least 1"), (dict(n_groups=0), "at least 1"), (dict(segs=((P, 0, 0),)), "count 0"),
            (dict(segs=((P, -4, 0),)), "count -4"), (dict(segs=((P, 5, 2),)), "group 2 of 2"), (dict(segs=((P, 5, -1),)), "group -1"),
            (dict(segs=((P, 5, 0), (None, 5, 1))), "segment 1 has a null param"),
            (dict(beta1=1.0), "beta1"), (dict(beta1=-0.5), "beta1"), (dict(beta2=1.0), "beta2"), (dict(beta2=-1e-3), "beta2"),
            (dict(eps=0.0), "eps"), (dict(eps=-1e-8), "eps"), (dict(max_norm=0.0), "max_norm"), (dict(max_norm=-1.0), "max_norm"),
            (dict(beta1=NAN), "NaN"), (dict(beta2=NAN), "NaN"), (dict(eps=NAN), "NaN"), (dict(max_norm=NAN), "NaN"))


def test_create_and_layout_refusals_come_before_the_device(lib):
    h = C.c_void_p(7)
    offs, total = (C.c_int64 * 4)(), C.c_int64()
    assert lib.tdmpc2_optim_create(None, C.byref(h)) == INVALID and b"null cfg" in lib.tdmpc2_last_error()
    cfg, keep = _cfg()
    assert lib.tdmpc2_optim_create(C.byref(cfg), None) == INVALID and b"null out" in lib.tdmpc2_last_error()
    assert lib.tdmpc2_optim_layout(None, offs, C.byref(total)) == INVALID and b"null cfg" in lib.tdmpc2_last_error()
    assert lib.tdmpc2_optim_layout(C.byref(cfg), None, C.byref(total)) == INVALID and b"null offsets" in lib.tdmpc2_last_error()
    assert lib.tdmpc2_optim_layout(C.byref(cfg), offs, None) == INVALID
    for over, word in BAD_CFGS:
        cfg, keep = _cfg(**over)
        h = C.c_void_p(7)
        assert lib.tdmpc2_optim_create(C.byref(cfg), C.byref(h)) == INVALID, over
        assert word in lib.tdmpc2_last_error().decode() and not h.value, (over, lib.tdmpc2_last_error())
        assert lib.tdmpc2_optim_layout(C.byref(cfg), offs, C.byref(total)) == INVALID, over


def test_step_and_set_step_refusals(lib):
    assert lib.tdmpc2_optim_step(None, P, P, P, 1, None, None) == INVALID and b"null handle" in lib.tdmpc2_last_error()
    assert lib.tdmpc2_optim_set_step(None, 3, None) == INVALID and b"null handle" in lib.tdmpc2_last_error()
    n = C.c_int64()
    assert lib.tdmpc2_optim_get_step(None, C.byref(n), None) == INVALID
    lib.tdmpc2_optim_destroy(None)  # a null handle is ignored


def test_layout_agrees_with_the_python_model():
    from tdmpc2_amd import native

    for case in oc.cases():
        cfg, keep = native.optim_cfg([(P, c, g) for c, g in zip(case["counts"], case["groups"])], case["lrs"], 0.9, 0.999, 1e-8, 1.0)
        assert native.optim_layout(cfg) == oc.layout(case["counts"]), case["name"]
    cfg, keep = native.optim_cfg([(P, (1 << 33) + 1, 0), (P, 5, 0)], [1e-3], 0.9, 0.999, 1e-8, 1.0)  # past 2^32 elements
    assert native.optim_layout(cfg) == ([0, (1 << 33) + 4], (1 << 33) + 12)


def test_no_cpu_fallback_and_export():
    import torch

    import tdmpc2_amd
    from tdmpc2_amd import TDMPC2, native

    with pytest.raises(native.NativeError, match="MI355X only"):
        tdmpc2_amd.ClipAdam([torch.nn.Parameter(torch.zeros(4))], lr=1e-3, max_norm=1.0)
    assert "ClipAdam" in tdmpc2_amd.__all__
    for name in ("optim", "pi_optim"):
        assert isinstance(TDMPC2.__dict__[name], property)
    assert callable(TDMPC2.optimizer_step)
