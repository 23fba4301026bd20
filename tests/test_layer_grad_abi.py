"""CPU: the trainable layer's additions to ABI 14 (include/tdmpc2_plan.h: tdmpc2_layer_*).  The version stays 14; every new symbol
is declared, bound, documented and exported; the descriptor matches the header; and every refusal comes with its code and message
before the device is touched."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tdmpc2_layer_workspace_bytes", "tdmpc2_layer_forward", "tdmpc2_layer_backward")
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
    assert lib.tdmpc2_plan_abi_version() == 14
    declared = set(re.findall(r"\b(tdmpc2_[a-z_]+)\s*\(", hdr))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert s in declared, s
        assert s in native.ABI_SYMBOLS, s
        assert f"`{s}" in doc, s
        assert hasattr(lib, s), s
    assert {s for s in declared if s.startswith("tdmpc2_layer_")} == set(SYMBOLS)
    assert (native.LAYER_LINEAR, native.LAYER_MISH, native.LAYER_SIMNORM) == (0, 1, 2)


def test_descriptor_matches_the_header(tmp_path):
    from tdmpc2_amd import native

    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tdmpc2_plan.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(tdmpc2_layer_desc), offsetof(tdmpc2_layer_desc, rows),\n'
                   '         offsetof(tdmpc2_layer_desc, simnorm_dim), offsetof(tdmpc2_layer_desc, ln_eps),\n'
                   '         (int)TDMPC2_LAYER_LINEAR, (int)TDMPC2_LAYER_MISH, (int)TDMPC2_LAYER_SIMNORM);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = native.LayerDesc
    assert got == [C.sizeof(D), D.rows.offset, D.simnorm_dim.offset, D.ln_eps.offset, 0, 1, 2]
    assert got[0] == 32


def _desc(**over):
    from tdmpc2_amd import native

    f = dict(kind=native.LAYER_MISH, groups=2, rows=3, in_dim=4, out_dim=8, shared_x=False, simnorm_dim=0)
    f.update(over)
    return native.layer_desc(**f)


def _fwd(lib, d, x=P, w=P, b=P, ln_w=P, ln_b=P, mask=None, y=P, pre=P, stat=P):
    rc = lib.tdmpc2_layer_forward(C.byref(d) if d is not None else None, x, w, b, ln_w, ln_b, mask, y, pre, stat, None)
    return rc, lib.tdmpc2_last_error().decode()


def _bwd(lib, d, ws_bytes=1 << 30, **over):
    a = dict(x=P, w=P, ln_w=P, ln_b=P, pre=P, stat=P, mask=None, dy=P, dx=P, dw=P, db=P, dln_w=P, dln_b=P, ws=P)
    a.update(over)
    rc = lib.tdmpc2_layer_backward(C.byref(d) if d is not None else None, a["x"], a["w"], a["ln_w"], a["ln_b"], a["pre"], a["stat"],
                                   a["mask"], a["dy"], a["dx"], a["dw"], a["db"], a["dln_w"], a["dln_b"], a["ws"], ws_bytes, None)
    return rc, lib.tdmpc2_last_error().decode()


BAD_DESCRIPTORS = ((dict(kind=3), "unknown kind 3"), (dict(kind=-1), "unknown kind -1"), (dict(rows=0), "at least 1"),
                   (dict(in_dim=0), "at least 1"), (dict(out_dim=-2), "at least 1"), (dict(groups=0), "at least 1"),
                   (dict(kind=2, simnorm_dim=0), "simnorm_dim 0"), (dict(kind=2, simnorm_dim=3), "simnorm_dim 3 must be at least 1 and divide out_dim 8"),
                   (dict(groups=1, shared_x=True), "shared_x needs more than one group"))


def test_workspace_bytes_is_host_only(lib):
    from tdmpc2_amd import native

    n = C.c_size_t(7)
    assert lib.tdmpc2_layer_workspace_bytes(None, C.byref(n)) == INVALID and b"null descriptor" in lib.tdmpc2_last_error()
    assert lib.tdmpc2_layer_workspace_bytes(C.byref(_desc()), None) == INVALID and b"null" in lib.tdmpc2_last_error()
    for over, word in BAD_DESCRIPTORS:
        assert lib.tdmpc2_layer_workspace_bytes(C.byref(_desc(**over)), C.byref(n)) == INVALID, over
        assert word in lib.tdmpc2_last_error().decode(), (over, lib.tdmpc2_last_error())
    act = lambda G, R, N: -(-G * R * N * 4 // 256) * 256  # noqa: E731
    assert native.layer_workspace_bytes(_desc()) == 2 * act(2, 3, 8)
    assert native.layer_workspace_bytes(_desc(kind=native.LAYER_LINEAR)) == act(2, 3, 8)
    assert native.layer_workspace_bytes(_desc(kind=native.LAYER_SIMNORM, simnorm_dim=8, groups=5, rows=1024, out_dim=512)) == 2 * 5 * 1024 * 512 * 4
    assert native.layer_workspace_bytes(_desc(groups=5, rows=1 << 20, out_dim=4096)) == 2 * 5 * (1 << 20) * 4096 * 4  # past 2^32 bytes


def test_forward_refusals_come_before_the_device(lib):
    from tdmpc2_amd import native

    rc, msg = _fwd(lib, None)
    assert rc == INVALID and "null descriptor" in msg
    for over, word in BAD_DESCRIPTORS:
        rc, msg = _fwd(lib, _desc(**over))
        assert rc == INVALID and word in msg, (over, rc, msg)
    for arg in ("x", "w", "b", "y"):
        rc, msg = _fwd(lib, _desc(), **{arg: None})
        assert rc == INVALID and "null x, w, b or y" in msg, arg
    for arg in ("ln_w", "ln_b", "pre", "stat"):
        rc, msg = _fwd(lib, _desc(), **{arg: None})
        assert rc == INVALID and "needs ln_w, ln_b, pre and stat" in msg, arg
        rc, msg = _fwd(lib, _desc(kind=native.LAYER_SIMNORM, simnorm_dim=4), **{arg: None})
        assert rc == INVALID and "needs ln_w, ln_b, pre and stat" in msg, arg
    rc, msg = _fwd(lib, _desc(groups=1 << 20, rows=1 << 20, out_dim=1 << 20))
    assert rc == UNSUPPORTED and "workgroups" in msg


def test_backward_refusals_come_before_the_device(lib):
    from tdmpc2_amd import native

    rc, msg = _bwd(lib, None)
    assert rc == INVALID and "null descriptor" in msg
    for over, word in BAD_DESCRIPTORS:
        rc, msg = _bwd(lib, _desc(**over))
        assert rc == INVALID and word in msg, (over, rc, msg)
    d = _desc()
    need = native.layer_workspace_bytes(d)
    rc, msg = _bwd(lib, d, ws_bytes=need - 1)
    assert rc == INVALID and f"workspace of {need - 1} bytes is too small, {need} needed" in msg
    rc, msg = _bwd(lib, d, ws=None)
    assert rc == INVALID and "null workspace" in msg
    rc, msg = _bwd(lib, _desc(kind=native.LAYER_LINEAR), mask=P, ws_bytes=0)  # a masked Linear needs its dlin
    assert rc == INVALID and "too small" in msg
    for some in (("dw",), ("db",), ("dln_w",), ("dln_b",), ("dw", "db"), ("dw", "db", "dln_w")):
        rc, msg = _bwd(lib, d, **{k: None for k in some})
        assert rc == INVALID and f"{4 - len(some)} of the 4 parameter gradients given" in msg, some
    rc, msg = _bwd(lib, _desc(kind=native.LAYER_LINEAR), dw=None)
    assert rc == INVALID and "1 of the 2 parameter gradients given" in msg
    none = dict(dw=None, db=None, dln_w=None, dln_b=None)
    rc, msg = _bwd(lib, d, dx=None, **none)
    assert rc == INVALID and "nothing to compute" in msg
    rc, msg = _bwd(lib, d, dy=None)
    assert rc == INVALID and "null dy" in msg
    rc, msg = _bwd(lib, d, w=None)
    assert rc == INVALID and "dx needs w" in msg
    rc, msg = _bwd(lib, d, x=None)
    assert rc == INVALID and "need x" in msg
    for arg in ("ln_w", "ln_b", "pre", "stat"):
        rc, msg = _bwd(lib, d, **{arg: None})
        assert rc == INVALID and "needs ln_w, ln_b, pre and stat" in msg, arg


def test_no_cpu_fallback():
    import torch

    from tdmpc2_amd import autograd, layers, native

    with pytest.raises(native.NativeError, match="MI355X only"):
        autograd.mlp_apply(layers.mlp(4, [8], 3), torch.zeros(2, 4))
    with pytest.raises(native.NativeError, match="MI355X only"):
        autograd.ensemble_apply(layers.StackedMLPParams(2, 4, 8, 3), torch.zeros(2, 4))


def test_the_flag_is_off_by_default_and_forwarded():
    import torch

    from tdmpc2_amd import TDMPC2, native
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.world_model import WorldModel

    m = WorldModel(named_config("tiny"))
    assert m.native_autograd is False
    before = native.LAYER_CALLS
    m.native_autograd = True  # a CPU input keeps the modules: the flag routes GPU inputs only
    z, a = torch.zeros(3, 64), torch.zeros(3, 4)
    assert m.next(z, a, None).shape == (3, 64) and m.Q(z, a, None, return_type="all").shape[0] == 3
    assert native.LAYER_CALLS == before
    assert "native_autograd" in TDMPC2.__dict__ and isinstance(TDMPC2.__dict__["native_autograd"], property)
