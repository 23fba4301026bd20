"""CPU: the C ABI of the task unit (include/tdmpc2_task.h: tdmpc2_task_forward, tdmpc2_task_backward, tdmpc2_task_renorm), a header
of its own beside ABI 14.  The new header declares exactly its symbols; they are bound, exported from both libraries and
documented; include/tdmpc2_plan.h still declares 72 symbols at version 14, include/tdmpc2_pi_grad.h its five, include/tdmpc2_dropout.h
and include/tdmpc2_draw.h their one; the descriptor matches a compiled probe; every refusal returns its code with its message before
a device is touched (no GPU here: a call that reached the device could not answer INVALID); the flags exist and default to off."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests import task_common as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, HIP, STATE = range(5)
P = 256  # a non-null, 16-byte aligned pointer that is never dereferenced: every call below is refused first


@pytest.fixture(scope="module")
def lib():
    from tdmpc2_amd import native

    return native.load_library()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return hdr, set(re.findall(r"\b(tdmpc2_[a-z_]+)\s*\(", hdr))


def test_the_new_header_declares_exactly_its_symbols(lib):
    from tdmpc2_amd import native

    _, declared = _declared("tdmpc2_task.h")
    assert declared == set(tc.SYMBOLS) == set(native.TASK_SYMBOLS) and len(native.TASK_SYMBOLS) == 3
    assert native.PROTOTYPES["tdmpc2_task.h"] is native._TASK_H and native._UNIT_COUNTER["task"] == "TASK_CALLS"
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`include/tdmpc2_task.h`" in doc
    hooks = C.CDLL(native.hooks_lib_path())  # linked into the hooks library too
    for s in tc.SYMBOLS:
        assert hasattr(lib, s) and hasattr(hooks, s), s
        assert not any(s in group for group in (native.ABI_SYMBOLS, native.PI_GRAD_SYMBOLS, native.DROPOUT_SYMBOLS, native.DRAW_SYMBOLS)), s
        assert f"`{s}" in doc, s


def test_abi_14_and_the_other_unit_headers_are_untouched():
    from tdmpc2_amd import native

    hdr, declared = _declared("tdmpc2_plan.h")
    assert re.search(r"#define\s+TDMPC2_PLAN_ABI_VERSION\s+14\b", hdr) and native.ABI_VERSION == 14
    assert len(declared) == len(native.ABI_SYMBOLS) == 72 and not any(s.startswith("tdmpc2_task") for s in declared)
    for name, symbols, count in (("tdmpc2_pi_grad.h", native.PI_GRAD_SYMBOLS, 5), ("tdmpc2_dropout.h", native.DROPOUT_SYMBOLS, 1),
                                 ("tdmpc2_draw.h", native.DRAW_SYMBOLS, 1)):
        _, got = _declared(name)
        assert got == set(symbols) and len(got) == count, name


def test_descriptor_matches_the_header(tmp_path):
    from tdmpc2_amd import native

    fields = ("steps", "batch", "ids_len", "id_bytes", "num_tasks", "x_dim", "task_dim", "a_dim", "max_norm", "reserved")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tdmpc2_task.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(tdmpc2_task_desc));\n'
                   + "".join(f'  printf(" %zu", offsetof(tdmpc2_task_desc, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = native.TaskDesc
    assert got == [C.sizeof(D)] + [getattr(D, f).offset for f in fields] == [40] + list(range(0, 40, 4))
    d = native.task_desc(3, 43, 43, 8, 30, 24, 96, 6, 1.0)
    assert [getattr(d, f) for f in fields] == [3, 43, 43, 8, 30, 24, 96, 6, 1.0, 0]
    assert native.task_desc(1, 1, 1, 4, 1, 1, 1).a_dim == 0 and native.task_desc(1, 1, 1, 4, 1, 1, 1).max_norm == 1.0


def _desc(**kw):
    from tdmpc2_amd import native

    f = dict(steps=4, batch=12, ids_len=12, id_bytes=8, num_tasks=30, x_dim=8, task_dim=64, a_dim=4, max_norm=1.0)
    f.update(kw)
    return native.task_desc(**f)


def _fwd(lib, d, table=P, ids=P, x=P, a=P, out=P):
    return lib.tdmpc2_task_forward(None if d is None else C.byref(d), table, ids, x, a, out, None)


def _bwd(lib, d, ids=P, dout=P, dx=P, da=P, dtable=P):
    return lib.tdmpc2_task_backward(None if d is None else C.byref(d), ids, dout, dx, da, dtable, None)


def _ren(lib, d, table=P, ids=P):
    return lib.tdmpc2_task_renorm(None if d is None else C.byref(d), table, ids, None)


def test_every_refusal_comes_before_the_device(lib):
    err = lambda: lib.tdmpc2_last_error().decode()  # noqa: E731
    calls = (("task_forward", _fwd), ("task_backward", _bwd), ("task_renorm", _ren))
    for name, call in calls:
        assert call(lib, None) == INVALID and f"{name}: null descriptor" in err()
        assert call(lib, _desc(), ids=None) == INVALID and f"{name}: a required pointer is null" in err()
        for field, bad, msg in (("steps", 0, "steps 0 < 1"), ("steps", -3, "steps -3 < 1"), ("batch", 0, "batch 0 < 1"),
                                ("x_dim", 0, "x_dim 0 < 1"), ("task_dim", 0, "task_dim 0 < 1"), ("task_dim", -1, "task_dim -1 < 1"),
                                ("a_dim", -1, "a_dim -1 is negative"), ("num_tasks", 0, "num_tasks 0 < 1"),
                                ("ids_len", 2, "ids_len 2 is neither 1 nor batch 12"), ("ids_len", 0, "ids_len 0 is neither"),
                                ("id_bytes", 2, "id_bytes 2 is neither 4 nor 8"), ("id_bytes", 16, "id_bytes 16 is neither")):
            assert call(lib, _desc(**{field: bad})) == INVALID and f"{name}: {msg}" in err(), (name, field, bad)
        top = (1 << 31) - 1
        assert call(lib, _desc(steps=top, batch=top, ids_len=1)) == UNSUPPORTED and "2^62 elements or more" in err(), name
        assert call(lib, _desc(steps=top, batch=top, ids_len=1, id_bytes=5)) == INVALID  # INVALID comes first
    for p in ("table", "x", "out"):
        assert _fwd(lib, _desc(), **{p: None}) == INVALID and "task_forward: a required pointer is null" in err(), p
    assert _fwd(lib, _desc(a_dim=0)) == INVALID and "an action pointer with a_dim 0" in err()
    assert _fwd(lib, _desc(), a=None) == INVALID and "null a with a_dim 4" in err()
    assert _bwd(lib, _desc(), dout=None) == INVALID and "task_backward: a required pointer is null" in err()
    assert _bwd(lib, _desc(), dx=None, da=None, dtable=None) == INVALID and "all three outputs are null" in err()
    assert _bwd(lib, _desc(a_dim=0)) == INVALID and "an action pointer with a_dim 0" in err()
    assert _ren(lib, _desc(), table=None) == INVALID and "task_renorm: a required pointer is null" in err()
    big = dict(steps=1 << 20, batch=1 << 16, ids_len=1, x_dim=1, task_dim=1, a_dim=1)  # 2^36 rows: 2^32 row blocks
    assert _fwd(lib, _desc(**big)) == UNSUPPORTED and "2^31 workgroups" in err()
    assert _bwd(lib, _desc(**big)) == UNSUPPORTED and "2^31 workgroups" in err()
    assert _ren(lib, _desc(max_norm=0.0)) == OK  # nothing to do, nothing launched


def test_no_cpu_fallback_and_surface():
    import torch

    from tdmpc2_amd import TDMPC2, autograd, native
    from tdmpc2_amd.world_model import WorldModel

    assert isinstance(native.TASK_CALLS, int)
    table, ids, x = torch.zeros(30, 8), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 3)
    d = native.task_desc(1, 2, 2, 8, 30, 3, 8)
    before = native.TASK_CALLS
    with pytest.raises(native.NativeError, match="MI355X only"):
        native.task_forward(d, table, ids, x, None, torch.zeros(2, 11))
    with pytest.raises(native.NativeError, match="MI355X only"):
        native.task_backward(d, ids, torch.zeros(2, 11), dx=torch.zeros(2, 3))
    with pytest.raises(native.NativeError, match="MI355X only"):
        native.task_renorm(d, table, ids)
    with pytest.raises(native.NativeError, match="all three outputs"):
        native.task_backward(d, ids, torch.zeros(2, 11))
    with pytest.raises(native.NativeError, match="MI355X only"):
        autograd.task_concat(table, ids, x)
    with pytest.raises(native.NativeError, match="ids for 2 batch columns"):
        autograd.task_concat(table, torch.zeros(3, dtype=torch.int64), x)
    assert native.TASK_CALLS == before and issubclass(autograd.TaskConcatFn, torch.autograd.Function)
    assert isinstance(TDMPC2.native_task_emb, property)
    src = open(os.path.join(ROOT, "tdmpc2_amd", "world_model.py")).read()
    assert "self.native_task_emb = False" in src and hasattr(WorldModel, "_net_in")


def test_the_flags_default_to_off():
    from tdmpc2_amd import TDMPC2
    from tests import update_common as uc

    cfg, _ = uc.build("tiny_mt-B12")
    agent = TDMPC2(cfg, device="cpu")
    assert agent.native_task_emb is False and agent.model.native_task_emb is False
    agent.native_task_emb = True
    assert agent.model.native_task_emb is True
