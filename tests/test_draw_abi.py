"""CPU: the C ABI of the draw unit (include/tdmpc2_draw.h: tdmpc2_draw_noise), a header of its own beside ABI 14.  The new header
declares exactly its symbol; it is bound, exported and documented; include/tdmpc2_plan.h still declares 72 symbols at version 14,
include/tdmpc2_pi_grad.h its five and include/tdmpc2_dropout.h its one; the descriptor matches a compiled probe; every refusal
returns its code with its message before a device is touched (no GPU here: a call that reached the device could not answer
INVALID)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests import draw_common as dr

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


def test_the_new_header_declares_exactly_its_symbol(lib):
    from tdmpc2_amd import native

    _, declared = _declared("tdmpc2_draw.h")
    assert declared == set(dr.SYMBOLS) == set(native.DRAW_SYMBOLS) and len(native.DRAW_SYMBOLS) == 1
    assert native.PROTOTYPES["tdmpc2_draw.h"] is native._DRAW_H and native._UNIT_COUNTER["draw"] == "DRAW_CALLS"
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`include/tdmpc2_draw.h`" in doc
    hooks = C.CDLL(native.hooks_lib_path())  # linked into the hooks library too
    for s in dr.SYMBOLS:
        assert hasattr(lib, s) and hasattr(hooks, s), s
        assert s not in native.ABI_SYMBOLS and s not in native.PI_GRAD_SYMBOLS and s not in native.DROPOUT_SYMBOLS, s
        assert f"`{s}" in doc, s


def test_abi_14_and_the_other_unit_headers_are_untouched():
    from tdmpc2_amd import native

    hdr, declared = _declared("tdmpc2_plan.h")
    assert re.search(r"#define\s+TDMPC2_PLAN_ABI_VERSION\s+14\b", hdr) and native.ABI_VERSION == 14
    assert len(declared) == len(native.ABI_SYMBOLS) == 72 and not any(s.startswith("tdmpc2_draw") for s in declared)
    _, pg = _declared("tdmpc2_pi_grad.h")
    assert pg == set(native.PI_GRAD_SYMBOLS) and len(pg) == 5
    _, dm = _declared("tdmpc2_dropout.h")
    assert dm == set(native.DROPOUT_SYMBOLS) and len(dm) == 1


def test_descriptor_matches_the_header(tmp_path):
    from tdmpc2_amd import native

    fields = ("n", "num_q", "seed_lo", "seed_hi", "call_lo", "call_hi", "reserved")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tdmpc2_draw.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(tdmpc2_draw_desc));\n'
                   + "".join(f'  printf(" %zu", offsetof(tdmpc2_draw_desc, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = native.DrawDesc
    assert got == [C.sizeof(D)] + [getattr(D, f).offset for f in fields] == [32, 0, 8, 12, 16, 20, 24, 28]
    d = native.draw_desc(7, 5, seed=0x0123456789ABCDEF, call=0xFEDCBA9876543210)
    assert (d.n, d.num_q, d.seed_lo, d.seed_hi, d.call_lo, d.call_hi) == (7, 5, 0x89ABCDEF, 0x01234567, 0x76543210, 0xFEDCBA98)


def _call(lib, d, state=None, normal=P, pair=P):
    return lib.tdmpc2_draw_noise(None if d is None else C.byref(d), state, normal, pair, None)


def test_every_refusal_comes_before_the_device(lib):
    from tdmpc2_amd import native

    err = lambda: lib.tdmpc2_last_error().decode()  # noqa: E731
    good = native.draw_desc(5, 5)
    assert _call(lib, None) == INVALID and "draw_noise: null descriptor" in err()
    assert _call(lib, good, normal=None, pair=None) == INVALID and "both outputs are null" in err()
    for n in (-1, -4):
        assert _call(lib, native.draw_desc(n, 5)) == INVALID and f"n {n} is negative" in err(), n
    assert _call(lib, native.draw_desc(0, 5)) == INVALID and "n 0 with a normal buffer" in err()
    assert _call(lib, good, normal=None) == INVALID and "null normal with n 5" in err()
    for off in (4, 8, 12, 1):
        assert _call(lib, good, normal=P + off) == INVALID and "not 16-byte aligned" in err(), off
    assert _call(lib, good, state=P, normal=P + 4) == INVALID  # with a device counter too
    for q in (1, 0, -2, 9):
        assert _call(lib, native.draw_desc(5, q)) == INVALID and f"num_q {q} outside [2, 8]" in err(), q
        assert _call(lib, native.draw_desc(0, q), normal=None) == INVALID and "num_q" in err(), q  # the pair alone
    for n in (1 << 62, (1 << 63) - 1):
        assert _call(lib, native.draw_desc(n, 5)) == UNSUPPORTED and "2^62 elements" in err(), n
        assert _call(lib, native.draw_desc(n, 0), pair=None) == UNSUPPORTED  # num_q is not read without a pair


def test_no_cpu_fallback_and_surface():
    import torch

    from tdmpc2_amd import TDMPC2, autograd, native

    assert isinstance(native.DRAW_CALLS, int)
    with pytest.raises(native.NativeError, match="MI355X only"):
        native.draw_noise(native.draw_desc(8, 5), None, torch.zeros(8), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(native.NativeError, match="MI355X only"):
        native.draw_noise(native.draw_desc(0, 5), None, None, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(native.NativeError, match="both outputs"):
        native.draw_noise(native.draw_desc(0, 5), None)
    with pytest.raises(native.NativeError, match="two contiguous int32 words"):
        native.draw_noise(native.draw_desc(8, 5), None, torch.zeros(8), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(native.NativeError, match="MI355X only"):
        autograd.Draws(0, "cpu")
    assert all(callable(getattr(autograd.Draws, n)) for n in ("draw", "state_dict", "load_state_dict"))
    assert isinstance(TDMPC2.draws, property)
