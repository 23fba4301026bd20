"""CPU: the C ABI of the dropout-mask unit (include/tdmpc2_dropout.h: tdmpc2_dropout_mask), a header of its own beside ABI 14.  The
new header declares exactly its symbol; it is bound, exported and documented; include/tdmpc2_plan.h still declares 72 symbols at
version 14 and include/tdmpc2_pi_grad.h its five; the descriptor matches a compiled probe; every refusal returns its code with its
message before a device is touched (no GPU here: a call that reached the device could not answer INVALID)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests import dropout_common as dc

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

    _, declared = _declared("tdmpc2_dropout.h")
    assert declared == set(dc.SYMBOLS) == set(native.DROPOUT_SYMBOLS) and len(native.DROPOUT_SYMBOLS) == 1
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`include/tdmpc2_dropout.h`" in doc
    hooks = C.CDLL(native.hooks_lib_path())  # linked into the hooks library too
    for s in dc.SYMBOLS:
        assert hasattr(lib, s) and hasattr(hooks, s), s
        assert s not in native.ABI_SYMBOLS and s not in native.PI_GRAD_SYMBOLS, s
        assert f"`{s}" in doc, s


def test_abi_14_and_the_policy_loss_header_are_untouched():
    from tdmpc2_amd import native

    hdr, declared = _declared("tdmpc2_plan.h")
    assert re.search(r"#define\s+TDMPC2_PLAN_ABI_VERSION\s+14\b", hdr) and native.ABI_VERSION == 14
    assert len(declared) == len(native.ABI_SYMBOLS) == 72 and not any(s.startswith("tdmpc2_dropout") for s in declared)
    _, pg = _declared("tdmpc2_pi_grad.h")
    assert pg == set(native.PI_GRAD_SYMBOLS) and len(pg) == 5


def test_descriptor_matches_the_header(tmp_path):
    from tdmpc2_amd import native

    fields = ("n", "p", "seed_lo", "seed_hi", "call_lo", "call_hi", "reserved")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tdmpc2_dropout.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(tdmpc2_dropout_desc));\n'
                   + "".join(f'  printf(" %zu", offsetof(tdmpc2_dropout_desc, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = native.DropoutDesc
    assert got == [C.sizeof(D)] + [getattr(D, f).offset for f in fields] == [32, 0, 8, 12, 16, 20, 24, 28]
    d = native.dropout_desc(7, 0.25, seed=0x0123456789ABCDEF, call=0xFEDCBA9876543210)
    assert (d.n, d.seed_lo, d.seed_hi, d.call_lo, d.call_hi) == (7, 0x89ABCDEF, 0x01234567, 0x76543210, 0xFEDCBA98)


def _call(lib, d, state=None, mask=P):
    return lib.tdmpc2_dropout_mask(None if d is None else C.byref(d), state, mask, None)


def test_every_refusal_comes_before_the_device(lib):
    from tdmpc2_amd import native

    good = native.dropout_desc(5, 0.25)
    assert _call(lib, None) == INVALID and b"dropout_mask: null descriptor" in lib.tdmpc2_last_error()
    assert _call(lib, good, mask=None) == INVALID and b"null mask" in lib.tdmpc2_last_error()
    for n, word in ((0, "n 0"), (-4, "n -4")):
        assert _call(lib, native.dropout_desc(n, 0.25)) == INVALID and word in lib.tdmpc2_last_error().decode(), n
    for p in (float("nan"), -0.01, 1.0, 2.0):
        assert _call(lib, native.dropout_desc(5, p)) == INVALID and b"outside [0, 1)" in lib.tdmpc2_last_error(), p
    for off in (4, 8, 12, 1):
        assert _call(lib, good, mask=P + off) == INVALID and b"not 16-byte aligned" in lib.tdmpc2_last_error(), off
    assert _call(lib, good, state=P, mask=P + 4) == INVALID  # with a device counter too
    for n in (1 << 62, (1 << 63) - 1):
        assert _call(lib, native.dropout_desc(n, 0.25)) == UNSUPPORTED and b"2^62 elements" in lib.tdmpc2_last_error(), n


def test_no_cpu_fallback_and_surface():
    import torch

    from tdmpc2_amd import TDMPC2, autograd, layers, native
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.world_model import WorldModel

    assert isinstance(native.DROPOUT_CALLS, int)
    with pytest.raises(native.NativeError, match="MI355X only"):
        native.dropout_mask(native.dropout_desc(8, 0.25), None, torch.zeros(8))
    with pytest.raises(native.NativeError, match="MI355X only"):
        autograd.DropoutMasks(0, "cpu")
    assert all(callable(getattr(autograd.DropoutMasks, n)) for n in ("draw", "state_dict", "load_state_dict"))
    cfg = named_config("tiny")
    assert cfg.dropout == 0.01  # the reference's default
    m = WorldModel(cfg)
    assert m.native_dropout is False and isinstance(TDMPC2.native_dropout, property)
    # on the CPU nothing is drawn in any mode, with the flag on or off: the outputs are what they were
    before = native.DROPOUT_CALLS
    z, a = torch.randn(6, cfg.latent_dim), torch.rand(6, cfg.action_dim)
    m.train()
    q0, p0 = m.Q(z, a, None, "all"), m.Q_pair(z, a, None, (1, 0))
    m.native_dropout = True
    q1, p1 = m.Q(z, a, None, "all"), m.Q_pair(z, a, None, (1, 0))
    assert native.DROPOUT_CALLS == before and torch.equal(q0, q1) and torch.equal(p0, p1)
    # a mask that is given is used, on the torch path too
    mask = torch.ones(cfg.num_q, 6, cfg.mlp_dim)
    mask[:, :, ::2] = 0.0
    q2 = m.Q(z, a, None, "all", q_mask=mask)
    assert not torch.equal(q2, q0) and torch.equal(q2, layers.QEnsemble.apply_params(m._Qs.params, torch.cat([z, a], -1), mask))
    assert torch.equal(m.Q_pair(z, a, None, (1, 0), q_mask=mask[[1, 0]]), q2[[1, 0]])
