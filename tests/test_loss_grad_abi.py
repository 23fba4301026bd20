"""CPU: the loss unit's additions to ABI 14 (include/tdmpc2_plan.h: tdmpc2_loss_*).  The version stays 14 and the header declares 72
symbols; every new symbol is declared, bound, documented and exported; the descriptor matches the header; every refusal returns its
code with its message before a device is touched (no GPU here: a call that reached the device could not answer INVALID)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests import loss_grad_common as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tdmpc2_loss_workspace_bytes", "tdmpc2_loss_forward", "tdmpc2_loss_backward")
OK, INVALID, UNSUPPORTED, HIP, STATE = range(5)
P = 256  # a non-null pointer that is never dereferenced: every call below is refused first
BIG = 1 << 40


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
    assert {s for s in declared if s.startswith("tdmpc2_loss_")} == set(SYMBOLS)
    assert len(declared) == len(native.ABI_SYMBOLS) == 72


def test_descriptor_matches_the_header(tmp_path):
    from tdmpc2_amd import native

    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tdmpc2_plan.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(tdmpc2_loss_desc), offsetof(tdmpc2_loss_desc, episodic),\n'
                   '         offsetof(tdmpc2_loss_desc, vmin), offsetof(tdmpc2_loss_desc, rho),\n'
                   '         offsetof(tdmpc2_loss_desc, termination_coef));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = native.LossDesc
    assert got == [C.sizeof(D), D.episodic.offset, D.vmin.offset, D.rho.offset, D.termination_coef.offset] == [56, 20, 24, 36, 52]


def _desc(episodic=True, **over):
    from tdmpc2_amd import native

    h = lc.hyper(101)
    d = dict(steps=3, batch=33, latent_dim=63, num_q=5, num_bins=101, episodic=episodic)
    d.update(over)
    return native.loss_desc(**d, **h)


def _fwd(lib, d, ins=None, losses=P, step_means=None, ws=P, ws_bytes=BIG):
    ins = [P] * 8 if ins is None else ins
    return lib.tdmpc2_loss_forward(C.byref(d) if d is not None else None, *ins, losses, step_means, ws, ws_bytes, None)


def _bwd(lib, d, ins=None, g=None, outs=(P, P, P, P)):
    ins = [P] * 8 if ins is None else ins
    return lib.tdmpc2_loss_backward(C.byref(d) if d is not None else None, *ins, g, *outs, None)


BAD_DESCS = ((dict(steps=0), INVALID, "steps 0"), (dict(steps=9), INVALID, "steps 9"), (dict(steps=-1), INVALID, "steps -1"),
             (dict(batch=0), INVALID, "batch 0"), (dict(latent_dim=0), INVALID, "latent_dim 0"), (dict(num_q=0), INVALID, "num_q 0"),
             (dict(num_bins=1), UNSUPPORTED, "num_bins 1"), (dict(num_bins=0), UNSUPPORTED, "num_bins 0"))


def test_descriptor_refusals_in_every_entry_point(lib):
    n = C.c_size_t(7)
    assert lib.tdmpc2_loss_workspace_bytes(None, C.byref(n)) == INVALID and b"null descriptor" in lib.tdmpc2_last_error()
    assert _fwd(lib, None) == INVALID and b"null descriptor" in lib.tdmpc2_last_error()
    assert _bwd(lib, None) == INVALID and b"null descriptor" in lib.tdmpc2_last_error()
    assert lib.tdmpc2_loss_workspace_bytes(C.byref(_desc()), None) == INVALID
    for over, code, word in BAD_DESCS:
        d = _desc(**over)
        for rc in (lib.tdmpc2_loss_workspace_bytes(C.byref(d), C.byref(n)), _fwd(lib, d), _bwd(lib, d)):
            assert rc == code and word in lib.tdmpc2_last_error().decode(), (over, rc, lib.tdmpc2_last_error())


def test_workspace_bytes(lib):
    from tdmpc2_amd import native

    assert native.loss_workspace_bytes(_desc()) == (3 + 5) * 3 * 33 * 4
    assert native.loss_workspace_bytes(_desc(episodic=False, steps=8, batch=1 << 24, num_q=5)) == 8 * 8 * (1 << 24) * 4


def test_pointer_refusals(lib):
    d, plain = _desc(), _desc(episodic=False)
    for i in range(6):  # a NULL required input
        ins = [P] * 8
        ins[i] = None
        assert _fwd(lib, d, ins) == INVALID and b"null z_pred" in lib.tdmpc2_last_error(), i
        assert _bwd(lib, d, ins) == INVALID and b"null z_pred" in lib.tdmpc2_last_error(), i
    assert _fwd(lib, d, losses=None) == INVALID and b"losses" in lib.tdmpc2_last_error()
    # termination pointers that do not match episodic
    for ins in ([P] * 6 + [None, P], [P] * 6 + [P, None], [P] * 6 + [None, None]):
        assert _fwd(lib, d, ins) == INVALID and b"episodic = 1" in lib.tdmpc2_last_error()
        assert _bwd(lib, d, ins) == INVALID and b"episodic = 1" in lib.tdmpc2_last_error()
    for ins in ([P] * 6 + [None, P], [P] * 6 + [P, None], [P] * 8):
        assert _fwd(lib, plain, ins) == INVALID and b"episodic = 0" in lib.tdmpc2_last_error()
        assert _bwd(lib, plain, ins, outs=(P, P, P, None)) == INVALID and b"episodic = 0" in lib.tdmpc2_last_error()
    assert _bwd(lib, plain, [P] * 6 + [None, None]) == INVALID and b"d_term_logit" in lib.tdmpc2_last_error()
    # workspace
    assert _fwd(lib, d, ws=None) == INVALID and b"null workspace" in lib.tdmpc2_last_error()
    need = (3 + 5) * 3 * 33 * 4
    assert _fwd(lib, d, ws_bytes=need - 1) == INVALID and b"too small" in lib.tdmpc2_last_error()
    # a backward with nothing to compute
    assert _bwd(lib, d, outs=(None, None, None, None)) == INVALID and b"every output is null" in lib.tdmpc2_last_error()


def test_a_grid_past_2_31_workgroups_is_unsupported(lib):
    huge = _desc(episodic=False, steps=8, batch=(1 << 31) - 1, latent_dim=1, num_bins=2, num_q=1 << 20)
    plain_ins = [P] * 6 + [None, None]
    assert _fwd(lib, huge, plain_ins) == UNSUPPORTED and b"2^31 workgroups" in lib.tdmpc2_last_error()
    assert _bwd(lib, huge, plain_ins, outs=(None, None, P, None)) == UNSUPPORTED and b"2^31 workgroups" in lib.tdmpc2_last_error()


def test_no_cpu_fallback_and_surface():
    import torch

    from tdmpc2_amd import TDMPC2, autograd, native
    from tdmpc2_amd.config import named_config

    cfg = named_config("tiny")
    T, B, L, NB, Qn = 2, 3, cfg.latent_dim, cfg.num_bins, cfg.num_q
    z = torch.zeros(T, B, L)
    with pytest.raises(native.NativeError, match="MI355X only"):
        autograd.model_loss(cfg, z, z, torch.zeros(T, B, NB), torch.zeros(T, B), torch.zeros(Qn, T, B, NB), torch.zeros(T, B),
                            *((torch.zeros(T, B),) * 2 if cfg.episodic else ()))
    assert isinstance(native.LOSS_CALLS, int) and callable(TDMPC2.update_model) and issubclass(autograd.ModelLossFn, torch.autograd.Function)
