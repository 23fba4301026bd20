"""CPU: the C ABI of the policy-loss unit (include/tdmpc2_pi_grad.h: tdmpc2_pigrad_*), a header of its own beside ABI 14.  The new
header declares exactly the five symbols; each is bound, exported and documented; include/tdmpc2_plan.h still declares 72 symbols at
version 14; the descriptor matches the header; every refusal returns its code with its message before a device is touched (no GPU
here: a call that reached the device could not answer INVALID)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests import pi_grad_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, HIP, STATE = range(5)
P = 256  # a non-null pointer that is never dereferenced: every call below is refused first


@pytest.fixture(scope="module")
def lib():
    from tdmpc2_amd import native

    return native.load_library()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return hdr, set(re.findall(r"\b(tdmpc2_[a-z_]+)\s*\(", hdr))


def test_the_new_header_declares_exactly_the_five_symbols(lib):
    from tdmpc2_amd import native

    _, declared = _declared("tdmpc2_pi_grad.h")
    assert declared == set(pc.SYMBOLS) == set(native.PI_GRAD_SYMBOLS) and len(native.PI_GRAD_SYMBOLS) == 5
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`include/tdmpc2_pi_grad.h`" in doc
    for s in pc.SYMBOLS:
        assert hasattr(lib, s) and s not in native.ABI_SYMBOLS, s
        assert f"`{s}" in doc, s
    hooks = C.CDLL(native.hooks_lib_path())  # linked into the hooks library too
    assert all(hasattr(hooks, s) for s in pc.SYMBOLS)


def test_abi_14_is_untouched():
    from tdmpc2_amd import native

    hdr, declared = _declared("tdmpc2_plan.h")
    assert re.search(r"#define\s+TDMPC2_PLAN_ABI_VERSION\s+14\b", hdr) and native.ABI_VERSION == 14
    assert len(declared) == len(native.ABI_SYMBOLS) == 72 and not any(s.startswith("tdmpc2_pigrad") for s in declared)


def test_descriptor_matches_the_header(tmp_path):
    from tdmpc2_amd import native

    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tdmpc2_pi_grad.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(tdmpc2_pigrad_desc), offsetof(tdmpc2_pigrad_desc, action_dim),\n'
                   '         offsetof(tdmpc2_pigrad_desc, multitask), offsetof(tdmpc2_pigrad_desc, vmin),\n'
                   '         offsetof(tdmpc2_pigrad_desc, entropy_coef), offsetof(tdmpc2_pigrad_desc, log_std_dif));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = native.PiGradDesc
    assert got == [C.sizeof(D), D.action_dim.offset, D.multitask.offset, D.vmin.offset, D.entropy_coef.offset,
                   D.log_std_dif.offset] == [44, 8, 16, 20, 32, 40]


def _desc(multitask=False, **over):
    from tdmpc2_amd import native

    d = dict(steps=3, batch=9, action_dim=6, num_bins=101, multitask=multitask)
    d.update(over)
    return native.pigrad_desc(**d, **pc.hyper())


def _calls(lib, d, mask=None):
    """Every entry point with non-null pointers throughout (mask as given)."""
    dp = C.byref(d) if d is not None else None
    return (lib.tdmpc2_pigrad_head_forward(dp, P, P, mask, P, P, P, None),
            lib.tdmpc2_pigrad_head_backward(dp, P, P, mask, P, P, P, None),
            lib.tdmpc2_pigrad_value_forward(dp, P, P, None),
            lib.tdmpc2_pigrad_loss_forward(dp, P, P, P, P, P, P, None),
            lib.tdmpc2_pigrad_loss_backward(dp, P, P, None, P, P, None))


BAD_DESCS = ((dict(steps=0), INVALID, "steps 0"), (dict(steps=17), INVALID, "steps 17"), (dict(steps=-1), INVALID, "steps -1"),
             (dict(batch=0), INVALID, "batch 0"), (dict(action_dim=0), INVALID, "action_dim 0"),
             (dict(action_dim=65), INVALID, "action_dim 65"), (dict(num_bins=1), UNSUPPORTED, "num_bins 1"),
             (dict(num_bins=0), UNSUPPORTED, "num_bins 0"), (dict(num_bins=4097), UNSUPPORTED, "num_bins 4097"))


def test_descriptor_refusals_in_every_entry_point(lib):
    assert _calls(lib, None) == (INVALID,) * 5 and b"null descriptor" in lib.tdmpc2_last_error()
    for over, code, word in BAD_DESCS:
        assert _calls(lib, _desc(**over)) == (code,) * 5, over
        msg = lib.tdmpc2_last_error().decode()  # of the last call made
        assert word in msg and "pigrad_loss_backward" in msg, (over, msg)


def test_pointer_refusals(lib):
    d, mt = _desc(), _desc(multitask=True)
    dp, mp = C.byref(d), C.byref(mt)
    for i in (0, 1, 3, 4, 5):  # head_forward: every pointer but the mask is required
        a = [P, P, None, P, P, P]
        a[i] = None
        assert lib.tdmpc2_pigrad_head_forward(dp, *a, None) == INVALID and b"null pi_out" in lib.tdmpc2_last_error(), i
    for i in (0, 1):
        a = [P, P, None, P, P, P]
        a[i] = None
        assert lib.tdmpc2_pigrad_head_backward(dp, *a, None) == INVALID and b"null pi_out or eps" in lib.tdmpc2_last_error(), i
    # a mask that does not match multitask
    assert lib.tdmpc2_pigrad_head_forward(dp, P, P, P, P, P, P, None) == INVALID and b"multitask = 0" in lib.tdmpc2_last_error()
    assert lib.tdmpc2_pigrad_head_backward(dp, P, P, P, P, P, P, None) == INVALID and b"multitask = 0" in lib.tdmpc2_last_error()
    assert lib.tdmpc2_pigrad_head_forward(mp, P, P, None, P, P, P, None) == INVALID and b"multitask = 1" in lib.tdmpc2_last_error()
    assert lib.tdmpc2_pigrad_head_backward(mp, P, P, None, P, P, P, None) == INVALID and b"multitask = 1" in lib.tdmpc2_last_error()
    # both incoming gradients NULL; no output
    assert lib.tdmpc2_pigrad_head_backward(dp, P, P, None, None, None, P, None) == INVALID
    assert b"no incoming gradient" in lib.tdmpc2_last_error()
    assert lib.tdmpc2_pigrad_head_backward(dp, P, P, None, P, None, None, None) == INVALID and b"d_pi_out is null" in lib.tdmpc2_last_error()
    for a in ((None, P), (P, None)):
        assert lib.tdmpc2_pigrad_value_forward(dp, *a, None) == INVALID and b"null q_logits or q" in lib.tdmpc2_last_error()
    for i in range(5):  # loss_forward: step_means alone is optional
        a = [P] * 6
        a[i] = None
        assert lib.tdmpc2_pigrad_loss_forward(dp, *a, None) == INVALID and b"null q, entropy" in lib.tdmpc2_last_error(), i
    for a in ((None, P), (P, None)):
        assert lib.tdmpc2_pigrad_loss_backward(dp, *a, None, P, P, None) == INVALID and b"null q_logits or scale" in lib.tdmpc2_last_error()
    assert lib.tdmpc2_pigrad_loss_backward(dp, P, P, P, None, None, None) == INVALID and b"every output is null" in lib.tdmpc2_last_error()


def test_a_grid_past_2_31_workgroups_is_unsupported(lib):
    huge = _desc(steps=16, batch=(1 << 31) - 1)  # 2^35 rows: 2^30 head workgroups fit, 2^33 wavefront groups do not
    dp = C.byref(huge)
    assert lib.tdmpc2_pigrad_value_forward(dp, P, P, None) == UNSUPPORTED and b"2^31 workgroups" in lib.tdmpc2_last_error()
    assert lib.tdmpc2_pigrad_loss_backward(dp, P, P, None, P, None, None) == UNSUPPORTED and b"2^31 workgroups" in lib.tdmpc2_last_error()
    # (the head's grid, 32 rows per workgroup, is 2^30 at that size: the wavefront-per-row launches run out first)
    assert lib.tdmpc2_pigrad_head_forward(dp, P, P, None, P, P, None, None) == INVALID  # refused on its pointers, not its grid


def test_no_cpu_fallback_and_surface():
    import torch

    from tdmpc2_amd import TDMPC2, autograd, native
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.scale import RunningScale
    from tdmpc2_amd.world_model import WorldModel

    cfg = named_config("tiny")
    T, B, A, NB = 2, 3, cfg.action_dim, cfg.num_bins
    scale = RunningScale(cfg, lambda: None, "cpu")
    with pytest.raises(native.NativeError, match="MI355X only"):
        autograd.pi_loss(cfg, torch.zeros(2, T, B, NB), torch.zeros(T, B), torch.zeros(T, B), scale)
    d = autograd.pi_desc(cfg, T, B, A, NB, -10.0, 12.0)
    with pytest.raises(native.NativeError, match="MI355X only"):
        autograd.PiHeadFn.apply(d, torch.zeros(T, B, 2 * A), torch.zeros(T, B, A), None)
    with pytest.raises(native.NativeError, match=r"q_logits \[2, T, B, bins\]"):
        autograd.pi_loss(cfg, torch.zeros(3, T, B, NB), torch.zeros(T, B), torch.zeros(T, B), scale)
    assert isinstance(native.PI_GRAD_CALLS, int)
    assert all(callable(getattr(TDMPC2, n)) for n in ("update_pi", "update", "_update")) and callable(WorldModel.Q_pair)
    assert issubclass(autograd.PiHeadFn, torch.autograd.Function) and issubclass(autograd.PiLossFn, torch.autograd.Function)
    # the torch tail of pi is what it was: with the flag off (and on the CPU in any case) no library call is made
    m = WorldModel(cfg)
    before = native.PI_GRAD_CALLS
    torch.manual_seed(0)
    a0, i0 = m.pi(torch.zeros(4, cfg.latent_dim), None)
    m.native_autograd = True
    torch.manual_seed(0)
    a1, i1 = m.pi(torch.zeros(4, cfg.latent_dim), None)
    assert native.PI_GRAD_CALLS == before and torch.equal(a0, a1) and torch.equal(i0["scaled_entropy"], i1["scaled_entropy"])
    eps = torch.randn(4, A)
    assert torch.equal(m.pi(torch.zeros(4, cfg.latent_dim), None, eps=eps)[0], m.pi(torch.zeros(4, cfg.latent_dim), None, eps=eps)[0])
