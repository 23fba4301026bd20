"""CPU: the C ABI of the pixel-gradient unit (include/tdmpc2_pixel_grad.h: tdmpc2_pixgrad_workspace_bytes, _shift_table, _forward,
_backward), a header of its own beside ABI 14.  The header declares exactly its symbols; they are bound, exported from both
libraries and documented; include/tdmpc2_plan.h still declares 72 symbols at version 14 and the other unit headers theirs; the
descriptor matches a compiled probe; every refusal returns its code with its message before a device is touched (no GPU here: a call
that reached the device could not answer INVALID / UNSUPPORTED); the shift table is pixel_route.h's; the flags exist and default to
off."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, 1, 2
P = 256  # a non-null pointer that is never dereferenced: every device call below is refused first
SYMBOLS = ("tdmpc2_pixgrad_workspace_bytes", "tdmpc2_pixgrad_shift_table", "tdmpc2_pixgrad_forward", "tdmpc2_pixgrad_backward")


@pytest.fixture(scope="module")
def lib():
    from tdmpc2_amd import native

    return native.load_library()


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return hdr, set(re.findall(r"\b(tdmpc2_[a-z_]+)\s*\(", hdr))


def test_the_new_header_declares_exactly_its_symbols(lib):
    from tdmpc2_amd import native

    _, declared = _declared("tdmpc2_pixel_grad.h")
    assert declared == set(SYMBOLS) == set(native.PIXEL_GRAD_SYMBOLS)
    assert native.PROTOTYPES["tdmpc2_pixel_grad.h"] is native._PIXEL_GRAD_H and native._UNIT_COUNTER["pixgrad"] == "PIXEL_GRAD_CALLS"
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`include/tdmpc2_pixel_grad.h`" in doc
    hooks = C.CDLL(native.hooks_lib_path())  # linked into the hooks library too
    for s in SYMBOLS:
        assert hasattr(lib, s) and hasattr(hooks, s), s
        assert not any(s in g for g in (native.ABI_SYMBOLS, native.PI_GRAD_SYMBOLS, native.DROPOUT_SYMBOLS, native.DRAW_SYMBOLS,
                                        native.TASK_SYMBOLS)), s
        assert f"`{s}" in doc, s


def test_abi_14_and_the_other_unit_headers_are_untouched():
    from tdmpc2_amd import native

    hdr, declared = _declared("tdmpc2_plan.h")
    assert re.search(r"#define\s+TDMPC2_PLAN_ABI_VERSION\s+14\b", hdr) and native.ABI_VERSION == 14
    assert len(declared) == len(native.ABI_SYMBOLS) == 72 and not any(s.startswith("tdmpc2_pixgrad") for s in declared)
    for name, symbols, count in (("tdmpc2_pi_grad.h", native.PI_GRAD_SYMBOLS, 5), ("tdmpc2_dropout.h", native.DROPOUT_SYMBOLS, 1),
                                 ("tdmpc2_draw.h", native.DRAW_SYMBOLS, 1), ("tdmpc2_task.h", native.TASK_SYMBOLS, 3)):
        _, got = _declared(name)
        assert got == set(symbols) and len(got) == count, name


def test_descriptor_matches_the_header(tmp_path):
    from tdmpc2_amd import native

    fields = ("n", "cin", "C", "obs_dtype", "seed_is_preact", "reserved")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tdmpc2_pixel_grad.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(tdmpc2_pixgrad_desc));\n'
                   + "".join(f'  printf(" %zu", offsetof(tdmpc2_pixgrad_desc, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D = native.PixGradDesc
    assert got == [C.sizeof(D)] + [getattr(D, f).offset for f in fields] == [24] + list(range(0, 24, 4))
    d = native.pixgrad_desc(17, 9, 32, 1, True)
    assert [getattr(d, f) for f in fields] == [17, 9, 32, 1, 1, 0]


def _desc(**kw):
    from tdmpc2_amd import native

    f = dict(n=3, cin=9, channels=32, obs_dtype=0, seed_is_preact=False)
    f.update(kw)
    return native.pixgrad_desc(**f)


def _four(*ptrs):
    arr = (C.c_void_p * 4)(*ptrs)
    return C.cast(arr, C.c_void_p), arr


def _fwd(lib, d, obs=P, shift=P, tab=P, W=(P,) * 4, b=(P,) * 4, fwd_ws=P, acts=P):
    Wp, k1 = (None, None) if W is None else _four(*W)
    bp, k2 = (None, None) if b is None else _four(*b)
    return lib.tdmpc2_pixgrad_forward(None if d is None else C.byref(d), obs, shift, tab, Wp, bp, fwd_ws, acts, None)


def _bwd(lib, d, obs=P, shift=P, tab=P, W=(P,) * 4, acts=P, dz=P, bwd_ws=P, dW=(P,) * 4, db=(P,) * 4):
    Wp, k1 = _four(*W)
    dWp, k2 = _four(*dW)
    dbp, k3 = _four(*db)
    return lib.tdmpc2_pixgrad_backward(None if d is None else C.byref(d), obs, shift, tab, Wp, acts, dz, bwd_ws, dWp, dbp, None)


def _ws(lib, d, a=True, f=True, b=True):
    x, y, z = C.c_size_t(), C.c_size_t(), C.c_size_t()
    return lib.tdmpc2_pixgrad_workspace_bytes(None if d is None else C.byref(d), C.byref(x) if a else None, C.byref(y) if f else None,
                                              C.byref(z) if b else None)


def test_every_refusal_comes_before_the_device(lib):
    err = lambda: lib.tdmpc2_last_error().decode()  # noqa: E731
    for name, call in (("pixgrad_forward", _fwd), ("pixgrad_backward", _bwd), ("pixgrad_workspace_bytes", _ws)):
        assert call(lib, None) == INVALID and f"{name}: null descriptor" in err()
        for kw, code, msg in ((dict(n=0), INVALID, "n 0 < 1"), (dict(n=-2), INVALID, "n -2 < 1"),
                              (dict(cin=0), UNSUPPORTED, "0 input channels outside [1, 16]"),
                              (dict(cin=17), UNSUPPORTED, "17 input channels outside [1, 16]"),
                              (dict(channels=4), UNSUPPORTED, "4 channels outside [8, 64]"),
                              (dict(channels=68), UNSUPPORTED, "68 channels outside [8, 64]"),
                              (dict(channels=30), UNSUPPORTED, "30 channels outside [8, 64] or no multiple of 4"),
                              (dict(obs_dtype=2), INVALID, "obs_dtype 2"), (dict(seed_is_preact=2), INVALID, "seed_is_preact 2"),
                              (dict(n=(1 << 20) + 1), UNSUPPORTED, "above 1048576 images")):
            d = _desc(**{k: v for k, v in kw.items() if k != "seed_is_preact"})
            if "seed_is_preact" in kw:
                d.seed_is_preact = kw["seed_is_preact"]
            assert call(lib, d) == code and f"{name}: " in err() and msg in err(), (name, kw, err())
    for p in ("obs", "shift", "tab", "fwd_ws", "acts", "W", "b"):
        assert _fwd(lib, _desc(), **{p: None}) == INVALID and "pixgrad_forward: null argument" in err(), p
    assert _fwd(lib, _desc(), W=(P, P, None, P)) == INVALID and "null weight or bias of layer 2" in err()
    assert _fwd(lib, _desc(), b=(None, P, P, P)) == INVALID and "null weight or bias of layer 0" in err()
    for p in ("obs", "shift", "tab", "acts", "dz", "bwd_ws"):
        assert _bwd(lib, _desc(), **{p: None}) == INVALID and "pixgrad_backward: null argument" in err(), p
    assert _bwd(lib, _desc(), W=(P, None, P, P)) == INVALID and "null weight of layer 1" in err()
    assert _bwd(lib, _desc(), dW=(P, P, P, None)) == INVALID and "dW and db of layer 3 are given or NULL together" in err()
    assert _bwd(lib, _desc(), db=(None, P, P, P)) == INVALID and "dW and db of layer 0" in err()
    assert _bwd(lib, _desc(), dW=(None,) * 4, db=(None,) * 4) == INVALID and "nothing to compute" in err()
    assert _ws(lib, _desc(), b=False) == INVALID and "pixgrad_workspace_bytes: null argument" in err()
    assert lib.tdmpc2_pixgrad_shift_table(None) == INVALID and "pixgrad_shift_table: null argument" in err()


def test_workspace_sizes():
    from tdmpc2_amd import native

    for n, cin, Cc in ((1, 1, 8), (17, 16, 64), (256, 9, 32)):
        a, f, b = native.pixgrad_workspace_bytes(native.pixgrad_desc(n, cin, Cc))
        assert a == 4 * n * Cc * (841 + 169 + 36 + 16)
        assert f == 4 * Cc * (49 * cin + 25 * Cc + 9 * Cc + 9 * Cc)
        parts = max(-(-n * hw // 256) * (k * k * (cin if l == 0 else Cc) + 1) * Cc
                    for l, (hw, k) in enumerate(((841, 7), (169, 5), (36, 3), (16, 3))))
        assert b == 4 * (n * Cc * (841 + 169 + 36 + 16) + parts)


def test_shift_table_is_pixel_route_s(lib, tmp_path):
    from tests import pixel_route_model as prm

    host = np.zeros((7, 64, 4), np.int32)
    assert lib.tdmpc2_pixgrad_shift_table(host.ctypes.data_as(C.c_void_p)) == OK
    lo, hi, w0, w1 = prm.shift_table(prm.build(str(tmp_path)))
    assert np.array_equal(host[..., 0], lo) and np.array_equal(host[..., 1], hi)
    assert np.array_equal(host[..., 2].view(np.float32), w0) and np.array_equal(host[..., 3].view(np.float32), w1)


def test_no_cpu_fallback_and_surface():
    import torch

    from tdmpc2_amd import TDMPC2, autograd, layers, native
    from tdmpc2_amd.world_model import WorldModel

    assert isinstance(native.PIXEL_GRAD_CALLS, int)
    before = native.PIXEL_GRAD_CALLS
    seq = layers.conv((3, 64, 64), 8, act=layers.SimNorm(8))
    obs, shift = torch.zeros(2, 3, 64, 64, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(native.NativeError, match="MI355X only"):
        autograd.pixel_encode(seq, obs, shift)
    with pytest.raises(native.NativeError, match="seq must be layers.conv"):
        autograd.pixel_encode(layers.conv((3, 64, 64), 8), obs, shift)
    with pytest.raises(native.NativeError, match="lives on an MI355X"):
        native.pixgrad_shift_table("cpu")
    d = native.pixgrad_desc(2, 3, 8)
    a, f, b = (torch.zeros(x // 4) for x in native.pixgrad_workspace_bytes(d))
    Ws, bs = [seq[i].weight.detach() for i in (2, 4, 6, 8)], [seq[i].bias.detach() for i in (2, 4, 6, 8)]
    with pytest.raises(native.NativeError, match="MI355X only"):
        native.pixgrad_forward(d, obs, shift, torch.zeros(7, 64, 4, dtype=torch.int32), Ws, bs, f, a)
    with pytest.raises(native.NativeError, match="MI355X only"):
        native.pixgrad_backward(d, obs, shift, torch.zeros(7, 64, 4, dtype=torch.int32), Ws, a, torch.zeros(2, 128), b,
                                [torch.zeros_like(w) for w in Ws], [torch.zeros_like(x) for x in bs])
    with pytest.raises(native.NativeError, match="acts / fwd_ws hold"):
        native.pixgrad_forward(d, obs, shift, torch.zeros(7, 64, 4, dtype=torch.int32), Ws, bs, f, a[:-1])
    assert native.PIXEL_GRAD_CALLS == before and issubclass(autograd.PixelEncoderFn, torch.autograd.Function)
    assert isinstance(TDMPC2.native_pixel_grad, property)
    src = open(os.path.join(ROOT, "tdmpc2_amd", "world_model.py")).read()
    assert "self.native_pixel_grad = False" in src and hasattr(WorldModel, "_encode_pixels")


def test_the_flag_defaults_to_off_and_off_is_the_module():
    import torch

    from tdmpc2_amd import TDMPC2
    from tdmpc2_amd.config import named_config

    cfg = named_config("c1", horizon=3)
    cfg.latent_dim, cfg.num_channels, cfg.obs = 16 * 8, 8, "rgb"
    cfg.obs_shape = {"rgb": (3, 64, 64)}
    agent = TDMPC2(cfg, device="cpu")
    assert agent.native_pixel_grad is False and agent.model.native_pixel_grad is False
    obs = torch.randint(0, 256, (2, 3, 64, 64), dtype=torch.uint8)
    torch.manual_seed(1)
    want = agent.model._encoder["rgb"](obs)
    torch.manual_seed(1)
    assert torch.equal(agent.model.encode(obs, None), want)
    agent.native_pixel_grad = True
    assert agent.model.native_pixel_grad is True
    torch.manual_seed(1)
    assert torch.equal(agent.model.encode(obs, None), want)  # a CPU input keeps the module, flag or not
