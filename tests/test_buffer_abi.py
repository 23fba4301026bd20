"""CPU: the replay buffer's additions to ABI 14 (include/tdmpc2_plan.h: tdmpc2_buffer_*).  The version stays 14; every new symbol
is declared, bound, documented and exported; the structs match the header; and every refusal comes with its code and message
before the device is touched (create never touches it: the storage is allocated by the first write)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("tdmpc2_buffer_create", "tdmpc2_buffer_destroy", "tdmpc2_buffer_add", "tdmpc2_buffer_load", "tdmpc2_buffer_sample",
           "tdmpc2_buffer_stats", "tdmpc2_buffer_set_call_counter")
OK, INVALID, UNSUPPORTED, HIP, STATE = range(5)


@pytest.fixture(scope="module")
def lib():
    from tdmpc2_amd import native

    return native.load_library()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tdmpc2_plan.h")).read(), flags=re.S)


def test_version_and_symbols(lib):
    from tdmpc2_amd import native

    hdr = _header()
    assert re.search(r"#define\s+TDMPC2_PLAN_ABI_VERSION\s+14\b", hdr) and native.ABI_VERSION == 14
    assert lib.tdmpc2_plan_abi_version() == 14
    declared = set(re.findall(r"\b(tdmpc2_[a-z_]+)\s*\(", hdr))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert s in declared, s
        assert s in native.ABI_SYMBOLS, s
        assert f"`{s}" in doc, s
        assert hasattr(lib, s), s
    assert {s for s in declared if s.startswith("tdmpc2_buffer_")} == set(SYMBOLS)


def test_struct_sizes_match_the_header(tmp_path):
    """The header's own sizeof / offsetof, from the host compiler, against the ctypes structures."""
    import subprocess

    from tdmpc2_amd import native

    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tdmpc2_plan.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(tdmpc2_buffer_field), sizeof(tdmpc2_buffer_cfg), sizeof(tdmpc2_buffer_info),\n'
                   '         offsetof(tdmpc2_buffer_cfg, max_batch), offsetof(tdmpc2_buffer_cfg, field), offsetof(tdmpc2_buffer_info, eligible),\n'
                   '         (size_t)TDMPC2_BUFFER_MAX_FIELDS);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(native.BufferField), C.sizeof(native.BufferCfg), C.sizeof(native.BufferInfo),
                   native.BufferCfg.max_batch.offset, native.BufferCfg.field.offset, native.BufferInfo.eligible.offset,
                   native.BUFFER_MAX_FIELDS]
    assert got[:3] == [12, 24 + 8 * 12, 32]


def _create(lib, capacity=10, slice_len=4, fields=((20, 0, 4), (4, 1, 3)), n_fields=None, max_batch=0, device=0):
    from tdmpc2_amd import native

    cfg = native.buffer_cfg(capacity, slice_len, list(fields), device, max_batch)
    if n_fields is not None:
        cfg.n_fields = n_fields
    h = C.c_void_p()
    rc = lib.tdmpc2_buffer_create(C.byref(cfg), C.byref(h))
    return rc, lib.tdmpc2_last_error().decode(), h


def test_create_refusals(lib):
    assert lib.tdmpc2_buffer_create(None, None) == INVALID and b"null" in lib.tdmpc2_last_error()
    for kw, word in ((dict(capacity=3), "capacity 3 < slice_len 4"), (dict(slice_len=1, fields=((4, 0, 1),)), "slice_len 1 < 2"),
                     (dict(n_fields=0), "n_fields 0"), (dict(n_fields=9), "n_fields 9"),
                     (dict(fields=((20, 0, 4), (0, 1, 3))), "field 1 has row_bytes 0"),
                     (dict(fields=((20, 0, 5),)), "outside the slice"), (dict(fields=((20, 2, 3),)), "outside the slice"),
                     (dict(fields=((20, -1, 2),)), "outside the slice"), (dict(fields=((20, 0, 0),)), "outside the slice"),
                     (dict(max_batch=-1), "max_batch")):
        rc, msg, h = _create(lib, **kw)
        assert rc == INVALID and word in msg and not h.value, (kw, rc, msg)


def test_call_refusals_come_before_the_device(lib):
    from tdmpc2_amd import native

    P2 = C.c_void_p * 2
    good = P2(256, 256)  # never dereferenced: every call below is refused first
    for name, args in (("tdmpc2_buffer_add", (None, 1, good, None)), ("tdmpc2_buffer_load", (None, 1, 1, good, None)),
                       ("tdmpc2_buffer_sample", (None, 1, good, None, 0, None)), ("tdmpc2_buffer_set_call_counter", (None, 0, None))):
        assert getattr(lib, name)(*args) == INVALID and b"null" in lib.tdmpc2_last_error(), name
    assert lib.tdmpc2_buffer_stats(None, C.byref(native.BufferInfo()), None) == INVALID
    lib.tdmpc2_buffer_destroy(None)  # a no-op
    rc, msg, h = _create(lib, max_batch=8)
    assert rc == OK and h.value  # create sizes and validates only: it works without a device
    try:
        err = lambda: lib.tdmpc2_last_error().decode()  # noqa: E731
        assert lib.tdmpc2_buffer_stats(h, None, None) == INVALID and "null" in err()
        assert lib.tdmpc2_buffer_add(h, 4, None, None) == INVALID and "null" in err()
        assert lib.tdmpc2_buffer_add(h, 4, P2(256, None), None) == INVALID and "null pointer for field 1" in err()
        assert lib.tdmpc2_buffer_add(h, 0, good, None) == INVALID and "at least one" in err()
        assert lib.tdmpc2_buffer_load(h, 0, 4, good, None) == INVALID and "at least one" in err()
        assert lib.tdmpc2_buffer_add(h, 11, good, None) == INVALID and "longer than the capacity of 10" in err()
        assert lib.tdmpc2_buffer_load(h, 3, 11, good, None) == INVALID and "longer than the capacity of 10" in err()
        assert lib.tdmpc2_buffer_sample(h, 2, None, None, 0, None) == INVALID and "null" in err()
        for batch in (0, -1, 9):
            assert lib.tdmpc2_buffer_sample(h, batch, good, None, 0, None) == INVALID and f"batch {batch} outside [1, 8]" in err()
        assert lib.tdmpc2_buffer_sample(h, 2, good, None, 0, None) == STATE and "no episode" in err()
        info = native.BufferInfo()
        assert lib.tdmpc2_buffer_stats(h, C.byref(info), None) == OK
        assert (info.num_eps, info.live_steps, info.cursor, info.eligible, info.next_call) == (0, 0, 0, 0, 0)
        assert lib.tdmpc2_buffer_set_call_counter(h, 41, None) == OK  # before the first write: carried over by it
        assert lib.tdmpc2_buffer_stats(h, C.byref(info), None) == OK and info.next_call == 41
    finally:
        lib.tdmpc2_buffer_destroy(h)


def test_no_host_storage():
    import torch

    from tdmpc2_amd import Buffer
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.native import NativeBuffer, NativeError

    with pytest.raises(NativeError, match="no host storage"):
        NativeBuffer(10, 4, [(4, 0, 4)], torch.device("cpu"))
    cfg = named_config("tiny")
    assert (cfg.buffer_size, cfg.steps, cfg.batch_size) == (1_000_000, 10_000_000, 256)  # the reference's config.yaml
    with pytest.raises(NativeError, match="no host storage"):
        Buffer(cfg, device="cpu")


def test_a_write_that_cannot_reach_its_device_leaves_the_handle_unchanged(lib):
    from tdmpc2_amd import native

    rc, _, h = _create(lib, device=9999)  # an ordinal no machine has: with or without a GPU the first write fails before it allocates
    assert rc == OK
    try:
        good = (C.c_void_p * 2)(256, 256)
        assert lib.tdmpc2_buffer_add(h, 4, good, None) == HIP  # nothing allocated, nothing written, the ring as it was
        info = native.BufferInfo()
        assert lib.tdmpc2_buffer_stats(h, C.byref(info), None) == OK and (info.num_eps, info.cursor, info.eligible) == (0, 0, 0)
    finally:
        lib.tdmpc2_buffer_destroy(h)
