"""CPU: the counted-wait reports (tools/isa_hazards.py --waits) of the fused family's model kernels, ks_value_roll and
ks_value_chain.  tests/test_isa_hazards.py exempts the ks_value family from the counted-wait model by name, because ks_value inlines
the hand-ordered weight ring (kloop_asm) whose flag-dependent waits the path-insensitive pass cannot follow.  The two new kernels
share that exemption through their name, so this file pins what the exemption covers: every report in them is one the ring
produces in ks_value itself (same counter, same kind of producing load), the exact-fp32 instantiations -- which
have no hand-written ring -- report nothing at all, and nothing but waits is reported.  profiles/model_isa_waits.txt is the
tool's own listing for the three kernels."""
import os
import re

import pytest

from tools import isa_hazards as hz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reports():
    if not os.path.exists(hz.OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    lib = os.path.join(ROOT, "tdmpc2_amd", "libtdmpc2_plan.so")
    if not os.path.exists(lib):
        pytest.skip("library not built (python -c 'import __graft_entry__ as g; g.build()')")
    return hz.scan_library(lib, waits=True)[2]


def _fam(kernel):
    return re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", kernel)


def _mn(text):
    return str(text).split()[0]


def _sig(r):
    """(counter, producing load) of a report.  The consuming instruction is whatever next touches the ring slot's registers on the
    path the model walks, so it differs from kernel to kernel; the producer is what identifies the ring."""
    return (r[1], _mn(r[3]))


def test_model_kernels_report_only_what_the_ring_reports_in_ks_value(reports):
    new = [r for r in reports if _fam(r[0]).startswith(("ks_value_roll", "ks_value_chain"))]
    ring = {_sig(r) for r in reports if _fam(r[0]).startswith("ks_valueILi")}   # ks_value<APAD, AR> itself
    assert ring and new
    assert all(r[1].endswith("-use") for r in new), [r[:2] for r in new if not r[1].endswith("-use")][:3]
    foreign = sorted({_sig(r) for r in new} - ring)
    assert not foreign, foreign
    # the ring's loads are global_load_dwordx4 weight fragments and ds_read_b128 activation fragments feeding MFMAs
    assert {s[1] for s in {_sig(r) for r in new}} <= {"global_load_dwordx4", "ds_read_b128"}
    # exact-fp32 instantiations <APAD, 1> have no hand-written ring: nothing to report
    assert not [r for r in new if re.search(r"ILi\d+ELi1EE", r[0])]
