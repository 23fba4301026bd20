"""tdmpc2_amd/csrc/refresh_route.h itself, compiled with g++ behind the C shim below.  Used by tests/test_refresh_route.py."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include "refresh_route.h"
// out: nops, op[4], nets, enc_layers, policy_copy, REFRESH_MAX_OPS
extern "C" void route(int split, unsigned nets, int enc_layers, int policy_copy, int lerp, int num_q, int episodic, int policy_alone,
                      int *out) {
    const RefreshRoute r = refresh_route(RefreshIn{split, nets, enc_layers, policy_copy, lerp, num_q, episodic, policy_alone});
    out[0] = r.nops;
    for (int i = 0; i < REFRESH_MAX_OPS; ++i) out[1 + i] = i < r.nops ? r.op[i] : -1;
    out[5] = (int)r.nets; out[6] = r.enc_layers; out[7] = r.policy_copy; out[8] = REFRESH_MAX_OPS;
}
extern "C" int scan_wblocks(long n) { return rf_scan_wblocks(n); }
extern "C" int pack_blocks(int ct, int kp, int nt) { return rf_pack_blocks(ct, kp, nt); }
extern "C" int transpose_blocks(int out, int in) { return rf_transpose_blocks(out, in); }
"""
RESET, SCAN, SCALES, PACK = range(4)
DYN, REW, PI, Q, TERM, TQ = (1 << i for i in range(6))


def build(tmpdir):
    src = os.path.join(str(tmpdir), "refresh_route_shim.cpp")
    with open(src, "w") as f:
        f.write(SHIM)
    so = os.path.join(str(tmpdir), "librefresh_route_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tdmpc2_amd", "csrc"), src, "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.scan_wblocks.argtypes = [ctypes.c_long]
    return lib


def route(lib, split, nets, enc_layers=0, policy_copy=0, lerp=0, num_q=5, episodic=0, policy_alone=0):
    out = (ctypes.c_int * 9)()
    lib.route(int(split), nets, enc_layers, int(policy_copy), int(lerp), num_q, int(episodic), int(policy_alone), out)
    return {"ops": list(out[1:1 + out[0]]), "nets": out[5], "enc_layers": out[6], "policy_copy": out[7], "max_ops": out[8]}
