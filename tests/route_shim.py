"""What the *_common.py helpers of the route headers share: the host compiler's command line, the two builds of a header's C shim
(a library loaded with its prototypes declared; a stand-alone program with its own main, optionally under AddressSanitizer and
UBSan, run directly with nothing preloaded), the numpy restatement of the 256-thread ordered sum and the measured gate."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "tdmpc2_amd", "csrc")]
MARGIN, FLOOR = 4.0, 2.0 ** -23  # the measured gate of DESIGN 3.4h: e <= MARGIN * max(e_torch32, FLOOR)


def build_shim(tmpdir, stem, source, prototypes, extra_flags=()):
    """`source` as lib<stem>_shim.so -> the loaded library; prototypes: name -> argtypes, or (argtypes, restype)."""
    src = os.path.join(str(tmpdir), stem + "_shim.cpp")
    with open(src, "w") as f:
        f.write(source)
    so = os.path.join(str(tmpdir), "lib" + stem + "_shim.so")
    subprocess.run([*CXX, *extra_flags, "-shared", "-fPIC", src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    for name, sig in prototypes.items():
        fn = getattr(lib, name)
        if isinstance(sig, tuple):
            fn.argtypes, fn.restype = sig
        else:
            fn.argtypes = sig
    return lib


def build_walk(tmpdir, stem, source, sanitize=False):
    """`source` (a shim and its MAIN) as one stand-alone program -> its path.  sanitize: built with -fsanitize=address,undefined."""
    src = os.path.join(str(tmpdir), stem + "_walk.cpp")
    with open(src, "w") as f:
        f.write(source)
    exe = os.path.join(str(tmpdir), stem + "_walk")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run([*CXX, *flags, src, "-o", exe], check=True)
    return exe


def ordered_sum_model(src):
    """seed_ordered_sum (seed_route.h) in numpy: thread-strided partials from 0 in rising order, then the in-place halving tree."""
    src = np.asarray(src, np.float32)
    rounds = -(-src.size // 256)
    p = np.zeros(rounds * 256, np.float32)
    p[:src.size] = src
    red = np.zeros(256, np.float32)
    for k in range(rounds):
        red = red + p[k * 256:(k + 1) * 256]
    w = 128
    while w > 0:
        red[:w] = red[:w] + red[w:2 * w]
        w //= 2
    return red[0]


def rel_err(got, ref):
    """e(T) = max |T - T64| / max |T64|."""
    ref = np.asarray(ref, np.float64)
    den = float(np.abs(ref).max())
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / (den if den > 0 else 1.0)


def gate(got, ref64, yard32):
    """e and the bound MARGIN * max(e_torch32, FLOOR) of one tensor."""
    return rel_err(got, ref64), MARGIN * max(rel_err(yard32, ref64), FLOOR)
