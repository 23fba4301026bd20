"""tdmpc2_amd/csrc/model_route.h itself, compiled with g++ behind the C shim below, and an INDEPENDENT Python statement of what
a model rollout / loss call has to launch (stages from the outputs asked for).  Used by tests/test_model_route.py."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include "model_route.h"
// out: refuse, nchain, launches, chain[9], then per stage run, gx, gy, gz, rows, steps, chunks, launches, produces
extern "C" void route(int family, int B, int H, int nq, int nb, int episodic, unsigned want, long cap, int ln_after, long *out) {
    const ModelRoute r = model_route(ModelIn{family, B, H, nq, nb, episodic, want, cap, ln_after});
    out[0] = r.refuse; out[1] = r.nchain; out[2] = r.launches;
    for (int i = 0; i < 1 + MODEL_MAXQ; ++i) out[3 + i] = r.chain[i];
    for (int s = 0; s < MS_COUNT; ++s) {
        long *o = out + 12 + 9 * s;
        const ModelStage &t = r.st[s];
        o[0] = t.run; o[1] = t.gx; o[2] = t.gy; o[3] = t.gz; o[4] = t.rows; o[5] = t.steps; o[6] = t.chunks; o[7] = t.launches; o[8] = t.produces;
    }
}
extern "C" long rowloss_floats(int B, int H, int nq) { return model_rowloss_floats(B, H, nq); }
"""
FUSED, LAYERED = 0, 1
ZS, REW_LOGITS, REW, Q_LOGITS, Q, TERM, LOSSES = 1, 2, 4, 8, 16, 32, 64
DYN, HEADS, TERM_STAGE, CONS, TAIL = range(5)
MC_TERM = 100
OK, BAD_H, BAD_B, NOT_EPISODIC, ROWS, NO_BINS, LOSSES_H0 = range(7)
TILE = 64


def build(tmpdir):
    src = os.path.join(str(tmpdir), "model_route_shim.cpp")
    with open(src, "w") as f:
        f.write(SHIM)
    so = os.path.join(str(tmpdir), "libmodel_route_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tdmpc2_amd", "csrc"), src, "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    ci = ctypes.c_int
    lib.route.argtypes = [ci, ci, ci, ci, ci, ci, ctypes.c_uint, ctypes.c_long, ci, ctypes.POINTER(ctypes.c_long)]
    lib.rowloss_floats.restype = ctypes.c_long
    return lib


def route(lib, family, B, H, nq, nb, episodic, want, cap, ln_after=0):
    out = (ctypes.c_long * (12 + 9 * 5))()
    lib.route(family, B, H, nq, nb, int(episodic), want, cap, int(ln_after), out)
    keys = ("run", "gx", "gy", "gz", "rows", "steps", "chunks", "launches", "produces")
    st = [dict(zip(keys, out[12 + 9 * s:21 + 9 * s])) for s in range(5)]
    return {"refuse": out[0], "chain": list(out[3:3 + out[1]]), "launches": out[2], "st": st}


def expected(family, B, H, nq, nb, episodic, want, cap):
    """What has to run, stated from the reference's data flow (tdmpc2.py:268-304), not from the header."""
    losses = bool(want & LOSSES)
    if not 0 <= H <= 8:
        return {"refuse": BAD_H}
    if B < 1:
        return {"refuse": BAD_B}
    if losses and H < 1:
        return {"refuse": LOSSES_H0}
    if losses and nb < 2:
        return {"refuse": NO_BINS}
    if (want & TERM) and not episodic:
        return {"refuse": NOT_EPISODIC}
    if family == LAYERED and (H * B > cap or B > cap):
        return {"refuse": ROWS}
    chains = []
    if H > 0 and (losses or want & (REW_LOGITS | REW)):
        chains.append(0)
    if H > 0 and (losses or want & (Q_LOGITS | Q)):
        chains += [1 + i for i in range(nq)]
    term = bool(want & TERM) or (losses and episodic)
    # latents needed: zs[H] by zs / termination / consistency; the chains read zs[0 .. H-1]
    last_z = H if (want & ZS or term or losses) else (H - 1 if chains else 0)
    return {"refuse": OK, "chains": chains, "term": term, "steps": last_z, "losses": losses}


def expected_launches(family, B, H, nq, episodic, want, cap, ln_after):
    """Kernel launches of an accepted call, counted from the launch sequences of plan_train.hip / model_layered_host.cuh."""
    e = expected(family, B, H, nq, 101, episodic, want, cap)
    n = 2 if e["losses"] else 0                       # consistency rows, tail
    if family == FUSED:
        return n + (e["steps"] > 0) + bool(e["chains"]) + e["term"]
    normed = 2 if ln_after else 1                     # a NormedLinear: GEMM (+ LayerNorm row kernel)
    chain = 2 * normed + 1 + 1                        # two hidden layers, head GEMM, row kernel
    if e["steps"]:
        n += 1 + e["steps"] * (1 + 3 * normed + 1)    # init; per step: actions, three NormedLinear layers, latent out
    if e["chains"]:
        n += 2 + len(e["chains"]) * chain             # init rows, actions, the chains
    if e["term"]:
        n += -(-(H + 1) * B // cap) * (1 + chain)     # per piece: init rows, the chain
    return n
