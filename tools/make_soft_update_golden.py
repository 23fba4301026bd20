"""Mint tests/golden/soft_update_tiny.npz from the reference's own WorldModel.soft_update_target_Q (common/world_model.py:82-86),
run verbatim through oracle/ref_runner.py (needs the reference tree; the committed fixture is what the tests read).

    python tools/make_soft_update_golden.py [out.npz]

Three updates (tau = 0.01) of the `tiny` case's target ensemble (tests/refresh_common.py: tiny_inputs).  Per step k = 1..3 and
tensor: `t32.k/<key>` -- the reference in fp32, continuing from its own step k - 1; `r64.k/<key>` -- the reference in fp64
started from the fp32 tensors of step k - 1, as its distance from `t32.k` in units of the gate (refresh_common.encode64).
Data only: the digests of the seeded inputs and the tensors after each step."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_runner  # noqa: E402
from tests import refresh_common as rc  # noqa: E402


class _Params(dict):
    """What the reference's TensorDictParams does for lerp_: the in-place torch op on every leaf."""

    def lerp_(self, end, weight):
        for k, v in self.items():
            v.lerp_(end[k], weight)
        return self


def reference_update(target, online, tau, dtype):
    ref = ref_runner._import_reference()
    wm = types.SimpleNamespace(cfg=types.SimpleNamespace(tau=tau),
                               _target_Qs_params=_Params({k: torch.tensor(v, dtype=dtype) for k, v in target.items()}),
                               _detach_Qs_params=_Params({k: torch.tensor(v, dtype=dtype) for k, v in online.items()}))
    ref.WorldModel.soft_update_target_Q(wm)
    return {k: v.numpy() for k, v in wm._target_Qs_params.items()}


def main(out):
    target, online = rc.tiny_inputs()
    rec = {"digest.target": np.array(rc.digest(target)), "tau": np.array(rc.TAU, np.float64)}
    cur = target
    for k in range(1, rc.STEPS + 1):
        o = online[k - 1]
        rec[f"digest.online.{k}"] = np.array(rc.digest(o))
        t32 = reference_update(cur, o, rc.TAU, torch.float32)
        t64 = reference_update(cur, o, rc.TAU, torch.float64)
        for key in rc.Q_KEYS:
            sc = rc.scale_of(cur[key], o[key])
            r16 = rc.encode64(t64[key], t32[key], sc)
            assert np.all(np.abs(rc.decode64(t32[key], r16, sc) - t64[key]) <= rc.TAIL_ERR * sc), key
            rec[f"t32.{k}/{key}"], rec[f"r64.{k}/{key}"] = t32[key], r16
        cur = t32
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", rc.GOLDEN))
