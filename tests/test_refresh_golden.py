"""CPU: tests/golden/soft_update_tiny.npz -- the reference's own WorldModel.soft_update_target_Q in fp32 against itself in fp64 --
meets the gate the GPU test sets for the library's soft update, |out - ref64| <= 2^-23 (|t| + |o|), on every element of every
step: the gate can be met by the reference alone.  The seeded inputs the GPU test rebuilds are the ones the fixture was minted from."""
import os

import numpy as np
import pytest

from tests import refresh_common as rc

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", rc.GOLDEN)


@pytest.fixture(scope="module")
def golden():
    return np.load(PATH)


@pytest.fixture(scope="module")
def inputs():
    return rc.tiny_inputs()


def test_fixture_inputs_are_the_seeded_ones(golden, inputs):
    target, online = inputs
    assert str(golden["digest.target"]) == rc.digest(target)
    for k in range(1, rc.STEPS + 1):
        assert str(golden[f"digest.online.{k}"]) == rc.digest(online[k - 1])
    assert float(golden["tau"]) == rc.TAU


def test_reference_fp32_meets_the_gate_against_its_fp64(golden, inputs):
    cur, online = inputs
    worst = -np.inf
    for k in range(1, rc.STEPS + 1):
        nxt = {}
        for key in rc.Q_KEYS:
            t, o, out = cur[key], online[k - 1][key], golden[f"t32.{k}/{key}"]
            assert out.dtype == np.float32 and out.shape == t.shape
            s = rc.scale_of(t, o)
            ref = rc.decode64(out, golden[f"r64.{k}/{key}"], s)
            # the decoded fp64 is the reference's, not a restatement: it agrees with numpy's fp64 lerp of the same inputs to fp64 round-off
            assert np.max(np.abs(ref - rc.lerp64(t, o, rc.TAU)) - rc.TAIL_ERR * s) <= 0.0
            worst = max(worst, rc.gate_excess(out, ref, t, o, slack=rc.TAIL_ERR))
            nxt[key] = out
        cur = nxt
    print(f"reference fp32 vs fp64: worst excess over the gate {worst:.3e} (<= 0 passes)")
    assert worst <= 0.0
