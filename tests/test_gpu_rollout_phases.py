"""-m gpu: the phases between the rollout kernel's GEMMs keep their bits when they are rescheduled -- the first-layer and hidden-layer
biases staged through LDS one epilogue ahead and z_H held in registers under the policy-prior chain (fused_kernels.cuh) and, as a
variant outside the tree (tools/variants/rollout_action_block.patch, measured slower), the action block with compile-time trip
counts and independent Philox chains.  None of them changes a floating-point operation, an
operand or an order, or a Philox counter, so every plan must return the bits of the commit before:
tests/golden/rollout_phase_digests.json (rows: tests/rollout_phase_rows.py) was minted on that commit's library by
tools/make_rollout_phase_digests.py, two runs that agreed.  The rows are the geometries at which those phases take another path:
multitask plans (beff bias rows, an action mask) with 32- and 64-row workgroups; Philox-mode plans at 16, 32, 48 and 64 action
columns, with and without policy-prior rows; the episodic kernel; exact fp32; a rollout of one step.
"""
import json

import pytest

from tests import rollout_phase_rows as pr

pytestmark = pytest.mark.gpu

with open(pr.GOLDEN) as f:
    GOLDEN = json.load(f)


def test_the_golden_file_has_every_row():
    assert set(GOLDEN["rows"]) == set(pr.ROWS)


@pytest.mark.parametrize("rid", sorted(pr.ROWS))
def test_the_plan_returns_the_bits_of_the_commit_before(rid):
    assert pr.run_row(rid) == GOLDEN["rows"][rid], (rid, "minted from", GOLDEN["commit"])
