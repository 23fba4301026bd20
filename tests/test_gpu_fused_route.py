"""-m gpu: the fused family's host path, bit for bit against the commit before it moved onto fused_route.h.

tests/golden/fused_plan_digests.json (tools/make_fused_plan_digests.py, two runs of that commit's library that agreed on every
row kept) holds the SHA-256 of what each call of tests/fused_plan_rows.py returns: action, prev_mean and the six debug stages of
tape-driven plans on every route -- two clusters per tile, one cluster, per tile (E = 1); an episodic cluster plan; forced 32-row
workgroups with the refit folded and forced 64-row ones with k_refit; both sides of the automatic 32 / 64-row switch; a multitask
call -- the value, activation tiles and scalars of a trace call, and a sharded plan evaluated in two row ranges.  Launching what
the route says with the parameter values the inline code passed leaves every one of these bits where it was."""
import json
import os

import pytest

from tests import fused_plan_rows as fr

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_plan_digests.json")) as f:
    GOLDEN = json.load(f)


def test_the_golden_file_has_the_rows_it_must():
    """only rows of the cluster routes may be missing (dropped by the mint when two runs of one library differed)"""
    assert set(GOLDEN["rows"]) <= set(fr.ROWS)
    assert set(fr.ROWS) - set(GOLDEN["rows"]) <= set(fr.CLUSTER_ROWS)
    assert sorted(GOLDEN["dropped"]) == sorted(set(fr.ROWS) - set(GOLDEN["rows"]))


@pytest.mark.parametrize("rid", sorted(GOLDEN["rows"]))
def test_the_call_returns_the_bits_it_returned_before(rid):
    assert fr.run_row(rid) == GOLDEN["rows"][rid], (rid, "minted from", GOLDEN["commit"])
