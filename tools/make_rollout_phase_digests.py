"""Mint tests/golden/rollout_phase_digests.json: SHA-256 digests of what the per-tile rollout path returns on the rows of
tests/rollout_phase_rows.py (bias sources, Philox-mode action blocks at every padding, episodic, exact fp32, a one-step
rollout).  It pins the outputs to the commit that minted the file, so that a change of the phases between the rollout kernel's
GEMMs is compared with that commit and not only with itself.  Public Python API only.  MI355X box, library of COMMIT
(TDMPC2_PLAN_LIB points at it when it is not the tree's own):

    python tools/make_rollout_phase_digests.py COMMIT out_a.json      # one process
    python tools/make_rollout_phase_digests.py COMMIT out_b.json      # a second one
    python tools/make_rollout_phase_digests.py --merge out_a.json out_b.json [tests/golden/rollout_phase_digests.json]

Every row runs the per-tile kernel (no waits between workgroups), so a row that differs between two runs of one library is an
error."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import rollout_phase_rows as pr  # noqa: E402


def mint(commit, out):
    rows = {rid: pr.run_row(rid) for rid in pr.ROWS}
    with open(out, "w") as f:
        json.dump({"commit": commit, "rows": rows}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out, len(rows), "rows")


def merge(a, b, out):
    with open(a) as f:
        ja = json.load(f)
    with open(b) as f:
        jb = json.load(f)
    assert ja["commit"] == jb["commit"], "the two runs are of different commits"
    bad = sorted(k for k in pr.ROWS if ja["rows"].get(k) is None or ja["rows"].get(k) != jb["rows"].get(k))
    assert not bad, f"rows differ between two runs of one library: {bad}"
    with open(out, "w") as f:
        json.dump({"commit": ja["commit"], "rows": ja["rows"]}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out, len(ja["rows"]), "rows, two runs agree")


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else pr.GOLDEN)
    else:
        mint(sys.argv[1], sys.argv[2])
