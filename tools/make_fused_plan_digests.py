"""Mint tests/golden/fused_plan_digests.json: SHA-256 digests of what the fused family's calls return (action, prev_mean and
the debug stages of tape-driven plans; a trace call; a sharded plan) on each of its host routes -- the rows of
tests/fused_plan_rows.py.  It pins the outputs to the commit that minted the file, so that a change of the fused host path is
compared with that commit and not only with itself.  Public Python API only.  MI355X box, library of COMMIT:

    python tools/make_fused_plan_digests.py COMMIT out_a.json      # one process
    python tools/make_fused_plan_digests.py COMMIT out_b.json      # a second one
    python tools/make_fused_plan_digests.py --merge out_a.json out_b.json [tests/golden/fused_plan_digests.json]

The merge keeps the rows on which the two runs agree.  Only rows of the cluster routes (their hand-overs are waits between
workgroups) may be dropped that way, and it names them; a per-tile row that differs between two runs of one library is an error."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import fused_plan_rows as fr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "fused_plan_digests.json")


def mint(commit, out):
    rows = {rid: fr.run_row(rid) for rid in fr.ROWS}
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
    keep = {k: v for k, v in ja["rows"].items() if jb["rows"].get(k) == v}
    dropped = sorted(set(fr.ROWS) - set(keep))
    bad = [k for k in dropped if k not in fr.CLUSTER_ROWS]
    assert not bad, f"per-tile rows differ between two runs of one library: {bad}"
    with open(out, "w") as f:
        json.dump({"commit": ja["commit"], "dropped": dropped, "rows": keep}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out, len(keep), "rows kept; dropped:", dropped or "none")


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else GOLDEN)
    else:
        mint(sys.argv[1], sys.argv[2])
