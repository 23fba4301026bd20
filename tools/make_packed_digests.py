"""Mint tests/golden/packed_digests.json: SHA-256 digests of the packed weight storage (tdmpc2_plan_export_packed), one per
segment owner (a net, or the state encoder), for the five (case, path, precision) rows of tests/test_gpu_refresh.py and the six
weight sets of tests/refresh_common.py: packed_inputs.  It pins the bytes the packer stores, so that a change of the packer is
compared with the commit that minted the file and not only with itself.  Public Python API only (bind_state_dict +
bind_encoder, export_packed): the tool runs unchanged on any commit that has them.  MI355X box:

    python tools/make_packed_digests.py COMMIT [out.json]

COMMIT is recorded as the commit whose library produced the bytes.  A second handle filled by refresh_state_dict must give the
same digests; the tool refuses to write a file otherwise."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from oracle import cases  # noqa: E402
from tests import refresh_common as rc  # noqa: E402


def main(commit, out):
    from tdmpc2_amd.native import NativePlanner

    dev = torch.device("cuda", 0)
    rows = {}
    for (name, path, prec), rid in zip(rc.CASES, rc.IDS):
        c = cases.build_case(name)
        A, B = (NativePlanner(c["cfg"], c["iterations"], dev, max_envs=2, path=path, precision=prec) for _ in range(2))
        rows[rid] = {}
        for label, sd in rc.packed_inputs(c, dev):
            A.bind_state_dict(sd)
            A.bind_encoder(sd)
            B.refresh_state_dict(sd)
            owners = rc.owner_digests(A.export_packed(), c["cfg"], prec == 2)
            assert owners == rc.owner_digests(B.export_packed(), c["cfg"], prec == 2), (rid, label, "refresh differs from the binds")
            rows[rid][label] = {"input": rc.sd_digest(sd), "owners": owners}
        A.close()
        B.close()
    with open(out, "w") as f:
        json.dump({"commit": commit, "refresh_gives_the_same": True, "rows": rows}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out, os.path.getsize(out), "bytes;", sum(len(r) for r in rows.values()), "weight sets, binds == refresh on every one")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", rc.PACKED_DIGESTS))
