"""Generator of tests/golden/update_steps.npz: K iterations of the reference's OWN `TDMPC2._update` (tdmpc2/tdmpc2.py:259-332, with
`update_pi` and `_td_target` under it) on one batch per case, run verbatim on the CPU by oracle/ref_runner.py:
run_reference_updates -- in fp64, in fp32, and in fp64 once per deliberately wrong control.  What is restated there (the two
optimisers, RunningScale's constructor, the soft update, `_detach_Qs`) is listed in its docstring; the cases, the seeded inputs and
the key layout are tests/update_common.py's.  One thread: the same reduction order on every machine.

    python tools/make_update_golden.py
"""
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import update_common as uc  # noqa: E402


def _infos(run, keys):
    assert all(tuple(i) == keys for i in run["infos"]), (run["infos"][0].keys(), keys)
    return np.asarray([[i[k] for k in keys] for i in run["infos"]], np.float64)


def generate_case(case_id):
    from oracle import ref_runner

    cfg, sd = uc.build(case_id)
    batch, pins = uc.inputs(case_id, cfg)
    keys = uc.info_keys(cfg)
    res = {f"{case_id}.{k}": v for k, v in {**batch, **pins}.items()}
    run = lambda dtype, control=None: ref_runner.run_reference_updates(  # noqa: E731
        cfg, sd, batch, pins, uc.K, dtype, uc.SCALE0, control=control)
    r64, r32 = run(torch.float64), run(torch.float32)
    assert r64["td"].dtype == np.float64 and r32["td"].dtype == np.float32
    res[f"{case_id}.info64"], res[f"{case_id}.info32"] = _infos(r64, keys), _infos(r32, keys)
    res[f"{case_id}.td64"], res[f"{case_id}.td32"] = r64["td"], r32["td"]
    if cfg.episodic:
        res[f"{case_id}.term_logit64"] = r64["term_logit"]
    for control in uc.controls_of(cfg):
        rc = run(torch.float64, control)
        res[f"{case_id}.{control}.info64"], res[f"{case_id}.{control}.td64"] = _infos(rc, keys), rc["td"]
    return res


def generate(case_ids=None):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        res = {"scale0": np.float64(uc.SCALE0)}
        for case_id in (case_ids or uc.CASES):
            res.update(generate_case(case_id))
        return res
    finally:
        torch.set_num_threads(threads)


def main():
    from oracle import ref_runner

    if not ref_runner.available():
        raise SystemExit("the reference tree is not available: nothing to generate")
    res = generate()
    buf = io.BytesIO()
    np.savez_compressed(buf, **res)
    with open(uc.GOLDEN, "wb") as f:
        f.write(buf.getvalue())
    print(f"wrote {uc.GOLDEN}: {len(buf.getvalue())} bytes, {len(res)} arrays")
    g = uc.golden()
    for case_id in uc.CASES:
        cfg, _ = uc.build(case_id)
        keys = uc.info_keys(cfg)
        print(case_id, {k: (None if b is None else float(f"{b:.3g}")) for k, b in uc.info_bounds(g, case_id, keys).items()})
        print("   pi_scale", g[f"{case_id}.info64"][:, keys.index("pi_scale")])
        for control in uc.controls_of(cfg):
            print("   ", control, "%.3g at %s" % uc.control_margin(g, case_id, control, keys))


if __name__ == "__main__":
    main()
