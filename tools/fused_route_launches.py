"""The fused family's launches per call, as the GPU saw them: the source of profiles/fused_route_launches.txt, which
tests/test_fused_route.py holds fused_route.h to.  Two steps, MI355X box:

    rocprofv3 --kernel-trace --output-format csv -d D -o t -- python tools/fused_route_launches.py run D/calls.txt
    python tools/fused_route_launches.py list D/calls.txt D/<...>/t_kernel_trace.csv profiles/fused_route_launches.txt

`run` makes one tape = NULL plan per (case, E, cluster, rows, fold) of CALLS x TUNING and writes their order; `list` cuts the
trace's dispatches of ks_* / k_refit at every ks_setup (each plan starts with exactly one) and writes one line per plan:
    case E cluster rows fold | ks_setup<..> grid workgroup ; [ks_pitraj<..> grid workgroup ;] I x [rollout kernel<..> grid workgroup [; k_refit grid workgroup]]
(grid in workgroups, workgroup in threads; the launches of one CEM iteration are written once, with the number of iterations)."""
import csv
import itertools
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = [("c1", 1), ("c1", 3), ("c1", 16), ("c1", 32), ("c1", 33), ("c1", 256), ("c2_i6", 1), ("c2_i6", 256), ("c2_ep", 1), ("mt5", 5)]
TUNING = list(itertools.product((0, 1, 2), (32, 64, 0), (0, 1, 2)))  # cluster, rows (0 = auto), fold


def run(order_path):
    import torch

    from oracle import cases
    from oracle import planner_oracle as po
    from tdmpc2_amd.native import NativePlanner
    from tests.gpu_common import dev
    from tests.test_gpu_philox import _many_env_inputs

    with open(order_path, "w") as f:
        for name, E in CALLS:
            c = cases.build_case(name)
            model = po.OracleModel(c["cfg"], {k: torch.as_tensor(v) for k, v in c["sd"].items()})
            planner = NativePlanner(c["cfg"], c["iterations"], dev(), max_envs=E, path=1)
            planner.bind_state_dict(model.sd)
            inp = _many_env_inputs(c, model, E)
            for cluster, rows, fold in TUNING:
                planner.set_cluster(cluster)
                planner.set_rows_per_workgroup(rows)
                planner.set_fold_refit(fold)
                planner.plan(inp["z0"], inp["disc_pow"], inp["prev_mean"].clone(), inp["t0"], task_emb=inp["task_emb"],
                             act_mask=inp["act_mask"], seed=5)
                torch.cuda.synchronize()
                assert planner.take_fault() == 0
                f.write(f"{name} {E} {cluster} {rows} {fold}\n")
                f.flush()
            planner.close()


def short(name):
    """ks_rollout<16, 2, 8, 0, 0, 0>(...) -> ks_rollout<16,2,8,0,0,0>; the parameter block's type is dropped."""
    m = re.search(r"\b(ks_\w+|k_refit)\b(<[^>]*>)?", name)
    return m.group(1) + (m.group(2) or "").replace(" ", "")


def list_(order_path, trace_csv, out):
    with open(order_path) as f:
        calls = [ln.strip() for ln in f if ln.strip()]
    with open(trace_csv) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    plans = []
    for r in rows:
        if not re.search(r"\b(ks_setup|ks_pitraj|ks_rollout\w*|k_refit)\b", r["Kernel_Name"]):
            continue
        k = short(r["Kernel_Name"])
        if k.startswith("ks_setup"):
            plans.append([])
        wg = int(r["Workgroup_Size_X"])
        plans[-1].append(f"{k} {int(r['Grid_Size_X']) // wg} {wg}")
    assert len(plans) == len(calls), (len(plans), len(calls))
    with open(out, "w") as f:
        for call, launches in zip(calls, plans):
            n0 = sum(1 for k in launches if k.startswith(("ks_setup", "ks_pitraj")))
            head, body = launches[:n0], launches[n0:]
            unit = next(body[:u] for u in (1, 2, len(body)) if body[:u] * (len(body) // u) == body)
            f.write(f"{call} | {' ; '.join(head)} ; {len(body) // len(unit)} x [{' ; '.join(unit)}]\n")
    print(out, len(calls), "calls")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        list_(sys.argv[2], sys.argv[3], sys.argv[4])
