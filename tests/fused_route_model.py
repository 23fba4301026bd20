"""The fused family's launch routes from tdmpc2_amd/csrc/fused_route.h itself, compiled with g++ behind the C shim below (as
tests/policy_route_model.py does for policy_route.h); the handle's scalars come from plan_layout.h in the same shim, as
tdmpc2_plan_create takes them.  Used by tests/test_fused_route.py."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include "fused_route.h"
using namespace tdk;
// tune: cluster_mode, force_rows, fold_refit, cl_fault, cl2_mode; entry: 0 a whole plan, 1 estimate_value (a0: tracing), 2 a sharded
// plan (a0, a1: the row range).  out: the route's fields in order, then Apad, cl_max_clusters, lds_bytes, row_bytes, cl_lds, cl2
extern "C" int route(const tdmpc2_plan_cfg *cfg, int num_cus, int E, const int *tune, int entry, int a0, int a1, long *out) {
    const PlanLayout lo = plan_layout(*cfg, num_cus, CreateEnv{});
    if (lo.err || lo.layered) return 1;
    bool cl2 = false;
    for (int i = 0; i < lo.nbuf; ++i) cl2 |= lo.buf[i].id == PB_CL2_XBUF;
    FusedIn in{};
    in.E = E; in.tiles = lo.tiles; in.N = cfg->num_samples; in.K = cfg->num_elites; in.H = cfg->horizon; in.A = cfg->action_dim;
    in.P = cfg->num_pi_trajs; in.num_cus = num_cus; in.cluster_mode = tune[0]; in.cl_max_clusters = lo.cl_max_clusters;
    in.cl2 = cl2 && tune[4]; in.episodic = cfg->episodic != 0; in.cl_fault = tune[3] != 0; in.force_rows = tune[1]; in.fold_refit = tune[2];
    in.lds_bytes = lo.lds_bytes; in.row_bytes = lo.row_bytes; in.cl_lds = lo.cl_lds;
    const FusedRoute r = entry == 0 ? fused_route_plan(in) : entry == 1 ? fused_route_value(in, a0 != 0) : fused_route_shard(in, a0, a1);
    const long v[] = {r.kind, r.pi_fold, r.pitraj, r.pitraj_nst, (long)r.pitraj_lds, r.nst, r.tiles, r.tile_off, r.grid, (long)r.lds, r.fold,
                      r.refit_stage, (long)r.refit_lds, r.refit_threads, r.arm_cl, r.arm_cl2, r.skip_cvec,
                      lo.Apad, lo.cl_max_clusters, (long)lo.lds_bytes, (long)lo.row_bytes, (long)lo.cl_lds, cl2};
    for (unsigned i = 0; i < sizeof v / sizeof v[0]; ++i) out[i] = v[i];
    return 0;
}
extern "C" long refit_lds(int N, int K, int H, int A, long budget, int *stage) {
    return (long)(budget ? refit_lds_bytes(N, K, H, A, stage, (size_t)budget) : refit_lds_bytes(N, K, H, A, stage));
}
extern "C" int refit_thr(int N) { return refit_threads(N); }
"""
FIELDS = ("kind", "pi_fold", "pitraj", "pitraj_nst", "pitraj_lds", "nst", "tiles", "tile_off", "grid", "lds", "fold", "refit_stage",
          "refit_lds", "refit_threads", "arm_cl", "arm_cl2", "skip_cvec", "Apad", "cl_max_clusters", "lds_bytes", "row_bytes", "cl_lds", "cl2")
TILE, CLUSTER, CLUSTER2 = 0, 1, 2
PLAN, VALUE, SHARD = 0, 1, 2
CUS = 256        # an MI355X
NTHREADS = 512   # workgroup of every ks_* kernel (common.cuh; the launcher shims of k_fused.hip / k_cluster.hip pass it)


def build(tmpdir):
    src = os.path.join(str(tmpdir), "fused_route_shim.cpp")
    with open(src, "w") as f:
        f.write(SHIM)
    so = os.path.join(str(tmpdir), "libfused_route_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tdmpc2_amd", "csrc"), src, "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    ci, pi = ctypes.c_int, ctypes.POINTER(ctypes.c_int)
    lib.route.argtypes = [ctypes.c_void_p, ci, ci, pi, ci, ci, ci, ctypes.POINTER(ctypes.c_long)]
    lib.refit_lds.argtypes = [ci, ci, ci, ci, ctypes.c_long, pi]
    lib.refit_lds.restype = ctypes.c_long
    return lib


def route(lib, plan_cfg, E, cluster=2, rows=0, fold=2, cl_fault=0, cl2_mode=1, cus=CUS, entry=PLAN, a0=0, a1=0):
    """The route of a call of E plans on a handle created from `plan_cfg` (tdmpc2_amd.native.PlanCfg) with the tuning given."""
    out = (ctypes.c_long * len(FIELDS))()
    tune = (ctypes.c_int * 5)(cluster, rows, fold, cl_fault, cl2_mode)
    assert lib.route(ctypes.byref(plan_cfg), cus, E, tune, entry, a0, a1, out) == 0
    return dict(zip(FIELDS, out))


def refit_lds(lib, N, K, H, A, budget=0):
    stage = ctypes.c_int()
    return lib.refit_lds(N, K, H, A, budget, ctypes.byref(stage)), stage.value


def launches(r, E, episodic, iterations):
    """The launches of a whole plan as profiles/fused_route_launches.txt writes them: (prologue, launches of one iteration, I)."""
    ap, ep = r["Apad"], int(bool(episodic))
    head = [f"ks_setup<{ap},0> {E} {NTHREADS}"]
    if r["pitraj"]:
        head.append(f"ks_pitraj<{ap},{r['pitraj_nst']},0> {E} {NTHREADS}")
    kern = {TILE: f"ks_rollout<{ap},{r['nst']},8,0,{ep},0>", CLUSTER: f"ks_rollout_cl<{ap},{ep}>", CLUSTER2: f"ks_rollout_cl2<{ap}>"}[r["kind"]]
    unit = [f"{kern} {r['grid']} {NTHREADS}"]
    if not r["fold"]:
        unit.append(f"k_refit {E} {r['refit_threads']}")
    return head, unit, iterations
