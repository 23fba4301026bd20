"""CPU test of the fused family's launch routes (tdmpc2_amd/csrc/fused_route.h, compiled with g++: tests/fused_route_model.py).

1. The launch table: for every call of profiles/fused_route_launches.txt -- c1 / c2_i6 / c2_ep / mt5 plans at the plan counts and
   under the 27 tunings (cluster 0/1/2 x rows 32/64/auto x fold 0/1/2) listed there -- the header's route gives the kernel
   instance, grid and workgroup size of ks_setup, ks_pitraj and every rollout and refit launch that an MI355X recorded
   (rocprofv3 --kernel-trace, dispatch order) running the library of the commit BEFORE the routes moved into the header
   (tools/fused_route_launches.py).
2. The rules that commit's fused_run / shard_values / estimate_value held inline, over E = 1 .. 512 and N in {64, 128, 512, 1024}.
3. refit_lds_bytes under both budgets: integers computed with g++ from that commit's function.
"""
import itertools
import os

import pytest

from tdmpc2_amd import native
from tdmpc2_amd.config import named_config, planner_iterations
from tests import fused_route_model as frm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = os.path.join(ROOT, "profiles", "fused_route_launches.txt")
# oracle/cases.py: CASES (config, overrides) of the recorded calls
CASE_CFG = {"c1": ("c1", {}), "c2_i6": ("c2", dict(iterations=4)), "c2_ep": ("c2", dict(iterations=2, episodic=True)), "mt5": ("mt5", {})}
CALLS = [("c1", 1), ("c1", 3), ("c1", 16), ("c1", 32), ("c1", 33), ("c1", 256), ("c2_i6", 1), ("c2_i6", 256), ("c2_ep", 1), ("mt5", 5)]
TUNING = list(itertools.product((0, 1, 2), (32, 64, 0), (0, 1, 2)))  # cluster, rows, fold
NS = (64, 128, 512, 1024)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return frm.build(tmp_path_factory.mktemp("fused_route"))


def case_cfg(name, E):
    conf, over = CASE_CFG[name]
    cfg = named_config(conf, **over)
    return cfg, planner_iterations(cfg), native.plan_cfg(cfg, planner_iterations(cfg), E, 0, native.PATH_FUSED, native.PREC_AUTO)


def c1(E, **over):
    c = native.plan_cfg(named_config("c1"), 6, E, 0, native.PATH_FUSED, native.PREC_AUTO)
    for k, v in over.items():
        setattr(c, k, v)
    return c


def recorded():
    table = {}
    with open(LAUNCHES) as f:
        for ln in f:
            call, rest = ln.strip().split(" | ")
            name, E, cluster, rows, fold = call.split()
            table[(name, int(E), int(cluster), int(rows), int(fold))] = rest
    return table


# ---------------------------------------------------------------------------------------------------------------- 1. launch table
def test_the_recorded_table_has_every_call():
    assert sorted(recorded()) == sorted((n, E) + t for (n, E) in CALLS for t in TUNING)


@pytest.mark.parametrize("name,E", CALLS, ids=[f"{n}-E{E}" for n, E in CALLS])
def test_the_route_gives_the_launches_the_gpu_recorded(lib, name, E):
    table = recorded()
    cfg, I, pc = case_cfg(name, E)
    for cluster, rows, fold in TUNING:
        r = frm.route(lib, pc, E, cluster=cluster, rows=rows, fold=fold)
        head, unit, n = frm.launches(r, E, cfg.episodic, I)
        assert f"{' ; '.join(head)} ; {n} x [{' ; '.join(unit)}]" == table[(name, E, cluster, rows, fold)], (cluster, rows, fold)


def test_the_two_sides_of_the_rows_switch(lib):
    """c1 (8 tiles of 64 rows per plan, 256 CUs): E = 16 is one round either way -> 32-row workgroups; E = 32 is two rounds of
    32-row workgroups (0.61 x 2) against one of 64-row ones -> 64; E = 33 is 3 x 0.61 against 2 -> 32 again."""
    assert [frm.route(lib, c1(E), E, cluster=0)["nst"] for E in (16, 32, 33, 64, 256)] == [1, 2, 1, 2, 2]


# ---------------------------------------------------------------------------------------------------------------- 2. rules
def py_refit_lds(N, K, H, A, budget=48 * 1024):
    M = 64
    while M < N:
        M *= 2
    base, elite = (2 * M + 3 * K + 4 * H * A + 48) * 4 + 64, K * H * A * 4
    return (base + elite, 1) if base + elite <= budget else (base, 0)


@pytest.mark.parametrize("N", NS)
def test_the_rules_of_a_whole_plan(lib, N):
    # c1 at N samples under every tuning; then what else the routes look at, under the tunings that reach a cluster route
    variants = [(dict(), 0, 1, 256, TUNING)] + [v + ([(1, 0, 2), (2, 0, 2), (2, 32, 1)],) for v in (
        (dict(episodic=1), 0, 1, 256), (dict(), 1, 1, 256), (dict(), 0, 0, 256), (dict(num_pi_trajs=0), 0, 1, 256),
        (dict(num_pi_trajs=40), 0, 1, 256), (dict(), 0, 1, 80), (dict(action_dim=64, num_elites=N), 0, 1, 256))]
    for over, cl_fault, cl2_mode, cus, tunings in variants:
        pc = c1(1, num_samples=N, **over)
        for E in range(1, 513):
            pc.max_envs = E
            for cluster, rows, fold in tunings:
                r = frm.route(lib, pc, E, cluster=cluster, rows=rows, fold=fold, cl_fault=cl_fault, cl2_mode=cl2_mode, cus=cus)
                tiles, P, key = N // 64, pc.num_pi_trajs, (N, E, over, cluster, rows, fold, cus)
                if r["kind"] != frm.TILE:  # a cluster route never exceeds the handle's clusters or the chip
                    assert cluster != 0 and 0 < E * tiles * 2 <= r["cl_max_clusters"], key
                    # (the two-cluster grid is padded to groups of 8 tiles x 2 roles: its 2 x 8 workgroups per tile are what must fit)
                    assert r["grid"] <= cus if r["kind"] == frm.CLUSTER else 2 * 8 * tiles * 2 <= cus, key
                    assert r["grid"] == (E * tiles * 2 + 7) // 8 * 64 * (2 if r["kind"] == frm.CLUSTER2 else 1), key
                    assert r["nst"] == 1 and r["lds"] == r["cl_lds"] and r["skip_cvec"] and r["arm_cl"], key
                else:
                    assert r["grid"] == E * r["tiles"] and r["tiles"] * r["nst"] == 2 * tiles and not r["skip_cvec"], key
                    assert r["lds"] == r["lds_bytes"] - (32 * r["row_bytes"] if r["nst"] == 1 else 0), key
                    if rows:  # every forced value is honoured
                        assert r["nst"] == rows // 32, key
                assert r["pi_fold"] == (r["kind"] != frm.TILE and 0 < P <= 32), key
                assert r["pitraj"] == (P > 0 and not r["pi_fold"]) and r["pitraj_nst"] == (1 if P <= 32 else 2), key
                if r["kind"] == frm.CLUSTER2:
                    assert E == 1 and cluster == 2 and not pc.episodic and not cl_fault and cl2_mode and r["cl2"] and r["arm_cl2"], key
                # the refit is folded only when the elite stage fits the 32-row tile, and then sized for it
                lds32, stage32 = py_refit_lds(N, pc.num_elites, pc.horizon, pc.action_dim, 32 * r["row_bytes"])
                one_round = r["kind"] != frm.TILE or r["grid"] <= cus
                assert r["fold"] == bool(stage32 and (fold == 1 or (fold == 2 and one_round))), key
                assert (r["refit_lds"], r["refit_stage"]) == ((lds32, stage32) if r["fold"] else py_refit_lds(N, pc.num_elites, pc.horizon, pc.action_dim)), key
                assert r["refit_threads"] == max(64, N), key


@pytest.mark.parametrize("N", NS)
def test_a_trace_call_always_gets_64_row_workgroups(lib, N):
    for E in range(1, 513):
        pc = c1(E, num_samples=N)
        for rows in (0, 32, 64):
            t = frm.route(lib, pc, E, rows=rows, entry=frm.VALUE, a0=1)
            assert (t["kind"], t["nst"], t["tiles"], t["grid"], t["lds"]) == (frm.TILE, 2, N // 64, E * N // 64, t["lds_bytes"]), (N, E, rows)
            v = frm.route(lib, pc, E, rows=rows, entry=frm.VALUE, a0=0)  # without a trace: the plan's per-tile geometry
            p = frm.route(lib, pc, E, rows=rows, cluster=0)
            assert (v["kind"], v["nst"], v["tiles"], v["grid"], v["lds"]) == (frm.TILE, p["nst"], p["tiles"], p["grid"], p["lds"]), (N, E, rows)
            assert not v["pitraj"] and not v["fold"] and not v["skip_cvec"] and v["arm_cl"] == p["arm_cl"]


@pytest.mark.parametrize("N", NS)
def test_shard_ranges_map_to_whole_tiles_with_the_right_offset(lib, N):
    for E in (1, 2, 3, 16, 255, 512):
        pc = c1(E, num_samples=N)
        for rows in (0, 32, 64):
            trows = 32 if rows == 32 else 64
            for b in range(0, N, 64):
                for e in range(b + 64, N + 1, 64):
                    r = frm.route(lib, pc, E, rows=rows, entry=frm.SHARD, a0=b, a1=e)
                    assert r["kind"] == frm.TILE and r["nst"] * 32 == trows and not r["fold"] and not r["pi_fold"], (N, E, rows, b, e)
                    assert (r["tile_off"] * trows, r["tiles"] * trows, r["grid"]) == (b, e - b, E * r["tiles"]), (N, E, rows, b, e)
                    assert r["pitraj"] and r["pitraj_nst"] == 1


# ---------------------------------------------------------------------------------------------------------------- 3. refit LDS
# (N, K, H, A, row_bytes): ((bytes, stage) under the default 48 KiB budget, (bytes, stage) under the 32-row tile's budget)
REFIT_LDS = {
    (512, 64, 3, 6, 2128): ((10016, 1), (10016, 1)),     # c1, mt5
    (512, 64, 3, 38, 2256): ((36128, 1), (36128, 1)),    # c2
    (64, 64, 3, 6, 2128): ((6432, 1), (6432, 1)),
    (1024, 64, 3, 6, 2128): ((14112, 1), (14112, 1)),
    (512, 64, 3, 64, 2320): ((8192, 0), (57344, 1)),     # the elites fit the tile's budget only
    (512, 512, 3, 38, 2256): ((12320, 0), (12320, 0)),   # ... and neither
}


def test_refit_lds_bytes_gives_the_values_it_gave_before_the_move(lib):
    for (N, K, H, A, rb), (dflt, tile) in REFIT_LDS.items():
        assert frm.refit_lds(lib, N, K, H, A) == dflt and frm.refit_lds(lib, N, K, H, A, 32 * rb) == tile, (N, K, H, A)
        assert py_refit_lds(N, K, H, A) == dflt and py_refit_lds(N, K, H, A, 32 * rb) == tile
    for name, A in (("c1", 6), ("c2_i6", 38), ("mt5", 6)):
        r = frm.route(lib, case_cfg(name, 1)[2], 1)
        assert (512, 64, 3, A, r["row_bytes"]) in REFIT_LDS
