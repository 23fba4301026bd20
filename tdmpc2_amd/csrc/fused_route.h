// The fused 512-wide family's launch routes (TDMPC2._plan after encode(), tdmpc2/tdmpc2.py:154-206, and _estimate_value,
// tdmpc2.py:122-136): which rollout kernel a call takes (one workgroup per row tile, a cluster of 8 per 32-row tile, two clusters
// per tile), 32- or 64-row workgroups, whether ks_pitraj runs or the first rollout launch folds it in, grid and dynamic LDS of every
// launch, whether the refit rides in the rollout launch, and what ks_setup arms.  Pure functions of the handle's scalars;
// plan_run.hip launches what they say, tests/test_fused_route.py compiles this header with g++ and checks them on the CPU
// (tests/fused_route_model.py) against the launches a GPU recorded (profiles/fused_route_launches.txt).
#pragma once
#include <cstddef>

#include "plan_layout.h"  // plan_cus

#ifndef TDMPC2_DEFAULT_THROUGHPUT_ST
#define TDMPC2_DEFAULT_THROUGHPUT_ST 2  // sample tiles per workgroup when a call has enough plans to fill the chip
#endif

namespace tdk {

// ---------------------------------------------------------------------------------------------------------------------------
// Elite selection + refit (k_refit, and the last-arriver epilogue of the rollout kernels: refit_plan of common.cuh)
// dynamic LDS of the refit; `stage` out: whether the K x H x A elite actions fit next to the rest (they are then gathered
// by the whole workgroup in one round of loads instead of 2 K dependent global loads per (t, a) thread: 35 -> 12 us)
inline size_t refit_lds_bytes(int N, int K, int H, int A, int *stage, size_t budget = 48 * 1024) {
    size_t M = 64;
    while (M < (size_t)N) M <<= 1;  // sort keys: 8 bytes per padded sample
    const size_t base = (2 * M + 3 * (size_t)K + 4 * H * A + 48) * 4 + 64;
    const size_t elite = (size_t)K * H * A * 4;
    *stage = base + elite <= budget;
    return *stage ? base + elite : base;
}
// threads of a k_refit workgroup: the sort width (one key per thread)
inline int refit_threads(int N) {
    int M = 64;
    while (M < N) M <<= 1;
    return M;
}

// ---------------------------------------------------------------------------------------------------------------------------
struct FusedIn {
    int E, tiles;  // plans of the call, 64-row tiles per plan
    int N, K, H, A, P;
    int num_cus;   // as the runtime reports them (plan_cus fills in an MI355X's where it does not)
    int cluster_mode, cl_max_clusters;
    bool cl2;      // the buffers of the two-cluster route exist and TDMPC2_CLUSTER2 left it on
    bool episodic, cl_fault;
    int force_rows, fold_refit;  // TDMPC2_TUNE_ROWS_PER_WORKGROUP (0 auto | 32 | 64), TDMPC2_TUNE_FOLD_REFIT (0 | 1 | 2 auto)
    size_t lds_bytes, row_bytes, cl_lds;
};
enum FusedKind { FR_TILE = 0, FR_CLUSTER = 1, FR_CLUSTER2 = 2 };
struct FusedRoute {
    int kind;        // ks_rollout | ks_rollout_cl | ks_rollout_cl2
    bool pi_fold;    // the first rollout launch computes the policy-prior trajectories (cluster 0 of each plan)
    bool pitraj;     // ks_pitraj is launched: grid E, 32 * pitraj_nst rows
    int pitraj_nst;
    size_t pitraj_lds;
    int nst;         // 32-row sample tiles per rollout workgroup
    int tiles, tile_off;  // row tiles of 32 * nst rows per plan in this launch, and the first of them
    int grid;        // workgroups
    size_t lds;
    bool fold;       // the refit runs inside the rollout launch (else k_refit: grid E, refit_threads)
    int refit_stage;
    size_t refit_lds;
    int refit_threads;
    bool arm_cl, arm_cl2;  // ks_setup zeroes the arrival words of the cluster / two-cluster route
    bool skip_cvec;        // ks_setup skips the z0 products (the cluster routes do not read cvec)
};

// dynamic LDS of a per-tile workgroup of nst 32-row tiles (ks_rollout, ks_pitraj)
inline size_t fused_tile_lds(const FusedIn &in, int nst) { return nst == 2 ? in.lds_bytes : in.lds_bytes - (size_t)32 * in.row_bytes; }

// 32- or 64-row workgroups.  A 64-row workgroup reuses every weight fragment for two row tiles and is the efficient one when
// the chip is full; a call with few plans is better served by twice as many 32-row workgroups.  Model: one workgroup per CU at
// a time, a round of 32-row workgroups takes 0.61 of a round of 64-row ones (measured, c1: 0.34 vs 0.556 ms per launch); pick
// the geometry with the shorter sum of rounds (E = 16: +30 % plans/s; profiles/README.md has the forced 32 / forced 64 / automatic
// table).  Always 8 wavefronts per workgroup: a 4-wave, 32-row geometry (two workgroups per CU, so that one's VALU epilogue
// overlaps the other's MFMA k-loop; the device code is templated for it: CtxT<APAD, 1, 4>) was measured and lost, 5.83 vs 4.88 ms
// per launch: each weight fragment then feeds one row tile, the k-loop needs 85 B/clk/CU of fragment loads and becomes L1-bound.
inline int fused_sample_tiles(const FusedIn &in, bool tracing) {
    if (tracing) return 2;  // the activation trace is laid out per 64-row tile
    if (in.force_rows) return in.force_rows / 32;
    const long cus = plan_cus(in.num_cus);
    const long w2 = (long)in.E * in.tiles, w1 = 2 * w2;
    const long r2 = (w2 + cus - 1) / cus, r1 = (w1 + cus - 1) / cus;
    return 0.61 * (double)r1 < (double)r2 ? 1 : TDMPC2_DEFAULT_THROUGHPUT_ST;
}

// what every entry point shares: ks_setup's flags and a per-tile rollout launch of `tiles` row tiles per plan from `tile_off`
inline FusedRoute fused_route_tiles(const FusedIn &in, int nst, int tiles, int tile_off) {
    FusedRoute r{};
    r.kind = FR_TILE;
    // the arrival words of this call's clusters start every plan at zero (phase numbers grow through its launches)
    r.arm_cl = in.cl_max_clusters && (long)in.E * in.tiles * 2 <= in.cl_max_clusters;
    r.arm_cl2 = r.arm_cl && in.E == 1 && in.cl2 && in.cluster_mode == 2;
    r.nst = nst; r.tiles = tiles; r.tile_off = tile_off;
    r.grid = in.E * tiles;
    r.lds = fused_tile_lds(in, nst);
    return r;
}

// one policy-prior pass of its own: one 32-row tile holds the trajectories when P <= 32 (the reference uses 24)
inline void fused_route_pitraj(const FusedIn &in, FusedRoute &r) {
    r.pitraj = in.P > 0 && !r.pi_fold;
    r.pitraj_nst = in.P <= 32 ? 1 : 2;
    r.pitraj_lds = fused_tile_lds(in, r.pitraj_nst);
}

// ---------------------------------------------------------------------------------------------------------------------------
// A whole plan (tdmpc2_plan_run): ks_setup, ks_pitraj unless folded, then per CEM iteration one rollout launch and, unless folded,
// k_refit.
inline FusedRoute fused_route_plan(const FusedIn &in) {
    const long cus = plan_cus(in.num_cus);
    // single-plan latency: 8 workgroups per 32-row tile when the whole call then still fits the chip in one round
    const long clusters = (long)in.E * in.tiles * 2;
    const bool cluster = in.cluster_mode != 0 && in.cl_max_clusters > 0 && clusters <= in.cl_max_clusters &&
                         (clusters + 7) / 8 * 64 <= cus;
    const int nst = cluster ? 1 : fused_sample_tiles(in, false);
    FusedRoute r = fused_route_tiles(in, nst, in.tiles * (2 / nst), 0);
    if (cluster) {
        // a single non-episodic plan: the reward chain runs beside the dynamics chain on a second cluster per tile (all 256 CUs)
        const bool two = in.cluster_mode == 2 && in.E == 1 && in.cl2 && !in.episodic && !in.cl_fault;
        r.kind = two ? FR_CLUSTER2 : FR_CLUSTER;
        // clusters of 8 workgroups in groups of 8 (one per XCD).  ks_rollout_cl2 maps blocks to (tile, role) in groups of 8 tiles x
        // 2 roles: BOTH roles of every started group of 8 tiles need their blocks ((2 * clusters + 7) / 8 groups left tiles 0 .. 3
        // of a 64- / 128-sample plan without their R cluster: D's mailbox wait gave up and the plan returned NaN)
        r.grid = (int)((clusters + 7) / 8 * 64) * (two ? 2 : 1);
        r.lds = in.cl_lds;
        r.skip_cvec = true;
        // ... which also computes the policy-prior trajectories (cluster 0 of each plan, first launch) and needs no z0 products
        r.pi_fold = in.P > 0 && in.P <= 32;
    }
    fused_route_pitraj(in, r);
    // elite selection + refit: inside the rollout launch (last workgroup of each plan, LDS budget = the 32-row tile) or as a launch
    // of its own.  The in-launch refit stages the re-derived elite actions in the (then idle) tile memory; if they do not fit it
    // is never folded.  (A requested per-iteration action dump does not change this: the dump reads h->actions after the launch.)
    // TDMPC2_TUNE_FOLD_REFIT: 0 never, 1 always, 2 (auto) only when the whole launch is one round of workgroups (few plans:
    // latency).  With several rounds every round ends with the refits of the plans that completed in it, on CUs whose next
    // workgroup then starts late: measured +0.5 ms on the 4.4 ms launch of 256 plans, against 30 us for the separate k_refit launch.
    r.refit_lds = refit_lds_bytes(in.N, in.K, in.H, in.A, &r.refit_stage, (size_t)32 * in.row_bytes);
    const bool one_round = cluster || (long)in.E * r.tiles <= cus;
    r.fold = r.refit_stage && (in.fold_refit == 1 || (in.fold_refit == 2 && one_round));
    if (!r.fold) r.refit_lds = refit_lds_bytes(in.N, in.K, in.H, in.A, &r.refit_stage);
    r.refit_threads = refit_threads(in.N);
    return r;
}

// tdmpc2_plan_estimate_value(_trace): ks_setup and one per-tile rollout launch on given actions; a trace forces 64-row workgroups
inline FusedRoute fused_route_value(const FusedIn &in, bool tracing) {
    const int nst = fused_sample_tiles(in, tracing);
    return fused_route_tiles(in, nst, in.tiles * (2 / nst), 0);
}

// A sharded plan (tdmpc2_plan_shard_begin / shard_values): ks_setup and ks_pitraj once, then per call the per-tile rollout launch of
// sample rows [row_begin, row_end) of every plan (aligned to 64).  32-row workgroups only when forced.  The refit is always k_refit.
inline FusedRoute fused_route_shard(const FusedIn &in, int row_begin, int row_end) {
    const int nst = in.force_rows == 32 ? 1 : 2, trows = 32 * nst;
    FusedRoute r = fused_route_tiles(in, nst, (row_end - row_begin) / trows, row_begin / trows);
    fused_route_pitraj(in, r);
    r.refit_lds = refit_lds_bytes(in.N, in.K, in.H, in.A, &r.refit_stage);
    r.refit_threads = refit_threads(in.N);
    return r;
}

}  // namespace tdk
