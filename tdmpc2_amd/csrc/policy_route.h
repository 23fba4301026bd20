// The policy prior's launch routes (WorldModel.pi, tdmpc2/common/world_model.py:144-184: _pi = NormedLinear(Mish) ->
// NormedLinear(Mish) -> Linear(2A), then the Gaussian head of common/math.py:12-29): which route a call takes, the rows per
// GEMV workgroup, the grid, threads and LDS of every launch, the work item of every thread, and the workspace binding
// allocates.  Pure functions; policy_kernels.cuh and plan_obs.hip call them, tests/test_policy_route.py compiles this
// header with g++ and checks them on the CPU (tests/policy_route_model.py).
#pragma once
#include <cstddef>

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

constexpr int POL_THREADS = 512;         // row-route and LayerNorm workgroups (= the encoder's ENC_THREADS: k_enc_norm is reused)
constexpr int POL_MAX_PER_THREAD = 8;    // output features per thread: widths up to 4096
constexpr int POL_MAX_WIDTH = POL_THREADS * POL_MAX_PER_THREAD;
constexpr int POL_GEMV_COLS = 64;        // output features per GEMV workgroup (lane = feature: 256 contiguous bytes per k)
constexpr int POL_GEMV_WAVES = 8;        // waves of a GEMV workgroup; they split the contraction
constexpr int POL_GEMV_THREADS = 64 * POL_GEMV_WAVES;
constexpr int POL_MAX_R = 8;             // rows per GEMV workgroup (each weight byte is read once per R rows)
constexpr int POL_HEAD_THREADS = 64;     // one wave per row: A <= 64 lanes
constexpr int POL_MAX_A = 64;
constexpr size_t POL_LDS_MAX = 160 * 1024;
constexpr int POL_SPREAD_LAUNCHES = 6;   // GEMV, norm, GEMV, norm, GEMV, head

// Auto threshold (profiles/policy_latency.json): the row route streams the whole chain through one CU per row, the
// spread route pays six launches (seven when acting) and spreads each layer over mlp_dim / 64 workgroups.  Measured on one MI355X
// (act_pi, observation -> action): 5M 65 vs 61 us at E = 1 and 68 vs 81 us at E = 8 .. 73 vs 84 us at E = 256; 19M 223 vs 287 us at
// E = 1 and 244 vs 344 us at E = 256; 48M 463 vs 212 us at E = 1.  So: the row route up to mlp_dim 1024 (the 1M, 5M and 19M models)
// for up to 256 rows -- the measured range --, the spread route for the 48M and 317M models and beyond 256 rows.
constexpr int POL_ROW_MAX_MLP = 1024;
constexpr int POL_ROW_MAX_ROWS = 256;

enum PolRouteKind { POL_ROW = 0, POL_SPREAD = 1 };
enum PolMode { POL_AUTO = 0, POL_FORCE_ROW = 1, POL_FORCE_SPREAD = 2 };  // TDMPC2_TUNE_POLICY_ROUTE

struct PolGrid {
    int x, y, threads;
    size_t lds;
    int R;        // GEMV: rows per workgroup (0 for the other launches)
    int in, out;  // GEMV: contraction and output width; norm / head: out = row width
};
struct PolRoute {
    int kind;
    int launches;
    PolGrid g[POL_SPREAD_LAUNCHES];  // ROW: g[0] only
};

// ---------------------------------------------------------------------------------------------------------------------------
// LDS
__host__ __device__ inline size_t pol_row_lds(int maxw) { return ((size_t)2 * maxw + POL_THREADS / 64) * 4; }  // x | y | reduction
__host__ __device__ inline size_t pol_gemv_lds(int R, int in) {
    return ((size_t)R * in + (size_t)POL_GEMV_WAVES * R * POL_GEMV_COLS) * 4;  // R input rows | per-wave partials
}
inline bool pol_row_fits(int maxw) { return maxw >= 1 && maxw <= POL_MAX_WIDTH && pol_row_lds(maxw) <= POL_LDS_MAX; }

// rows per GEMV workgroup: a power of two up to POL_MAX_R, no more than the rows there are, halved until its LDS fits
inline int pol_rows_per_wg(int n, int in) {
    int R = 1;
    while (R < POL_MAX_R && R < n) R *= 2;
    while (R > 1 && pol_gemv_lds(R, in) > POL_LDS_MAX) R /= 2;
    return R;
}

// workspace of the spread route: x [max_envs][mlp] (Mish activations) and y [max_envs][max(mlp, 2A)] (pre-activations)
inline size_t pol_ws_x_floats(int max_envs, int mlp) { return (size_t)max_envs * mlp; }
inline size_t pol_ws_y_floats(int max_envs, int mlp, int A) { return (size_t)max_envs * (mlp > 2 * A ? mlp : 2 * A); }

// ---------------------------------------------------------------------------------------------------------------------------
// Route of one call of n rows (a spread-route chunk: n <= max_envs).  in0 = latent_dim + task_dim, maxw = the widest layer the
// row-route launch runs (the policy's, and when acting with a narrow encoder, the encoder's too).
inline int pol_auto_kind(int mlp, int n) { return mlp <= POL_ROW_MAX_MLP && n <= POL_ROW_MAX_ROWS ? POL_ROW : POL_SPREAD; }

inline PolRoute pol_route(int n, int in0, int mlp, int A, int maxw, int mode) {
    PolRoute r{};
    int kind = mode == POL_FORCE_ROW ? POL_ROW : mode == POL_FORCE_SPREAD ? POL_SPREAD : pol_auto_kind(mlp, n);
    if (kind == POL_ROW && !pol_row_fits(maxw)) kind = POL_SPREAD;
    r.kind = kind;
    if (kind == POL_ROW) {
        r.launches = 1;
        r.g[0] = PolGrid{n, 1, POL_THREADS, pol_row_lds(maxw), 0, 0, 0};
        return r;
    }
    r.launches = POL_SPREAD_LAUNCHES;
    const int ins[3] = {in0, mlp, mlp}, outs[3] = {mlp, mlp, 2 * A};
    for (int l = 0; l < 3; ++l) {
        const int R = pol_rows_per_wg(n, ins[l]);
        r.g[2 * l] = PolGrid{(outs[l] + POL_GEMV_COLS - 1) / POL_GEMV_COLS, (n + R - 1) / R, POL_GEMV_THREADS,
                             pol_gemv_lds(R, ins[l]), R, ins[l], outs[l]};
        if (l < 2) r.g[2 * l + 1] = PolGrid{n, 1, POL_THREADS, 0, 0, 0, mlp};
    }
    r.g[5] = PolGrid{n, 1, POL_HEAD_THREADS, 0, 0, 0, A};
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Work items.  GEMV: thread t of workgroup (bx, by) computes output feature f of rows by * R .. by * R + R - 1 (the reduction
// over the waves is done by threads t < R * 64: row by * R + t / 64, feature bx * 64 + t % 64).
struct PolItem {
    int row, f;
    bool valid;
};
__host__ __device__ inline PolItem pol_gemv_item(int bx, int by, int R, int t, int n, int out) {
    const int row = by * R + t / POL_GEMV_COLS, f = bx * POL_GEMV_COLS + t % POL_GEMV_COLS;
    return PolItem{row, f, t < R * POL_GEMV_COLS && row < n && f < out};
}
// row route and norm: thread t's u-th feature of row bx
__host__ __device__ inline PolItem pol_row_item(int bx, int t, int u, int width) {
    const int f = t + u * POL_THREADS;
    return PolItem{bx, f, f < width};
}
// head: lane t = action dimension of row bx
__host__ __device__ inline PolItem pol_head_item(int bx, int t, int A) { return PolItem{bx, t, t < A}; }
