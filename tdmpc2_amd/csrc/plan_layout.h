// What tdmpc2_plan_create decides for a configuration before it touches the device: whether the configuration is accepted, which
// kernel family and arithmetic it gets, every derived scalar the handle stores, and the device buffers the handle owns from the
// start -- which exist, how large each is, which start zeroed.  Pure functions of (configuration, compute units, creation-time
// switches); plan_core.hip allocates what they return.  Plain C++ (no HIP types, no allocation, no environment), like
// layer_route.h: tests/test_plan_layout.py compiles it with g++, and tests/layer_route_model.py takes the capacities the routes
// are tested with from here.  (The lazily grown sets -- weights, encoders, task tables, model / policy-loss rows -- are not here.)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>

#include "../../include/tdmpc2_plan.h"
#include "layer_route.h"  // GBM

namespace tdk {

// ---------------------------------------------------------------------------------------------------------------------------
// Constants the layout shares with the kernels (common.cuh includes this header)
constexpr int ROWS = 64;        // sample rows per rollout workgroup
constexpr int WIDTH = 512;      // latent_dim == mlp_dim of the fused size class
constexpr int MAXQ = 8;
constexpr int MAXH = 8;
constexpr int GBK = 32;           // layered family: k-chunk staged through LDS
enum { BE_DYN = 0, BE_REW = 1, BE_PI = 2, BE_Q0 = 3 };  // slots of the effective first-layer biases; BE_Q0 + head
// cluster path (cluster_kernels.cuh)
constexpr int CL = 8;                  // workgroups per cluster
constexpr int CL_SLOTS = 6;            // exchange tiles per cluster (S4 holds a head's logits, [32][128] fp32; S5: episodic models)
constexpr int CL_TILE = 32 * WIDTH;    // floats per exchange tile
constexpr int CL_FLAG_STRIDE = 16;     // arrival words reserved per cluster (64 B)
constexpr int CL2_SLOTS = 6 + 2 * MAXH;  // ks_rollout_cl2 (cluster2_kernels.cuh), exchange tiles per cluster: 0 / 1 layers, 4 head, 5 policy head, 6 + t: Z[t], 6 + MAXH + t: prior policy head of step t
// sizes that only the host decides
constexpr size_t LDS_MAX = 160 * 1024;        // LDS of a gfx950 workgroup
constexpr size_t LDS_LN = 4096;               // fused family: LayerNorm partials, and as much again for the LayerNorm affine (CtxT::gb)
constexpr size_t CL_LDS_RING = (size_t)2 * 8 * 4 * 64 * 16;  // cluster path: its weight-fragment ring, 64 KiB
constexpr size_t ARRIVE_PER_32_ROWS = 64;     // fused NormedLinear epilogue: arrival counters a stage may take per 32 rows and chain
constexpr size_t KS_SLOT_FLOATS = 65536;      // g_gemm_w's K-split: one 256 x 256 fp32 partial accumulator = 256 KiB per (split tile, part)
constexpr size_t KS_XCDS = 8, KS_PARTS = 4;   // its tail tiles are counted per XCD; most K-parts of one
constexpr size_t KS_TAIL_MAX = 32;            // mode 1 splits the last round of any launch = at most 32 tail tiles per XCD
constexpr size_t MWS_TILE_FLOATS = 128 * 256; // few-row path: one partial-sum tile of 64 x 256 (128 x 256) floats, one per CU at most
constexpr int DEFAULT_CUS = 256;

inline size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }
// column tiles of 32 of a model's widest row (hidden or latent): what the statistics exchange, the wide tile and the few-row path go by
inline int plan_maxct(const tdmpc2_plan_cfg &c) { return (std::max(c.mlp_dim, c.latent_dim) + 31) / 32; }
// compute units the sizes and routes are worked out for: the device's, or an MI355X's where the runtime does not say
inline long plan_cus(int num_cus) { return num_cus > 0 ? num_cus : DEFAULT_CUS; }

// ---------------------------------------------------------------------------------------------------------------------------
// The creation-time switches (plan_core.hip fills them from the environment once, at the top of create)
struct CreateEnv {
    bool one_stream = false;  // TDMPC2_ONE_STREAM (set): layered family without its second chain
    bool fuse_ln = true;      // TDMPC2_FUSE_LN: NormedLinear epilogue inside the GEMM (layered, split arithmetic)
    int ksplit = 2;           // TDMPC2_KSPLIT, clamped to [0, 2] (Layered::ksplit)
    bool fewrow = true;       // TDMPC2_FEWROW (Layered::mid)
    int cluster = 2;          // TDMPC2_CLUSTER (tdmpc2_plan::cluster_mode)
    bool gw_timing = false;   // TDMPC2_GW_TIMING (set), -DGW_TIMING builds only
    bool timing = false;      // TDMPC2_TIMING (set), -DSPLIT_TIMING builds only
};

// ---------------------------------------------------------------------------------------------------------------------------
// The buffers a handle owns from creation on.  (The K-split workspaces are sized by ksws_slots below: set_tuning may grow them.)
enum PlanBufId {
    PB_BINS, PB_ACTIONS, PB_VALUE, PB_MEAN, PB_STD, PB_TICKET, PB_QIDX_BUF, PB_ONE, PB_BEFF,
    PB_CVEC, PB_ZSCRATCH,                                                                      // fused family
    PB_CL_XBUF, PB_CL_ZS, PB_CL_FLAGS, PB_CL2_XBUF, PB_CL2_ZS, PB_CL2_FLAGS, PB_CL2_MAIL,       // its cluster path
    PB_X, PB_HA, PB_HB, PB_LG, PB_G, PB_QT, PB_TERM, PB_QIDX, PB_Z0X, PB_LCVEC,                 // layered family
    PB_HA2, PB_HB2, PB_LG2,                                                                    // its second chain
    PB_STATS, PB_STATS2, PB_ARRIVE, PB_MWS0, PB_MWS1, PB_PRE, PB_PRE2,                          // split arithmetic
    PB_COUNT
};
struct PlanBuf {
    PlanBufId id;
    const char *name;
    size_t bytes;
    bool zero;  // starts zeroed
};
struct PlanLayout {
    int err = TDMPC2_OK;  // a refusal: code and message, nothing else is filled
    char msg[512] = "";
    int path = 0, precision = 0;  // resolved (never AUTO)
    bool layered = false, split = false;
    bool second_chain = false;    // layered family: buffers, stream and events of the second chain of GEMMs
    bool err_line = false;        // the host-mapped error line of the bounded waits (cluster path, fused NormedLinear epilogue)
    int Apad = 0, tiles = 0, nnets = 0, stride = 0;
    size_t row_bytes = 0, lds_bytes = 0, cl_lds = 0;
    int cl_max_clusters = 0;
    int Kin = 0, Mp = 0, ldl = 0, Ppad = 0, ldpre = 0;  // Layered
    size_t cvec_rows = 0, stats_cap = 0, arrive_cap = 0, ks_tiles = 0, mws_cap = 0;
    int nbuf = 0;
    PlanBuf buf[PB_COUNT];
    void add(PlanBufId id, const char *name, size_t bytes, bool zero = false) { buf[nbuf++] = PlanBuf{id, name, bytes, zero}; }
};

// g_gemm_w's K-split workspaces (256 KiB per split tile and part, one workspace per chain), sized for what the handle's mode can
// use (every layered handle used to pay for 1 024 slots per chain -- 0.5 GiB -- whatever its mode): mode 0 none; mode 2
// (the default) only splits launches of at most cus / 2 tiles = at most cus / 16 tail tiles per XCD; mode 1 the last round of any
// launch = 32 tail tiles per XCD; never more than all the tiles of the handle's largest call.  Slots per workspace.
inline size_t ksws_slots(size_t ks_tiles, int num_cus, int mode) {
    if (!ks_tiles || mode == 0) return 0;
    const size_t cus = (size_t)plan_cus(num_cus);
    const size_t cap_slots = KS_XCDS * (mode == 2 ? round_up(cus / 16, 4) : KS_TAIL_MAX) * KS_PARTS;
    return std::min(cap_slots, ks_tiles * KS_PARTS);
}

#define PLAN_REFUSE(code, ...)                           \
    do {                                                 \
        lo.err = (code);                                 \
        snprintf(lo.msg, sizeof lo.msg, __VA_ARGS__);    \
        return lo;                                       \
    } while (0)

inline PlanLayout plan_layout(const tdmpc2_plan_cfg &c, int num_cus, const CreateEnv &env) {
    PlanLayout lo;
    // ---- limits common to both kernel families
    if (c.action_dim < 1 || c.action_dim > 64) PLAN_REFUSE(TDMPC2_ERR_UNSUPPORTED, "action_dim %d outside [1, 64]", c.action_dim);
    // num_bins 0 / 1: the reference's regression heads -- one output column, two_hot_inv = identity / symexp (math.py:76-79)
    if (c.num_bins < 0 || c.num_bins > 128) PLAN_REFUSE(TDMPC2_ERR_UNSUPPORTED, "num_bins %d outside [0, 128]", c.num_bins);
    if (c.num_q < 2 || c.num_q > MAXQ) PLAN_REFUSE(TDMPC2_ERR_UNSUPPORTED, "num_q %d outside [2, %d]", c.num_q, MAXQ);
    if (c.horizon < 1 || c.horizon > MAXH) PLAN_REFUSE(TDMPC2_ERR_UNSUPPORTED, "horizon %d outside [1, %d]", c.horizon, MAXH);
    if (c.num_samples % ROWS != 0 || c.num_samples < ROWS || c.num_samples > 1024)
        PLAN_REFUSE(TDMPC2_ERR_UNSUPPORTED, "num_samples %d must be a multiple of %d in [%d, 1024]", c.num_samples, ROWS, ROWS);
    if (c.num_pi_trajs < 0 || c.num_pi_trajs > ROWS || c.num_pi_trajs >= c.num_samples)
        PLAN_REFUSE(TDMPC2_ERR_UNSUPPORTED, "num_pi_trajs %d outside [0, %d]", c.num_pi_trajs, ROWS);
    if (c.num_elites < 1 || c.num_elites > c.num_samples) PLAN_REFUSE(TDMPC2_ERR_INVALID, "num_elites %d", c.num_elites);
    if (c.num_valid_samples != 0 && (c.num_valid_samples < c.num_elites || c.num_valid_samples > c.num_samples ||
                                     c.num_valid_samples <= c.num_pi_trajs || c.num_samples - c.num_valid_samples >= GBM))
        PLAN_REFUSE(TDMPC2_ERR_INVALID, "num_valid_samples %d: 0, or the true sample count behind num_samples %d rounded up to the row tile "
                    "(>= num_elites %d, > num_pi_trajs %d)", c.num_valid_samples, c.num_samples, c.num_elites, c.num_pi_trajs);
    if (c.simnorm_dim != 8) PLAN_REFUSE(TDMPC2_ERR_UNSUPPORTED, "simnorm_dim %d (kernels are built for 8)", c.simnorm_dim);
    if (c.multitask && c.task_dim < 1) PLAN_REFUSE(TDMPC2_ERR_INVALID, "multitask needs task_dim > 0");
    if (c.multitask && c.episodic)  // the reference asserts the same: tdmpc2/common/world_model.py:136
        PLAN_REFUSE(TDMPC2_ERR_UNSUPPORTED, "termination head with task ids is not supported (reference world_model.py:136)");
    if (c.iterations < 1 || c.max_envs < 1) PLAN_REFUSE(TDMPC2_ERR_INVALID, "iterations / max_envs must be positive");
    if (c.latent_dim < 8 || c.mlp_dim < 8 || c.latent_dim % 8 != 0)
        PLAN_REFUSE(TDMPC2_ERR_UNSUPPORTED, "latent_dim %d / mlp_dim %d", c.latent_dim, c.mlp_dim);
    // ---- kernel family
    const bool fits_fused = c.latent_dim == WIDTH && c.mlp_dim == WIDTH;
    const bool fits_layered = c.latent_dim % 32 == 0 && c.mlp_dim % 32 == 0 && c.num_samples % GBM == 0;
    int path = c.path;
    if (path == TDMPC2_PATH_AUTO) path = fits_fused ? TDMPC2_PATH_FUSED : TDMPC2_PATH_LAYERED;
    if (path == TDMPC2_PATH_FUSED && !fits_fused)
        PLAN_REFUSE(TDMPC2_ERR_UNSUPPORTED, "fused planner kernels are built for latent_dim == mlp_dim == %d (got %d / %d)",
                    WIDTH, c.latent_dim, c.mlp_dim);
    if (path == TDMPC2_PATH_LAYERED && !fits_layered)
        PLAN_REFUSE(TDMPC2_ERR_UNSUPPORTED, "layered planner kernels need latent_dim %% 32 == 0, mlp_dim %% 32 == 0 and "
                    "num_samples %% %d == 0 (got %d / %d / %d)", GBM, c.latent_dim, c.mlp_dim, c.num_samples);
    if (path != TDMPC2_PATH_FUSED && path != TDMPC2_PATH_LAYERED) PLAN_REFUSE(TDMPC2_ERR_INVALID, "unknown path %d", c.path);
    int prec = c.precision;
    if (prec == TDMPC2_PREC_AUTO) prec = TDMPC2_PREC_SPLIT_F16;
    if (prec != TDMPC2_PREC_FP32 && prec != TDMPC2_PREC_SPLIT_F16) PLAN_REFUSE(TDMPC2_ERR_INVALID, "unknown precision %d", c.precision);
    if (prec == TDMPC2_PREC_SPLIT_F16 && path == TDMPC2_PATH_LAYERED && (c.mlp_dim > 4096 || c.latent_dim > 4096))
        PLAN_REFUSE(TDMPC2_ERR_UNSUPPORTED, "the layered f16x2-split row kernels hold a row of at most 4096 columns in registers");

    lo.path = path;
    lo.precision = prec;
    lo.layered = path == TDMPC2_PATH_LAYERED;
    lo.split = prec == TDMPC2_PREC_SPLIT_F16;
    lo.Apad = (c.action_dim + 15) / 16 * 16;  // the fused kernels are instantiated for action paddings 16 / 32 / 48 / 64
    lo.tiles = c.num_samples / ROWS;
    lo.nnets = BE_Q0 + c.num_q;
    const size_t cus = (size_t)plan_cus(num_cus);
    const size_t E = c.max_envs, H = c.horizon, N = c.num_samples, A = c.action_dim;
    if (!lo.layered) {
        if (lo.split) {
            // operand form: row = [hi: SH halfs | lo: SH halfs | 8 pad]; row stride in dwords SH + 4 = 4 x odd
            const int SH = WIDTH + lo.Apad;
            lo.stride = 2 * SH + 8;  // in halfs
            lo.row_bytes = (size_t)lo.stride * 2;
        } else {
            // fp32 rows [z (512) | a (Apad) | 4 pad]: stride / 4 odd -> conflict-free ds_read_b128 across 16 rows
            lo.stride = WIDTH + lo.Apad + 4;  // in floats
            lo.row_bytes = (size_t)lo.stride * 4;
        }
        // after the tile: LayerNorm partials, LayerNorm affine (CtxT::gb), then mean / std [2 H A] of the rollout kernel or
        // the 64 row -> task entries of ks_value
        const size_t tail = std::max<size_t>(2 * H * A * 4, 256);
        lo.lds_bytes = (size_t)ROWS * lo.row_bytes + LDS_LN /* LayerNorm partials */ + LDS_LN /* LayerNorm affine */ + tail + 64;
        if (lo.lds_bytes > LDS_MAX) PLAN_REFUSE(TDMPC2_ERR_UNSUPPORTED, "LDS tile of %zu bytes exceeds 160 KiB", lo.lds_bytes);
    }
    lo.add(PB_BINS, "bins", (size_t)(c.num_bins > 1 ? c.num_bins : 2) * 4);
    lo.add(PB_ACTIONS, "actions", E * H * N * A * 4);
    lo.add(PB_VALUE, "value", E * N * 4);
    lo.add(PB_MEAN, "mean", E * H * A * 4);
    lo.add(PB_STD, "std", E * H * A * 4);
    lo.add(PB_TICKET, "ticket", E * 4, true);
    lo.add(PB_QIDX_BUF, "qidx_buf", E * 2 * 4);
    if (!lo.split) lo.add(PB_ONE, "one", 4);  // unit scale of the exact arithmetic (LayerS::oscale / ascale)
    if (!lo.layered) {
        lo.add(PB_CVEC, "cvec", E * 2 * WIDTH * 4);
        lo.add(PB_BEFF, "beff", E * lo.nnets * WIDTH * 4);
        lo.add(PB_ZSCRATCH, "zscratch", E * lo.tiles * ROWS * WIDTH * 4);
        // cluster path (single-plan latency): split arithmetic, sized for the calls that fit the chip in one round
        if (lo.split) {
            const size_t per_env = (size_t)lo.tiles * 2;  // 32-row tiles = clusters per plan
            const size_t envs = std::min(E, cus / (per_env * CL));
            lo.cl_lds = (size_t)32 * lo.row_bytes + 2 * LDS_LN + round_up(2 * H * A * 4, 16) + CL_LDS_RING + 64;
            if (envs >= 1 && lo.cl_lds <= LDS_MAX) {
                const size_t ncl = envs * per_env;
                lo.add(PB_CL_XBUF, "cl_xbuf", ncl * CL_SLOTS * CL_TILE * 4);
                lo.add(PB_CL_ZS, "cl_zs", ncl * CL * 32 * WIDTH * 4);
                lo.add(PB_CL_FLAGS, "cl_flags", ncl * CL_FLAG_STRIDE * 4, true);
                lo.cl_max_clusters = (int)ncl;
                lo.err_line = true;
                // two clusters per tile for ONE plan (ks_rollout_cl2): needs every CU of the chip
                if (!c.episodic && 2 * per_env * CL <= cus) {
                    const size_t n2 = 2 * per_env;
                    lo.add(PB_CL2_XBUF, "cl2_xbuf", n2 * CL2_SLOTS * CL_TILE * 4);
                    lo.add(PB_CL2_ZS, "cl2_zs", n2 * CL * 32 * WIDTH * 4);
                    lo.add(PB_CL2_FLAGS, "cl2_flags", n2 * CL_FLAG_STRIDE * 4, true);
                    lo.add(PB_CL2_MAIL, "cl2_mail", per_env * 32 * 2 * 4);
                }
            }
        }
        return lo;
    }
    lo.Kin = (int)round_up((size_t)c.latent_dim + A, GBK);
    lo.Mp = c.mlp_dim;
    lo.ldl = (int)round_up((size_t)(c.num_bins > 2 * c.action_dim ? c.num_bins : 2 * c.action_dim), 32);
    lo.Ppad = (int)round_up((size_t)(c.num_pi_trajs > 0 ? c.num_pi_trajs : 1), 32);
    const size_t Rp = round_up(E * N, GBM);  // the policy-prior pass (E * Ppad rows) reuses the same buffers
    const size_t Kin = lo.Kin, Mp = lo.Mp, ldl = lo.ldl;
    // stale rows of padded tiles are computed but never read back; start them finite
    lo.add(PB_X, "X", Rp * Kin * 4, true);
    lo.add(PB_HA, "HA", Rp * Mp * 4, true);
    lo.add(PB_HB, "HB", Rp * Mp * 4, true);
    lo.add(PB_LG, "LG", Rp * ldl * 4);
    lo.add(PB_G, "G", Rp * 4);
    lo.add(PB_QT, "QT", Rp * 4);
    lo.add(PB_TERM, "TERM", Rp * 4);
    lo.add(PB_QIDX, "qidx", E * 2 * 4);
    // beff is read per ROW of a GEMM tile; tiles of the policy-prior pass may run past the last plan: + 4 plans
    lo.add(PB_BEFF, "beff", (round_up(E, GBM) + 4) * lo.nnets * Mp * 4, true);
    // second chain (reward || dynamics, Q head || Q head): buffers, stream, events
    lo.second_chain = !env.one_stream;
    if (lo.second_chain) {
        lo.add(PB_HA2, "HA2", Rp * Mp * 4, true);
        lo.add(PB_HB2, "HB2", Rp * Mp * 4, true);
        lo.add(PB_LG2, "LG2", Rp * ldl * 4);
    }
    if (!lo.split) return lo;
    // lay_cvec: z0 rows in operand form (one per plan, padded to a GEMM tile), cvec [2][rows][Mp]
    lo.cvec_rows = round_up(E, GBM);
    lo.add(PB_Z0X, "Z0X", lo.cvec_rows * Kin * 4, true);
    lo.add(PB_LCVEC, "lay.cvec", 2 * lo.cvec_rows * Mp * 4);
    // fused NormedLinear epilogue: exchange buffer, counters, error word
    const size_t maxct = (size_t)plan_maxct(c);
    lo.stats_cap = Rp * ((maxct + 3) / 4) * 2;
    lo.arrive_cap = ARRIVE_PER_32_ROWS * (Rp / 32) * 2;  // two chains
    lo.add(PB_STATS, "stats", lo.stats_cap * 4);
    lo.add(PB_STATS2, "stats2", lo.stats_cap * 4);
    lo.add(PB_ARRIVE, "arrive", lo.arrive_cap * 4, true);
    lo.err_line = true;
    // g_gemm_w's K-split tail: 256 x 256 tiles of the handle's largest call (0: the wide tile never applies); ksws_slots
    lo.ks_tiles = (Rp % 256 == 0 && maxct >= 8) ? (Rp / 256) * ((maxct + 7) / 8) : 0;
    // the few-row path (layered_mid.cuh): partial sums of a launch's two problems -- parts x tiles <= #CUs tiles of 64 x 256
    // (128 x 256) floats each.  Only where a single plan fits the chip in one round of such tiles, and the second buffer set exists.
    if (lo.second_chain && (N + 127) / 128 * ((maxct + 7) / 8) <= cus) {
        lo.mws_cap = cus * MWS_TILE_FLOATS;
        lo.add(PB_MWS0, "mws[0]", lo.mws_cap * 4);
        lo.add(PB_MWS1, "mws[1]", lo.mws_cap * 4);
    }
    // fp32 pre-activations of the NormedLinear layers whose epilogue is not fused (the fallback after a reported wait,
    // TDMPC2_TUNE_FUSE_LN = 0, tiles the fused path does not take): one buffer per chain
    lo.ldpre = std::max(lo.Mp, (int)round_up((size_t)c.latent_dim, 32));
    lo.add(PB_PRE, "PRE", Rp * lo.ldpre * 4);
    if (lo.second_chain) lo.add(PB_PRE2, "PRE2", Rp * lo.ldpre * 4);
    return lo;
}
#undef PLAN_REFUSE

}  // namespace tdk
