// The route of every split-arithmetic GEMM launch of the layered family: which kernel and template instance, the grid, the tile
// order, the K-parts, and whether the NormedLinear epilogue runs inside the GEMM -- the launches whose workgroups wait for each
// other.  Pure functions of the layer's shape and of what the handle offers; layered_host.cuh fills the
// kernels' parameters around what they return and launches.  Plain C++ (no HIP types), like tile_order.h: tests/test_layer_route.py
// compiles it with g++, checks the launches it returns in the dispatcher model of tests/test_tile_order.py and pins the routes
// of the benched geometries.  Also here: the ids, defaults and accepted ranges of the measurement knobs (tdmpc2_plan_set_tuning).
#pragma once
#include <algorithm>
#include <cstddef>

#include "tile_order.h"

// ---------------------------------------------------------------------------------------------------------------------------
// Tile constants the routes and the kernels share
constexpr int GBM = 128;          // rows per GEMM workgroup (the narrow tiles; the wide tile takes 256)
constexpr int GM_TM = 128;        // g_gemm_m (layered_mid.cuh): rows of a tile
constexpr int MR_R = 8;           // m_rows<512>: rows per workgroup
// m_rows' LN kinds on FEW rows (fewer than MR_WIDE_MIN: one plan of the 48M model, the policy-prior pass) take one workgroup of
// 256 threads per row (m_rows<256>, layered_mid.cuh: m_rows_ln1)
#ifndef MR_WIDE_MIN_ROWS
#define MR_WIDE_MIN_ROWS 1024
#endif
constexpr int MR_WIDE_MIN = MR_WIDE_MIN_ROWS;

// ---------------------------------------------------------------------------------------------------------------------------
// Measurement knobs of the tile choice.  They used to be environment variables read inside the shipped library (VERDICT r5 weak
// #10: 28 names, an A/B surface that could silently change a deployment); now they are fields of the handle, reachable ONLY through
// tdmpc2_plan_set_tuning(h, TDMPC2_TUNE_EXPERT + id, value) -- the Python binding maps TDMPC2_X_<NAME> of its own environment onto
// that call for the A/B tools (tdmpc2_amd/native.py), the library itself reads none of them.
// Order = enum tdmpc2_expert_knob of include/tdmpc2_plan.h.
enum LayKnob { LK_W256_MIN, LK_W_SPLIT_MIN, LK_W_SPLIT_MAX, LK_W_SPLIT_OVH, LK_KSPLIT_AUTO_LO, LK_KSPLIT_AUTO_MIN, LK_W_XCD_ROWS, LK_NCT1,
               LK_WIDE_MIN, LK_RT4, LK_FILL_PERMILLE, LK_FILL_HEAD_PERMILLE, LK_SD1, LK_XCD_ROWS, LK_COL_PAD, LK_TWOHOT_UNFUSED,
               LK_Z0_SHARED_OFF, LK_MID_PARTS_MAX, LK_MID_FUSE_LN, LK_MID_SPLIT_XCD, LK_MID_PIFOLD, LK_COUNT };
// default and the values that have a meaning (anything else: TDMPC2_ERR_INVALID).  -1 = automatic where the code has a rule;
// a negative LK_W256_MIN switches the wide tile off.
struct LayKnobSpec {
    int def, lo, hi;
};
constexpr LayKnobSpec LAY_KNOBS[LK_COUNT] = {
    {192, -(1 << 30), 1 << 30},  // LK_W256_MIN: tiles from which a fused NormedLinear layer takes g_gemm_w (< 0: never)
    {192, 0, 1 << 30},           // LK_W_SPLIT_MIN: K-split mode 1: fewest workgroups of a split launch
    {4, 1, 4},                   // LK_W_SPLIT_MAX: most K-parts of a tail tile (1: no split)
    {12000, 0, 1 << 30},         // LK_W_SPLIT_OVH: a split tile's overhead, / (k16-slabs + 25), in 1/1000 tile times
    {16, 0, 1 << 30},            // LK_KSPLIT_AUTO_LO: K-split mode 2: fewest tiles of a split launch
    {-1, -1, 1 << 30},           // LK_KSPLIT_AUTO_MIN: K-split mode 2: fewest workgroups of a split launch (-1: cus / 4)
    {-1, -1, 4},                 // LK_W_XCD_ROWS: g_gemm_w's order (gemm_s_order: -1 auto, 0 row-major, 1 XCD-local, 2 / 4 rectangles;
                                 // the 9 of profiles/README.md r5g named an engine-local order that is no longer built: 9 would be 1)
    {0, 0, 1},                   // LK_NCT1: never the 128 x 256 tile
    {128, 0, 1 << 30},           // LK_WIDE_MIN: workgroups from which a wide output takes the 128 x 256 tile
    {0, 0, 1},                   // LK_RT4: always 128-row narrow tiles
    {750, 0, 1 << 20},           // LK_FILL_PERMILLE: workgroups per 2 x #CUs a narrow tile must fill before its rows are halved
    {750, 0, 1 << 20},           // LK_FILL_HEAD_PERMILLE: the same for outputs of one column block (heads)
    {0, 0, 1},                   // LK_SD1: never the four-chunk-deep narrow tiles
    {-1, -1, 4},                 // LK_XCD_ROWS: the fused narrow tiles' order (gemm_s_order)
    {1, -1, 1},                  // LK_COL_PAD: padding of the row-major order (gemm_s_order: 0 never)
    {0, 0, 1},                   // LK_TWOHOT_UNFUSED: the two-hot never in the GEMM's epilogue
    {0, 0, 1},                   // LK_Z0_SHARED_OFF: no shared z0 products at t = 0 (lay_cvec)
    {16, 1, 1 << 20},            // LK_MID_PARTS_MAX: most K-parts of a few-row problem
    {1, 0, 1},                   // LK_MID_FUSE_LN: whole-K few-row tiles run the NormedLinear epilogue in g_gemm_m
    {1, 0, 1},                   // LK_MID_SPLIT_XCD: two few-row problems of one shape on one half of the XCDs each
    {1, 0, 1},                   // LK_MID_PIFOLD: a single few-row plan computes the policy-prior rows inside iteration 0's stage
};
struct LayKnobs {  // the handle's values (Layered::knob)
    int v[LK_COUNT];
    constexpr LayKnobs() : v{} {
        for (int i = 0; i < LK_COUNT; ++i) v[i] = LAY_KNOBS[i].def;
    }
    int operator[](int i) const { return v[i]; }
    int &operator[](int i) { return v[i]; }
};

// ---------------------------------------------------------------------------------------------------------------------------
// What the handle offers a launch (Layered and the buffer set of the chain the launch is on)
struct LayCtx {
    long cus;                          // compute units of the device
    int ksplit;                        // TDMPC2_TUNE_KSPLIT: 0 never, 1 whenever the rule says so, 2 few-tile launches only
    bool fuse_ln;                      // the handle's consent to inter-workgroup waits (off after a reported wait: apply_modes)
    bool row_env;                      // a per-row env map (multitask value calls)
    bool arrive;                       // arrival counters exist
    size_t arrive_off, arrive_cap;     // the next free counter of the stage, counters of the handle
    bool stats;                        // the chain's statistics exchange buffer exists
    size_t stats_cap;                  // floats of it
    bool ksws;                         // the chain's K-split workspace exists
    size_t ksws_slots;                 // its 256 KiB slots
    const int *knob;                   // [LK_COUNT]
};

// What follows the nn.Linear (= the EPI of the GEMM instance that runs it inside its epilogue)
enum { LR_PLAIN = 0, LR_MISH = 1, LR_SIMNORM = 2, LR_TWOHOT = 3 };

// ---------------------------------------------------------------------------------------------------------------------------
// One per-layer launch (lay_gemm, split arithmetic)
struct LayIn {
    size_t rows_p;      // padded rows
    int rows_per_env;
    int CT;             // output column tiles of 32
    int nk;             // k16-blocks contracted (the t = 0 first layers: the action columns only)
    int want;           // LR_MISH / LR_SIMNORM: a NormedLinear; LR_TWOHOT: a two-hot head (the row routine may join the epilogue)
};
struct LayRoute {
    bool w;             // g_gemm_w<epi, wo.parts > 1> (512 threads), else g_gemm_s<nct, rt, sd, epi, 0> (GTHREADS)
    int nct, rt, sd;    // g_gemm_s: column tiles per wave (2: the 128 x 256 tile), rows / 32, row-operand staging depth
    int epi;            // 0 plain; 1 / 2 NormedLinear (Mish / SimNorm) inside the GEMM: its workgroups wait; 3 the two-hot in the epilogue
    int nrowblk, ncolblk;
    GemmSOrder ord;     // epi 1 / 2: the tile order
    GemmWOrder wo;      // g_gemm_w: the K-split tail (parts 1: none)
    unsigned grid;
    size_t arrive;      // arrival counters the launch takes from the stage's
    bool ln_after;      // a NormedLinear not fused: pre-activations -> PRE, lay_ln behind the GEMM
};

inline LayRoute lay_route(const LayIn &in, const LayCtx &c) {
    const int *knob = c.knob;
    const long cus = c.cus;
    const bool ln = in.want == LR_MISH || in.want == LR_SIMNORM;
    LayRoute r{};
    // Can the NormedLinear epilogue run inside the GEMM?  (always decided the same way whatever the tile: the statistics'
    // combination order is tile-independent, so a plan's bits do not depend on the size of the call it is part of)
    const bool can_fuse = ln && c.fuse_ln && c.arrive && c.stats && in.rows_p * ((in.CT + 3) / 4) * 2 <= c.stats_cap;
    // ---- the 256 x 256 tile (g_gemm_w): fused NormedLinear layers of calls that fill the chip with one workgroup per CU
    const long w256_min = knob[LK_W256_MIN];
    // (Measured and rejected, profiles/README.md r4f: 256 x 224 / 192 tiles -- 8 x 1 wave layout, one W fragment set -- for widths
    // like the 48M model's 1792 = 8 x 224, which would fill 1.875 rounds of the chip instead of 1.64: the layout reads every W
    // fragment eight times from LDS (128 KiB per slab) and lost 4.5 % in spite of the better fill.)
    constexpr int NT = 8;
    const int ncb256 = (in.CT + NT - 1) / NT;
    const size_t stats_need = in.rows_p * ((in.CT + 3) / 4) * 2;
    // K-split tail (tile_order.h: gemm_w_order): tiles of the launch's last, partly filled round are computed by `parts`
    // workgroups each.  That makes the wide tile worth taking from fewer tiles on (a 180-tile SimNorm layer: 720 workgroups)
    const int nrowblk_w = (int)(in.rows_p / 256);
    const long cus_x = cus >= 8 ? cus / 8 : 1;
    const long ks_min = knob[LK_W_SPLIT_MIN];
    const int ks_maxp = knob[LK_W_SPLIT_MAX];
    const int ks_ovh = knob[LK_W_SPLIT_OVH];
    GemmWOrder wo{};
    wo.parts = 1;
    const bool w_shape = can_fuse && in.CT >= 8 && in.rows_p % 256 == 0 && in.rows_per_env % 256 == 0 && ncb256 <= 32 && !c.row_env &&
                         stats_need <= c.stats_cap && w256_min >= 0;
    // ksplit 0 never; 1 whenever the round arithmetic says so; 2 (default) only for launches that leave most of the chip idle -- 16 ..
    // 128 tiles, i.e. one or two plans of the 317M model (64 tiles -> 256 workgroups of a quarter of K: single-plan latency 17.85 ->
    // 16.2 ms, +9.7 % plans/s at E = 1; the 48M model at E = 4: +6 %; profiles/r5j_*).  On launches that fill the chip the partial sums'
    // traffic (256 KiB per part through the fabric, +210 MB per hidden GEMM of the 48M model at E = 30) costs more than the better fill
    // buys: c3 -10 ... -13 %, c4 -2.7 % (profiles/README.md r5d).
    const long tiles_w = (long)nrowblk_w * ncb256;
    const long ks_auto_lo = knob[LK_KSPLIT_AUTO_LO];
    const long ks_auto_min = knob[LK_KSPLIT_AUTO_MIN] >= 0 ? knob[LK_KSPLIT_AUTO_MIN] : cus / 4;
    const bool ks_want = c.ksplit == 1 || (c.ksplit == 2 && tiles_w >= ks_auto_lo && tiles_w <= cus / 2);
    if (w_shape && ks_want && c.ksws && ks_maxp > 1) {
        const int nk = in.nk;
        wo = gemm_w_order(nrowblk_w, ncb256, (int)cus_x, nk, ks_maxp, ks_ovh / (nk + 25));
        if (wo.parts > 1 && ((size_t)8 * wo.max_tail * wo.parts > c.ksws_slots || (long)wo.nblk < (c.ksplit == 2 ? ks_auto_min : ks_min))) wo.parts = 1;
    }
    const size_t n_arrive = (size_t)nrowblk_w + (wo.parts > 1 ? (size_t)8 * wo.max_tail : 0);
    if (w_shape && ((long)nrowblk_w * ncb256 >= w256_min || wo.parts > 1) &&
        c.arrive_off + n_arrive <= c.arrive_cap /* out of arrival counters: the narrow tiles below degrade to the unfused LayerNorm */) {
        r.w = true;
        r.epi = in.want;
        r.nrowblk = nrowblk_w;
        r.ncolblk = ncb256;
        r.wo = wo;
        r.arrive = n_arrive;
        // tile order: XCD-local row blocks keep the column blocks of a row block -- which wait for each other -- on consecutive
        // slots of ONE XCD (with one workgroup per CU and <= 16 column blocks two launches in flight cannot starve each other:
        // 2 x 15 waiting workgroups < 32 CUs), and read every A row through one L2
        const int xr_env = knob[LK_W_XCD_ROWS];
        // TDMPC2_GEMM_W_XCD_ROWS=2: XCD rectangles, a row block on 2 XCDs -- per XCD and launch A/4 + W/2 instead of A/8 + W
        // through the L2.  At 16 column blocks (317M model): c4 +1 %, fabric-side reads of the launch 881 -> 654 MB, of a stage
        // 27.3 -> 20.6 GB (profiles/README.md r4s, r4t) -- but NOT the default: with a row block on two XCDs two launches in
        // flight can wait for each other in a circle (A's XCD full of launch 1 waiting for B's, B's full of launch 2 waiting
        // for A's); the stress test lost 3 waits in 6 300 stages that way, the XCD-local order none (r4za).
        const int xr_auto = r.nrowblk >= 16 ? 1 : 0;
        r.ord = gemm_s_order(r.nrowblk, r.ncolblk, xr_env >= 0 ? xr_env : xr_auto, 1);
        r.grid = (unsigned)(wo.parts > 1 ? wo.nblk : r.ord.nblk);
        return r;
    }
    // wide outputs (>= 256 columns) take the 128 x 256 tile from 128 such workgroups on: with a second chain in flight
    // (lay_estimate_value) a partly filled round is not idle (A/B r3n: threshold 512 -> 256: c3 +2.0 %, c4 +2.3 %; 128: single
    // plans of the 317M model 20.8 -> 18.7 ms; below that single plans of the 48M model lose)
    const size_t wide_min = knob[LK_NCT1] ? (size_t)1 << 30 : (size_t)knob[LK_WIDE_MIN];
    const bool wide = in.CT >= 8 && (in.rows_p / GBM) * ((in.CT + 7) / 8) >= wide_min;
    r.ncolblk = wide ? (in.CT + 7) / 8 : (in.CT + 3) / 4;
    // rows per workgroup tile: 128 when that fills the chip (two workgroups per CU), else 64 or 32 -- few rows mean
    // single-plan latency, where occupancy beats operand reuse (TDMPC2_GEMM_RT=4 forces the 128-row tile)
    const long slots = 2L * cus;
    int rt = 4;
    if (!wide && !knob[LK_RT4]) {
        const double fill = knob[LK_FILL_PERMILLE] / 1000.0;
        const double fill_head = knob[LK_FILL_HEAD_PERMILLE] / 1000.0;
        const double f = in.CT <= 4 ? fill_head : fill;  // narrow outputs (two-hot / policy heads): one column block
        while (rt > 1 && (double)((long)(in.rows_p / (32 * rt)) * r.ncolblk) < (double)slots * f) rt >>= 1;
    }
    r.nrowblk = (int)(in.rows_p / (32 * rt));
    const int nblk = r.nrowblk * r.ncolblk;
    // few workgroups per CU: row operand staged four chunks deep, weight ring of 8 / 16 blocks (g_gemm_s<.., .., 4>)
    const bool deep = !wide && (long)nblk < 2 * slots && !knob[LK_SD1];
    // The throughput tile stages its row operand TWO chunks ahead (g_gemm_s<2, 4, 2, ..>: same sums; c3 +0.4 ... 0.7 %,
    // c4 +0.5 % over one chunk ahead in three same-call A/Bs, profiles/README.md r3z / r3y / r3x).
    r.nct = wide ? 2 : 1;
    r.rt = rt;
    r.sd = wide ? 2 : deep ? 4 : 1;
    r.grid = (unsigned)nblk;
    const bool fuse = can_fuse && c.arrive_off + (size_t)r.nrowblk <= c.arrive_cap;
    if (fuse) {
        r.epi = in.want;
        r.arrive = (size_t)r.nrowblk;
        // tile order (tile_order.h); TDMPC2_GEMM_XCD_ROWS = 0 / 1: never / always XCD-local row blocks, TDMPC2_GEMM_COL_PAD = 0:
        // no padding of the row-major order
        r.ord = gemm_s_order(r.nrowblk, r.ncolblk, knob[LK_XCD_ROWS], knob[LK_COL_PAD]);
        r.grid = (unsigned)r.ord.nblk;
    } else if (ln) {
        r.ln_after = true;
    } else if (in.want == LR_TWOHOT && !wide && rt <= 2 && in.CT <= 4 && (long)nblk >= cus && !knob[LK_TWOHOT_UNFUSED]) {
        // two-hot head: the row routine in the epilogue -- from one workgroup per CU on (c3 E = 30: +1.4 %; a single plan's 16-32
        // workgroups are better served by l_twohot's one wavefront per row across the chip: 3.33 vs 3.44 ms, profiles r4i)
        r.epi = LR_TWOHOT;
    }
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The few-row path (layered_mid.cuh): every nn.Linear = one g_gemm_m problem (K-parts of 128 x 256 tiles, raw fp32 partial sums) +
// one m_rows problem; a launch of either kernel carries one or two problems.
struct MidCtx {
    bool split, mid;                   // split arithmetic; TDMPC2_TUNE_FEWROW
    int ksplit;                        // TDMPC2_TUNE_KSPLIT (0: the few-row path is off too)
    bool mws, side_bufs, row_env;      // partial-sum workspaces, the second buffer set, a per-row env map
    long cus;
    int maxct;                         // column tiles of 32 of the widest layer: max(mlp_dim, latent_dim) / 32, rounded up
};

// The few-row path takes the call (both lay_estimate_value's and lay_pitraj's, and lay_run's decision to fold the policy-prior rows)
inline bool mid_ok(const MidCtx &m, size_t rows_p) {
    if (!m.split || !m.mid || m.ksplit == 0 || !m.mws || !m.side_bufs || m.row_env) return false;
    return 2 * (long)(rows_p / GM_TM) * ((m.maxct + 7) / 8) <= m.cus;  // a launch's two widest problems fill at most one round of the chip
}

struct MidProbIn {
    int CT;             // output column tiles of 32
    int nk16;           // k16-blocks contracted
    bool ln;            // MR_LN_MISH / MR_LN_SIMNORM (else a head: two-hot, policy, termination)
    bool actions;       // the rows also write the next step's action columns (m_rows only)
    bool stats;         // the statistics exchange buffer of this problem's slot
};
struct MidIn {
    size_t rows, rows_p;
    int rows_per_env;
    int n;                     // problems (1 or 2)
    MidProbIn pr[2];
    bool rows_one_by_one;      // the second problem's rows read what the first one's wrote (the two Q heads' two-hots)
    bool arrive_pending;       // the stage's counters have not been zeroed yet
    size_t mws_cap;            // floats per partial-sum workspace
};
struct MidRoute {
    bool ws_ok;                // the partial sums fit the workspaces
    struct Prob {
        int nk, ncolblk, nrowblk, parts, nblk;  // g_gemm_m: k32-slabs, column blocks of 256, row blocks of GM_TM, K-parts, workgroups
        int ldw;
        long part_stride;
        bool epi;              // the NormedLinear epilogue inside g_gemm_m (whole-K tile: its workgroups wait); else m_rows
        bool reset;            // zero the stage's counters in front of this problem (the first that waits)
        size_t arrive;         // counters it takes
        int nwg;               // m_rows workgroups
    } pr[2];
    int split_xcd;             // g_gemm_m: one problem per half of the XCDs
    unsigned gblk;             // g_gemm_m workgroups (512 threads)
    int nrow;                  // m_rows problems (0: no launch)
    int mr_threads;            // m_rows<256> / m_rows<512>
    int serial;                // m_rows: one grid over problem 0's rows, both problems in order
    unsigned rblk;
};

inline MidRoute mid_route(const MidIn &in, const LayCtx &c) {
    MidRoute m{};
    m.ws_ok = true;
    const long cus = c.cus;
    long tiles = 0;
    for (int i = 0; i < in.n; ++i) tiles += (long)(in.rows_p / GM_TM) * ((in.pr[i].CT + 7) / 8);
    const int pmax = c.knob[LK_MID_PARTS_MAX];
    const int pall = (int)std::max<long>(1, std::min<long>(pmax, cus / std::max<long>(tiles, 1)));
    bool pending = in.arrive_pending;
    size_t off = c.arrive_off;
    for (int i = 0; i < in.n; ++i) {
        const MidProbIn &o = in.pr[i];
        MidRoute::Prob &g = m.pr[i];
        g.nk = o.nk16 / 2;  // k32-slabs
        g.ncolblk = (o.CT + 7) / 8; g.nrowblk = (int)(in.rows_p / GM_TM);
        g.parts = std::max(1, std::min(pall, g.nk / 2));
        g.ldw = g.ncolblk * 256; g.part_stride = (long)in.rows_p * g.ldw;
        if ((size_t)g.parts * g.part_stride > in.mws_cap) m.ws_ok = false;
        g.nblk = 8 * ((g.ncolblk * g.parts + 7) / 8) * g.nrowblk;
        m.gblk += (unsigned)g.nblk;
        if ((int)in.rows < MR_WIDE_MIN) g.nwg = o.ln ? (int)in.rows : (int)((in.rows + 3) / 4);  // m_rows<256>
        else g.nwg = (int)((in.rows + MR_R - 1) / MR_R);                                        // m_rows<512>
        // whole-K tiles of a NormedLinear: LayerNorm + activation + split in the GEMM's own epilogue (no partial sums, no m_rows) -- the
        // 317M model's hidden layers (2 x 128 tiles = the chip), the 48M model from four plans on.  Needs the exchange buffers and the
        // handle's consent (fuse_ln: off after a reported wait, apply_modes).  Rows that also carry the next step's actions stay with m_rows.
        const size_t stats_need = in.rows_p * ((o.CT + 3) / 4) * 2;
        if (o.ln && g.parts == 1 && c.fuse_ln && c.knob[LK_MID_FUSE_LN] && !o.actions && o.stats && c.arrive && stats_need <= c.stats_cap &&
            (pending ? 0 : off) + (size_t)g.nrowblk <= c.arrive_cap && in.rows_per_env % GM_TM == 0) {
            if (pending) {
                pending = false;
                g.reset = true;
                off = 0;
            }
            g.epi = true;
            g.arrive = (size_t)g.nrowblk;
            off += g.arrive;
        } else {
            m.nrow++;
            m.rblk += (unsigned)g.nwg;
        }
    }
    // two problems of one shape: one per half of the XCDs (g_gemm_m); each problem's share of the grid is 4 x ceil(jobs / 4) x row blocks
    if (in.n == 2 && c.knob[LK_MID_SPLIT_XCD] && m.pr[0].ncolblk * m.pr[0].parts == m.pr[1].ncolblk * m.pr[1].parts &&
        m.pr[0].nrowblk == m.pr[1].nrowblk) {
        const int jobs = m.pr[0].ncolblk * m.pr[0].parts;
        m.split_xcd = 1;
        m.gblk = 8u * (unsigned)((jobs + 3) / 4) * (unsigned)m.pr[0].nrowblk;
        m.pr[0].nblk = m.pr[1].nblk = (int)m.gblk / 2;
    }
    m.mr_threads = (int)in.rows < MR_WIDE_MIN ? 256 : 512;
    if (in.rows_one_by_one && m.nrow == 2) {  // the second problem's rows read what the first one's wrote (the two Q heads' two-hots, qtmp):
        m.serial = 1;                         // one grid over problem 0's rows, every wavefront does its row of both problems in order
        m.rblk = (unsigned)m.pr[0].nwg;
    }
    return m;
}
