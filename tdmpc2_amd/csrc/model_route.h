// Which launches a tdmpc2_plan_model_rollout / model_losses call is made of (the forward half of TDMPC2._update,
// tdmpc2/tdmpc2.py:259-304), as a pure function of the call's shape and of the outputs asked for.  Compilable on the host,
// no HIP types: tests/test_model_route.py builds it with the host compiler and checks it against tests/model_route_model.py.
//
// A call is up to five STAGES, each one kind of launch:
//   MS_DYN    the open-loop latent rollout zs[t+1] = next(zs[t], a[t]) (tdmpc2.py:268-276).  The only stage whose steps are
//             ordered: one workgroup per 64-row tile walks the steps (fused family), or one dynamics GEMM chain per step over
//             the B rows (layered family).  zs always goes through HBM -- it is an output, and the input of the other stages.
//   MS_HEADS  the chains that read (zs[t], a[t]): the reward head and EVERY Q head (tdmpc2.py:278-280).  They are independent
//             of each other and of the step order, so they run over all H * B rows at once: one workgroup per (row tile,
//             step, chain) in ONE launch (fused), one GEMM chain per head over the H * B flattened rows (layered).
//   MS_TERM   the termination head on all of zs (tdmpc2.py:281-283), (H + 1) * B rows, like a chain of MS_HEADS.
//   MS_CONS   per-row squared distance of zs[1:] to next_z (tdmpc2.py:274), a row kernel.
//   MS_TAIL   one workgroup adds the per-row loss terms in a fixed order (deterministic; no float atomics) and forms the five
//             losses (tdmpc2.py:285-304).
// There is one decomposition per family: the chains of a step are spread over workgroups (fused) or over whole-batch GEMMs
// (layered), and no stage waits for another workgroup -- stages are ordered by the stream.
#pragma once

enum { MODEL_FUSED = 0, MODEL_LAYERED = 1 };
enum { MODEL_MAXH = 8, MODEL_MAXQ = 8, MODEL_TILE = 64 };
// outputs a caller may ask for (bit mask)
enum {
    MW_ZS = 1, MW_REW_LOGITS = 2, MW_REW = 4, MW_Q_LOGITS = 8, MW_Q = 16, MW_TERM = 32,
    MW_LOSSES = 64  // tdmpc2_plan_model_losses: every chain is needed, whatever else is asked for
};
enum { MS_DYN = 0, MS_HEADS = 1, MS_TERM = 2, MS_CONS = 3, MS_TAIL = 4, MS_COUNT = 5 };
// chain ids of MS_HEADS (the kernels' view): 0 = reward, 1 + i = Q head i; MS_TERM runs chain MC_TERM
enum { MC_REWARD = 0, MC_Q0 = 1, MC_TERM = 100 };
// refusals
enum { MR_OK = 0, MR_BAD_H = 1, MR_BAD_B = 2, MR_NOT_EPISODIC = 3, MR_ROWS = 4, MR_NO_BINS = 5, MR_LOSSES_H0 = 6 };

struct ModelIn {
    int family;      // MODEL_FUSED | MODEL_LAYERED
    int B, H;        // batch rows, rollout steps (0 <= H <= MODEL_MAXH)
    int num_q, num_bins, episodic;
    unsigned want;   // MW_* mask
    long row_cap;    // layered family: rows of its activation workspace (max_envs x num_samples, rounded up to the GEMM tile)
    int ln_after;    // layered family: 1 = a NormedLinear is a GEMM AND a LayerNorm row kernel (exact-fp32 arithmetic, or the fused
                     // epilogue off: TDMPC2_TUNE_FUSE_LN = 0 / a downgraded handle); 0 = one launch (the epilogue inside the GEMM)
};

struct ModelStage {
    int run;             // 0: not launched
    int gx, gy, gz;      // fused family: the launch's grid (gx row tiles).  layered family / row kernels: gx workgroups, gy = gz = 1
    long rows;           // rows the stage covers (per launch of the stage when it is chunked)
    int steps;           // MS_DYN: dynamics steps rolled
    int chunks;          // launches (layered MS_TERM: (H + 1) * B rows in pieces of at most row_cap)
    int launches;        // kernel launches of the stage
    unsigned produces;   // MW_* bits this stage writes
};

struct ModelRoute {
    int refuse;                    // MR_*
    ModelStage st[MS_COUNT];
    int nchain;                    // chains of MS_HEADS
    int chain[1 + MODEL_MAXQ];     // their ids, in launch order
    int launches;                  // all stages
};

inline ModelRoute model_route(const ModelIn &in) {
    ModelRoute r{};
    if (in.H < 0 || in.H > MODEL_MAXH) { r.refuse = MR_BAD_H; return r; }
    if (in.B < 1) { r.refuse = MR_BAD_B; return r; }
    const bool losses = (in.want & MW_LOSSES) != 0;
    if (losses && in.H < 1) { r.refuse = MR_LOSSES_H0; return r; }
    if (losses && in.num_bins < 2) { r.refuse = MR_NO_BINS; return r; }
    if ((in.want & MW_TERM) && !in.episodic) { r.refuse = MR_NOT_EPISODIC; return r; }
    const bool rew = in.H > 0 && (losses || (in.want & (MW_REW_LOGITS | MW_REW)));
    const bool qs = in.H > 0 && (losses || (in.want & (MW_Q_LOGITS | MW_Q)));
    const bool term = (in.want & MW_TERM) || (losses && in.episodic);
    const bool all_z = (in.want & MW_ZS) || term || losses;   // zs[H] is needed
    const long hb = (long)in.H * in.B, hb1 = (long)(in.H + 1) * in.B;
    const int tiles = (in.B + MODEL_TILE - 1) / MODEL_TILE;
    const int layered = in.family == MODEL_LAYERED;
    if (layered && (hb > in.row_cap || in.B > in.row_cap)) { r.refuse = MR_ROWS; return r; }
    // launches of one layered chain of three layers, its row kernel not counted: the head / last GEMM and two NormedLinear layers
    // of 1 + ln_after launches each.  (With the epilogue on, lay_route may still fall back to GEMM + row kernel for a shape whose
    // statistics exchange does not fit: `launches` is then a lower bound; grids and stages are exact.)
    const int nl = 1 + (in.ln_after ? 1 : 0);
    const int per_chain = 1 + 2 * nl;
    const int dyn_chain = 3 * nl;   // the dynamics' last layer is a NormedLinear too (SimNorm)

    // ---- MS_DYN
    ModelStage &d = r.st[MS_DYN];
    d.steps = all_z ? in.H : ((rew || qs) ? in.H - 1 : 0);
    if (d.steps > 0) {
        d.run = 1; d.rows = in.B; d.chunks = 1;
        d.gx = tiles; d.gy = d.gz = 1;
        d.launches = layered ? 1 + d.steps * (1 + dyn_chain + 1) : 1;  // layered: init, then per step set-action + 3 layers + extract
        d.produces = in.want & MW_ZS;
    }
    // ---- MS_HEADS
    if (rew) r.chain[r.nchain++] = MC_REWARD;
    if (qs) for (int i = 0; i < in.num_q; ++i) r.chain[r.nchain++] = MC_Q0 + i;
    ModelStage &hd = r.st[MS_HEADS];
    if (r.nchain) {
        hd.run = 1; hd.rows = hb; hd.chunks = 1;
        hd.gx = layered ? (int)((hb + 3) / 4) : tiles; hd.gy = layered ? 1 : in.H; hd.gz = layered ? 1 : r.nchain;
        hd.launches = layered ? 2 + r.nchain * (per_chain + 1) : 1;
        hd.produces = in.want & (MW_REW_LOGITS | MW_REW | MW_Q_LOGITS | MW_Q);
    }
    // ---- MS_TERM
    ModelStage &tm = r.st[MS_TERM];
    if (term) {
        tm.run = 1;
        tm.chunks = layered ? (int)((hb1 + in.row_cap - 1) / in.row_cap) : 1;
        tm.rows = layered ? (tm.chunks == 1 ? hb1 : in.row_cap) : hb1;
        tm.gx = layered ? (int)((tm.rows + 3) / 4) : tiles; tm.gy = layered ? 1 : in.H + 1; tm.gz = 1;
        tm.launches = layered ? tm.chunks * (1 + per_chain + 1) : 1;
        tm.produces = in.want & MW_TERM;
    }
    // ---- MS_CONS, MS_TAIL
    if (losses) {
        ModelStage &c = r.st[MS_CONS];
        c.run = 1; c.rows = hb; c.chunks = 1; c.gx = (int)((hb + 3) / 4); c.gy = c.gz = 1; c.launches = 1;
        ModelStage &t = r.st[MS_TAIL];
        t.run = 1; t.rows = hb; t.chunks = 1; t.gx = t.gy = t.gz = 1; t.launches = 1; t.produces = MW_LOSSES;
    }
    for (int s = 0; s < MS_COUNT; ++s) r.launches += r.st[s].launches;
    return r;
}

// rows of the per-row loss workspace: [3 + num_q][H * B] floats (consistency, reward, termination, Q head 0 ..)
enum { MK_CONS = 0, MK_REW = 1, MK_TERM = 2, MK_Q0 = 3 };
inline long model_rowloss_floats(int B, int H, int num_q) { return (long)(MK_Q0 + num_q) * H * B; }
