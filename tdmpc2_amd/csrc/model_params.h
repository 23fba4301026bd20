// Kernel parameter blocks of the model rollout / loss entry points (tdmpc2_plan_model_rollout / model_losses; kernels:
// model_kernels.cuh, model_layered.cuh; routes: model_route.h).  Included by launch.h inside namespace tdk.
#pragma once
#include "model_route.h"

// what every row kernel of the loss stage needs: the targets of TDMPC2._update (tdmpc2.py:285-304) and where the per-row terms go
struct ModelLossArgs {
    int num_bins;
    float vmin, vmax, bin_size;
    const float *bins;        // [num_bins] bin centres (two_hot_inv)
    const float *t_reward;    // [H, B] or null
    const float *t_td;        // [H, B] or null
    const float *t_term;      // [H, B] or null
    float *rowloss;           // [3 + num_q][HB] per-row loss terms (MK_* of model_route.h), or null: no losses asked for
    long HB;
    const unsigned int *err;  // layered family: the handle's fault word (a bounded wait gave up: every output is NaN), else null
};

// optional outputs of the rollout (tdmpc2_model_out, device pointers)
struct ModelOutArgs {
    float *rew_logits, *rew, *q_logits, *q, *term_logit;
};

// fused family: ks_value_roll (grid: row tiles) and ks_value_chain (grid: row tiles x steps x chains)
struct ModelParams {
    int B, H, A, Apad, nq, nnets, steps;
    NetS dyn, rew, term;
    NetS q[MAXQ];
    const float *z0;        // [B, L]
    const float *actions;   // [H, B, A]
    float *zs;              // [H + 1, B, L]: the caller's output or the handle's workspace; zs[0] is written by the host
    int chain[1 + MAXQ];    // chain of blockIdx.z (MC_* of model_route.h)
    ModelOutArgs out;
    ModelLossArgs ls;
    const int *task_ids;    // [B] or null (single task)
    const float *beff_tab;  // [n_tasks, nnets, WIDTH] effective first-layer biases
};

// layered family: one head's logits [rows, ld] -> logits / value outputs and the per-row loss term
struct ModelHeadRowsParams {
    const float *lg;
    int ld, rows, B, kind;  // kind: MK_REW | MK_Q0 + i | MK_TERM; B: batch rows (MK_TERM: row - B is the target's row)
    long row0;              // first row of this launch in the stage (chunked termination stage)
    float *logits_out;      // [rows, max(num_bins, 1)] or null
    float *val_out;         // [rows] or null (MK_TERM: the logit)
    ModelLossArgs ls;
};

// zs[1:] against next_z: rowloss[MK_CONS][row] = sum_c (zs[B + row, c] - next_z[row, c])^2
struct ModelConsParams {
    const float *zs1, *next_z;
    int rows, L;
    float *rowloss;
};

// the fixed-order final add (one workgroup)
struct ModelTailParams {
    const float *rowloss;
    int B, H, L, nq, episodic;
    float rho_pow[MODEL_MAXH];   // rho^t as the reference forms it (a Python float power, tdmpc2.py:274)
    float coef[4];               // consistency, reward, value, termination
    float *losses;               // [5] consistency, reward, value, termination, total
    float *step_means;           // [4, H] unweighted per-step batch means, or null
    const unsigned int *err;
};

// X operand columns [0, L) -> fp32 rows (layered family, the latent a dynamics step wrote)
struct ModelGetZParams {
    const float *X;
    int ldx, L, rows, split;
    float *out;                  // [rows, L]
    const unsigned int *err;
};
