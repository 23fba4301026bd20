// Kernel parameter blocks of tdmpc2_plan_policy_loss / running_scale / termination_stats (the forward of TDMPC2.update_pi after
// pi and Q, tdmpc2/tdmpc2.py:223-239; kernels: policy_loss_kernels.cuh).  Included by launch.h inside namespace tdk.
#pragma once

enum { PL_MAX_STEPS = 8, PL_SCALE_MAX_N = 16384, PL_THREADS = 1024 };

// RunningScale.update (common/scale.py:21-43) on n floats: one workgroup
struct RunningScaleParams {
    const float *x;      // [n]
    int n;
    float tau;
    float *scale;        // [1] read and written
    float *percentiles;  // [2] or null
    const unsigned int *err;  // layered family: the handle's fault word (set: the scale is left as it is, the percentiles are NaN), else null
};

// pi_loss and the info means from the per-row terms (one workgroup, fixed order)
struct PolicyLossTailParams {
    float *q, *entropy, *scaled_entropy;        // [T, B] each (read; NaN-filled on a fault of the layered GEMMs)
    const float *scale;                         // [1] RunningScale.value AFTER this call's update
    int B, T;
    float entropy_coef;
    float rho_pow[PL_MAX_STEPS + 1];
    float *step_means;                          // [3, T] or null
    float *loss;                                // [4] pi_loss, mean entropy, mean scaled_entropy, scale
    const unsigned int *err;                    // layered family: the handle's fault word (set: EVERY output is NaN), else null
    float *action;                              // [T, B, A] or null: NaN-filled on such a fault too (every piece's rows)
    int A;
};

// math.termination_statistics (common/math.py:97-109): one workgroup
struct TerminationStatsParams {
    const float *logit, *target;  // [n] each
    int n;
    float *stats;                 // [2] rate, f1
};
