// State-observation encoder: the limits and the parameter blocks its kernels (encoder_kernels.cuh, instantiated in k_plan.hip)
// share with the host side (plan_obs.hip launches, plan_weights.hip binds), through launch.h.
#pragma once

constexpr int ENC_MAX_LAYERS = 6;    // num_enc_layers is 2..5 in the reference's model table (common/__init__.py:1-24)
constexpr int ENC_THREADS = 512;
constexpr int ENC_MAX_PER_THREAD = 8;  // output features per thread: widths up to 4096 (the 317M model's enc_dim)

struct EncLayerDev {
    const float *wt;    // [in][out], transposed nn.Linear weight
    const float *bias;  // [out]
    const float *g, *b; // LayerNorm affine [out]
    int in, out;
};
struct EncodeArgs {
    EncLayerDev l[ENC_MAX_LAYERS];
    int nl;
    int obs_dim, T, maxw, simnorm_dim;
    const float *obs;       // [E, obs_dim]
    const float *task_emb;  // [E, T] or null
    float *z;               // [E, latent_dim]
};

// A layer beyond ENC_WIDE columns takes the layer-at-a-time route (k_enc_gemv + k_enc_norm: encoder_kernels.cuh).
constexpr int ENC_WIDE = 1024;
// k_enc_gemv holds the whole input row plus its partials in dynamic LDS, (in + 256) floats, and a launch may ask for 64 KiB of
// it: the widest input a layer may have.  Only an observation can be wider than a layer (4096), so this is a limit on obs_dim.
constexpr size_t ENC_GEMV_LDS_MAX = 64 * 1024;
constexpr int ENC_MAX_IN = (int)(ENC_GEMV_LDS_MAX / 4) - 256;

struct EncGemvArgs {
    const float *wt, *bias;  // [in][out], [out]
    const float *x;          // [E, ldx] activations (layer 0: obs | task_emb assembled by the caller kernel)
    const float *obs, *emb;  // layer 0 only: obs [E, obs_dim], emb [E, T] (x = null)
    int obs_dim, T;
    int in, out, ldx;
    float *y;                // [E, out] pre-activations
};
struct EncNormArgs {
    const float *y;      // [E, width] pre-activations
    const float *g, *b;  // [width]
    float *out;          // [E, width]: Mish(LN(y)) (hidden layers) or SimNorm(LN(y)) (last layer = z)
    int width, last, simnorm_dim;
};
