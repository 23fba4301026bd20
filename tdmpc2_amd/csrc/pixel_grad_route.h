// The pixel encoder in training (tdmpc2_pixgrad_*, include/tdmpc2_pixel_grad.h): what the forward saves, the GEMM views of the
// backward, their tiles and grids, the order of every sum, the workspace offsets and the refusals, as pure functions.  Geometry
// and the forward's GEMM view are pixel_route.h's and pixel_batch_route.h's.  pixel_grad_kernels.cuh and k_pixel_grad.hip call these;
// tests/test_pixel_grad_route.py compiles this header with g++ and checks them on the CPU.
//
// Layer l (0..3) of the forward is D [rows, C] = A [rows, K_l] B [K_l, C] with rows = n pix_hw(l) output pixels of consecutive
// images (pixel_batch_route.h).  With dy_l [n][C][pix_hw(l)] the gradient of layer l's pre-activation:
//   DW   dW_l [m, co] = sum_r A [r, m] dy_l [r, co]     m = (ci k + ky) k + kx in the Conv2d order, and one more row m = K_l whose
//                                                       A is 1.0: that row is db_l, summed in dW's order
//        The reduction over the rows r is cut into chunks of PG_CHUNK consecutive rows and a chunk into sub-chains of PG_SUB rows.  A
//        sub-chain is one fmaf chain from zero over its rows in rising order (the 32x32x2 MFMA adds row 2 s, then row 2 s + 1 of
//        step s); the chunk's partial starts from zero and adds its sub-chains in rising order, and is written to the workspace:
//        part [chunk][m][co].  A second launch adds an element's partials: groups of PG_FOLD consecutive chunks, each
//        group summed from zero in rising order, then the group sums added from zero in rising order.  Both depend on n alone.
//   DA   da_{l-1} [q, ci] = sum_kk dy_l [src(q, kk)] W_l [co, ci, ky, kx]   q = an input pixel of layer l, kk = (co k + ky) k + kx
//        The transposed convolution, l = 3, 2, 1: src is the output pixel ((y - ky) / S, (x - kx) / S) when both divide and lie
//        inside the map; every other term multiplies zero.  One element is one wave's sum: fmaf chains of PG_DA_SEG steps (2 terms
//        each) from zero, each added to the element's total (from zero) in rising order.  The epilogue multiplies by the ReLU mask
//        a_{l-1} > 0 and writes dy_{l-1}.
#pragma once
#include "pixel_batch_route.h"

constexpr int PG_CHUNK = PIXB_WG_ROWS;  // rows of a dW / db partial chain: 256, one workgroup (layer 0 stages the forward's patch)
constexpr int PG_SUB = 32;              // rows of a sub-chain (16 MFMA steps): a chunk's partial adds eight of them
constexpr int PG_FOLD = 32;             // partials per group of the second stage
constexpr int PG_DA_SEG = 128;          // MFMA steps (256 terms) per partial chain of da
constexpr int PG_FOLD_THREADS = 256;
constexpr int PG_ROW_THREADS = 256;
constexpr int PG_MAX_N = 1 << 20;
// launches of one backward with every output asked for: the seed, three transposed convolutions, and per layer the partials and
// their fold.  n does not change it; a NULL dW / db pair drops that layer's two.
constexpr int PG_LAUNCHES = 1 + 3 + 2 * PIX_LAYERS;
constexpr int PG_FWD_LAUNCHES = 1 + PIX_LAYERS;  // the re-pack and the four layers

struct PgDesc {  // = tdmpc2_pixgrad_desc
    int32_t n, cin, C, obs_dtype, seed_is_preact;
    uint32_t reserved;
};

enum { PG_OK = 0, PG_BAD_N, PG_BAD_CIN, PG_BAD_C, PG_BAD_DTYPE, PG_BAD_SEED, PG_TOO_LARGE };
__host__ __device__ inline int pg_check(const PgDesc &d) {
    if (d.n < 1) return PG_BAD_N;
    if (d.cin < 1 || d.cin > PIX_MAX_CIN) return PG_BAD_CIN;
    if (d.C < PIX_MIN_C || d.C > PIX_MAX_C || d.C % PIX_CO != 0) return PG_BAD_C;
    if (d.obs_dtype != 0 && d.obs_dtype != 1) return PG_BAD_DTYPE;
    if (d.seed_is_preact != 0 && d.seed_is_preact != 1) return PG_BAD_SEED;
    if (d.n > PG_MAX_N) return PG_TOO_LARGE;
    return PG_OK;
}

// ---- what the forward keeps: acts = [n][pix_ws_floats(C)] (post-ReLU outputs of layers 0..2, the batch route's layout), then z [n][16 C]
__host__ __device__ inline size_t pg_z_off(int n, int C) { return (size_t)n * pix_ws_floats(C); }
__host__ __device__ inline size_t pg_acts_floats(int n, int C) { return (size_t)n * (pix_ws_floats(C) + (size_t)pix_hw(3) * C); }
// fwd_ws: the four weights as [cin_l][k][k][C], one after the other
__host__ __device__ inline size_t pg_wp_floats(int l, int cin, int C) { return (size_t)pixb_k(l, pixb_cin(l, cin, C)) * C; }
__host__ __device__ inline size_t pg_wp_off(int l, int cin, int C) {
    size_t o = 0;
    for (int j = 0; j < l; ++j) o += pg_wp_floats(j, cin, C);
    return o;
}
__host__ __device__ inline size_t pg_fwd_ws_floats(int cin, int C) { return pg_wp_off(PIX_LAYERS, cin, C); }

// ---- DW
__host__ __device__ inline int pg_dw_m(int l, int cin, int C) { return pixb_k(l, pixb_cin(l, cin, C)) + 1; }  // taps + the bias row
__host__ __device__ inline int pg_dw_tap_tiles(int M) { return (M + PIXB_TILE - 1) / PIXB_TILE; }
__host__ __device__ inline int pg_dw_tiles(int l, int cin, int C) { return pg_dw_tap_tiles(pg_dw_m(l, cin, C)) * pixb_col_tiles(C); }
__host__ __device__ inline PixbTap pg_tap(int l, int m) {  // Conv2d order
    const int K = pix_kernel(l), kk = K * K;
    return PixbTap{m / kk, m % kk / K, m % K};
}
__host__ __device__ inline PixbSrc pg_dw_src(int l, long r, int m) { return pixb_src(l, r, pg_tap(l, m)); }
__host__ __device__ inline int pg_a_off(int l, PixbTap t) {
    return l == 0 ? pixb_l0_patch_off(t.ci, t.ky, t.kx) : (t.ci * pix_side(l) + t.ky) * pix_side(l) + t.kx;
}
__host__ __device__ inline long pg_chunks(int l, int n) { return (pixb_rows(l, n) + PG_CHUNK - 1) / PG_CHUNK; }
__host__ __device__ inline int pg_chunk_rows(int l, int n, long chunk) {
    const long left = pixb_rows(l, n) - chunk * PG_CHUNK;
    return left < PG_CHUNK ? (int)left : PG_CHUNK;
}
// the grid of the partials' launch: x = chunks; y splits a chunk's tiles between workgroups (layer 0 keeps one: it stages the patch once).
// Tile t of a chunk = (tap tile t / col_tiles, column tile t % col_tiles) belongs to wave (t % (8 y)) % 8 of workgroup y = (t % (8 y)) / 8.
__host__ __device__ inline int pg_dw_grid_y(int l, int cin, int C) {
    return l == 0 ? 1 : (pg_dw_tiles(l, cin, C) + PIXB_WAVES - 1) / PIXB_WAVES;
}
__host__ __device__ inline size_t pg_dw_lds(int l, int cin) {
    return (size_t)PG_CHUNK * 8 + (l == 0 ? (size_t)cin * PIXB_L0_SLOTS * PIX_IN * 4 : 0);
}
// the rows' parts of the operand addresses, relative to the chunk's first image e0: A (the LDS patch, or acts) and B (dy_l)
__host__ __device__ inline int pg_row_a(int l, int C, const PixbStage &sg, int e0, long r) {
    const int e = pixb_row_image(l, r), px = pixb_row_pixel(l, r);
    if (l == 0) return pixb_l0_patch_off(0, pixb_l0_slot(sg, e, pix_stride(0) * (px / pix_out(0))), pix_stride(0) * (px % pix_out(0)));
    return (int)((size_t)(e - e0) * pix_ws_floats(C) + pix_ws_off(l - 1, C)) + pixb_a_base(l, px);
}
__host__ __device__ inline int pg_row_b(int l, int C, int e0, long r) {
    return (pixb_row_image(l, r) - e0) * C * pix_hw(l) + pixb_row_pixel(l, r);
}
__host__ __device__ inline size_t pg_part_off(int M, int C, long chunk, int m, int co) { return ((size_t)chunk * M + m) * C + co; }
__host__ __device__ inline long pg_fold_groups(long chunks) { return (chunks + PG_FOLD - 1) / PG_FOLD; }
__host__ __device__ inline long pg_fold_group(long chunk) { return chunk / PG_FOLD; }
__host__ __device__ inline int pg_fold_blocks(int M, int C) { return (M * C + PG_FOLD_THREADS - 1) / PG_FOLD_THREADS; }

// ---- DA (l = 1..3): rows = the n pix_hw(l - 1) input pixels of layer l, columns = its C input channels, K = C k k
__host__ __device__ inline int pg_da_k(int l, int C) { return C * pix_kernel(l) * pix_kernel(l); }
__host__ __device__ inline int pg_da_steps(int l, int C) { return (pg_da_k(l, C) + PIXB_KSTEP - 1) / PIXB_KSTEP; }
__host__ __device__ inline int pg_da_segs(int l, int C) { return (pg_da_steps(l, C) + PG_DA_SEG - 1) / PG_DA_SEG; }
__host__ __device__ inline long pg_da_rows(int l, int n) { return (long)n * pix_hw(l - 1); }
struct PgDaK {
    int co, ky, kx;
};
__host__ __device__ inline PgDaK pg_da_decode(int l, int kk) {
    const int K = pix_kernel(l), k2 = K * K;
    return PgDaK{kk / k2, kk % k2 / K, kk % K};
}
struct PgDaSrc {
    int valid, image, co, oy, ox;
};
__host__ __device__ inline PgDaSrc pg_da_src(int l, long q, int kk) {
    const PgDaK t = pg_da_decode(l, kk);
    const int S = pix_stride(l), side = pix_side(l), hw = side * side;
    const int px = (int)(q % hw), ty = px / side - t.ky, tx = px % side - t.kx;
    const bool ok = ty >= 0 && tx >= 0 && ty % S == 0 && tx % S == 0 && ty / S < pix_out(l) && tx / S < pix_out(l);
    return PgDaSrc{ok ? 1 : 0, (int)(q / hw), t.co, ok ? ty / S : 0, ok ? tx / S : 0};
}
__host__ __device__ inline int pg_da_w_off(int l, int C, int kk, int ci) {  // inside the Conv2d tensor [C][C][k][k]
    const PgDaK t = pg_da_decode(l, kk);
    const int K = pix_kernel(l);
    return ((t.co * C + ci) * K + t.ky) * K + t.kx;
}
__host__ __device__ inline long pg_da_blocks(int l, int n) { return (pg_da_rows(l, n) + PIXB_WG_ROWS - 1) / PIXB_WG_ROWS; }
__host__ __device__ inline size_t pg_da_lds(int l, int C) { return (size_t)(pg_da_k(l, C) + 1) * 16; }
__host__ __device__ inline PixbItem pg_da_item(int l, int n, long block, int wave) {
    const long row0 = block * PIXB_WG_ROWS + (long)wave * PIXB_TILE, left = pg_da_rows(l, n) - row0;
    return PixbItem{row0, left <= 0 ? 0 : left < PIXB_TILE ? (int)left : PIXB_TILE};
}

// ---- bwd_ws (float offsets): dy_0 .. dy_3, each [n][C][pix_hw(l)], then the partials of the layer in flight (the largest layer's room)
__host__ __device__ inline size_t pg_dy_floats(int l, int n, int C) { return (size_t)n * C * pix_hw(l); }
__host__ __device__ inline size_t pg_dy_off(int l, int n, int C) {
    size_t o = 0;
    for (int j = 0; j < l; ++j) o += pg_dy_floats(j, n, C);
    return o;
}
__host__ __device__ inline size_t pg_dy_elem(int l, int C, size_t image, int c, int px) { return (image * C + c) * pix_hw(l) + px; }
__host__ __device__ inline size_t pg_part_base(int n, int C) { return pg_dy_off(PIX_LAYERS, n, C); }
__host__ __device__ inline size_t pg_part_floats(int l, int n, int cin, int C) { return (size_t)pg_chunks(l, n) * pg_dw_m(l, cin, C) * C; }
__host__ __device__ inline size_t pg_bwd_ws_floats(int n, int cin, int C) {
    size_t most = 0;
    for (int l = 0; l < PIX_LAYERS; ++l) {
        const size_t f = pg_part_floats(l, n, cin, C);
        most = f > most ? f : most;
    }
    return pg_part_base(n, C) + most;
}
