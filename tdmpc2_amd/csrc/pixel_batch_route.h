// The pixel encoder's batch route (pixel_batch_kernels.cuh): the four convolutions as exact-fp32 implicit GEMMs on
// v_mfma_f32_32x32x2_f32, for calls of any number of images (training batches: (H + 1) B frame stacks).  This header decides
// the GEMM view of a layer (which output element a row / column is, which tap a k-index is, which input element a (row, k)
// reads), the work decomposition (tiles, grid, LDS, the item of a wave, the element of an accumulator register), layer 0's
// staging of the resampled patch, and the passes of a call over the reserved workspace.  Geometry, workspace layout and the
// ShiftAug table are pixel_route.h's.  Pure functions; pixel_batch_kernels.cuh and plan_obs.hip call them,
// tests/test_pixel_batch_route.py compiles this header with g++ and checks them on the CPU (tests/pixel_batch_route_model.py).
#pragma once
#include "pixel_route.h"

// ---------------------------------------------------------------------------------------------------------------------------
// GEMM view of layer l:  D [rows, cols] = A [rows, K] * B [K, cols]
//   rows   output pixels of consecutive images: row r = image r / pix_hw(l), pixel r % pix_hw(l) (row-major (oy, ox)); a tile of
//          PIXB_TILE rows may straddle images (layer 3 has 16 pixels per image: a tile holds two)
//   cols   the C output channels, padded to whole tiles; padding columns multiply zero weights and are never stored
//   K      cin k k taps, padded to whole trips of the kernel's k-loop (PIXB_KGROUP instructions of k-step PIXB_KSTEP); a padding
//          step multiplies a zero weight (and a zero input)
// The order of k is the order in which k_pix_spread (pixel_kernels.cuh) adds a pixel's terms, so that the MFMA's fmaf chain
// repeats it: layer 0 runs (ky, kx) outside and the input channel inside, layers 1..3 the input channel outside and (ky, kx)
// inside.  Either way B's row for k is row (ci k k + ky k + kx) of the bound weights [cin][ky][kx][C], read where they are.
constexpr int PIXB_TILE = 32;    // rows and columns of an accumulator tile (32x32x2 MFMA)
constexpr int PIXB_KSTEP = 2;    // k per instruction: lanes 0..31 hold k = 2 s, lanes 32..63 k = 2 s + 1
constexpr int PIXB_KGROUP = 4;   // instructions per trip of the k-loop
constexpr int PIXB_WAVES = 8;    // waves of a workgroup: consecutive row tiles
constexpr int PIXB_THREADS = 64 * PIXB_WAVES;
constexpr int PIXB_WG_ROWS = PIXB_TILE * PIXB_WAVES;  // 256
constexpr int PIXB_ACC = 16;     // accumulator registers per lane

__host__ __device__ constexpr int pixb_cin(int l, int cin, int C) { return l == 0 ? cin : C; }  // input channels of layer l
__host__ __device__ constexpr int pixb_k(int l, int cin_l) { return cin_l * pix_kernel(l) * pix_kernel(l); }
__host__ __device__ constexpr int pixb_k_steps(int l, int cin_l) { return (pixb_k(l, cin_l) + PIXB_KSTEP - 1) / PIXB_KSTEP; }
__host__ __device__ constexpr int pixb_k_pad(int l, int cin_l) {
    return (pixb_k_steps(l, cin_l) + PIXB_KGROUP - 1) / PIXB_KGROUP * PIXB_KGROUP * PIXB_KSTEP;
}
__host__ __device__ constexpr int pixb_col_tiles(int C) { return (C + PIXB_TILE - 1) / PIXB_TILE; }
__host__ __device__ constexpr long pixb_rows(int l, int n) { return (long)n * pix_hw(l); }

struct PixbTap {
    int ci, ky, kx;
};
// k-index (k < pixb_k) -> tap
__host__ __device__ inline PixbTap pixb_k_decode(int l, int cin_l, int k) {
    const int K = pix_kernel(l), kk = K * K;
    const int ci = l == 0 ? k % cin_l : k / kk, tap = l == 0 ? k / cin_l : k % kk;
    return PixbTap{ci, tap / K, tap % K};
}
// float offset of B's row k inside the bound weights of layer l
__host__ __device__ inline int pixb_w_off(int l, int cin_l, int C, int k) {
    const PixbTap t = pixb_k_decode(l, cin_l, k);
    const int K = pix_kernel(l);
    return ((t.ci * K + t.ky) * K + t.kx) * C;
}

// (row, tap) -> the element of layer l's input that A [row, k] is: image, channel, (y, x) of the layer's input map
// (pix_side(l) squared; for layer 0 the ShiftAug-resampled, preprocessed frame)
struct PixbSrc {
    int image, ci, y, x;
};
__host__ __device__ inline int pixb_row_image(int l, long r) { return (int)(r / pix_hw(l)); }
__host__ __device__ inline int pixb_row_pixel(int l, long r) { return (int)(r % pix_hw(l)); }
__host__ __device__ inline PixbSrc pixb_src(int l, long r, PixbTap t) {
    const int p = pixb_row_pixel(l, r), oy = p / pix_out(l), ox = p % pix_out(l);
    return PixbSrc{pixb_row_image(l, r), t.ci, pix_stride(l) * oy + t.ky, pix_stride(l) * ox + t.kx};
}
// (layer, row, k-index) -> source element: the two maps above composed (k < pixb_k(l, cin_l))
__host__ __device__ inline PixbSrc pixb_src(int l, int cin_l, long r, int k) { return pixb_src(l, r, pixb_k_decode(l, cin_l, k)); }

// ---------------------------------------------------------------------------------------------------------------------------
// Layer 0's staging.  A workgroup's PIXB_WG_ROWS rows are whole or partial output rows g = image * 29 + oy of at most two
// images (256 < 841); output row oy reads input rows 2 oy .. 2 oy + 6.  The workgroup resamples, ONCE per element, the input rows
// its output rows read -- rows [yA0, yA0 + nA) of its first image in slots 0 .. nA - 1, rows [0, nB) of the next image behind
// them -- for every input channel and all 64 columns into LDS: patch[ci][slot][64].
constexpr int PIXB_L0_SLOTS = 2 * ((PIXB_WG_ROWS - 1) / 29 + 2) + 10;  // 2 G + 10 for G output rows over two images: 30
struct PixbStage {
    int eA, yA0, nA, nB;  // first image, its first staged input row, staged rows of the first / the second image
};
// r0, r1: first and last (valid) row of the workgroup
__host__ __device__ inline PixbStage pixb_l0_stage(long r0, long r1) {
    const int o = pix_out(0), S = pix_stride(0), K = pix_kernel(0);
    const long g0 = r0 / o, g1 = r1 / o;
    const int eA = (int)(g0 / o), eZ = (int)(g1 / o);
    const int oyA0 = (int)(g0 % o), oyA1 = eZ == eA ? (int)(g1 % o) : o - 1;
    PixbStage s{eA, S * oyA0, S * (oyA1 - oyA0) + K, 0};
    if (eZ != eA) s.nB = S * (int)(g1 % o) + K;
    return s;
}
__host__ __device__ inline int pixb_l0_slot(const PixbStage &s, int image, int y) { return image == s.eA ? y - s.yA0 : s.nA + y; }
__host__ __device__ inline int pixb_l0_patch_off(int ci, int slot, int x) { return (ci * PIXB_L0_SLOTS + slot) * PIX_IN + x; }

// A [row, k] = base(row) + pixb_a_off(k): the k-dependent part of the input element's address -- in the LDS patch (layer 0: the
// row's base is pixb_l0_patch_off(0, slot of input row 2 oy, 2 ox)) or in the image's previous-layer output [C][side][side]
// (layers 1..3: the base is (S oy) side + S ox inside it).
__host__ __device__ inline int pixb_a_off(int l, int cin_l, int k) {
    const PixbTap t = pixb_k_decode(l, cin_l, k);
    if (l == 0) return pixb_l0_patch_off(t.ci, t.ky, t.kx);
    return (t.ci * pix_side(l) + t.ky) * pix_side(l) + t.kx;
}
__host__ __device__ inline int pixb_a_base(int l, int pixel) {  // layers 1..3
    return (pix_stride(l) * (pixel / pix_out(l))) * pix_side(l) + pix_stride(l) * (pixel % pix_out(l));
}

// ---------------------------------------------------------------------------------------------------------------------------
// Work decomposition.  One launch per layer (the stream orders them; no workgroup waits for another), grid x = workgroups of
// PIXB_WG_ROWS rows.  Wave w of workgroup b owns rows [row0, row0 + PIXB_TILE) and, one after the other, every column tile.  LDS:
// the k table (A offset, B offset per padded k) and, for layer 0, the patch.
__host__ __device__ inline size_t pixb_lds(int l, int C, int cin) {
    const size_t tab = (size_t)pixb_k_pad(l, pixb_cin(l, cin, C)) * 8;
    return tab + (l == 0 ? (size_t)cin * PIXB_L0_SLOTS * PIX_IN * 4 : 0);
}
inline PixGrid pixb_grid(int l, int n, int C, int cin) {
    return PixGrid{(int)((pixb_rows(l, n) + PIXB_WG_ROWS - 1) / PIXB_WG_ROWS), 1, 1, PIXB_THREADS, pixb_lds(l, C, cin)};
}
struct PixbItem {
    long row0;
    int rows;  // valid rows of the tile (0: the wave has nothing to do)
};
__host__ __device__ inline PixbItem pixb_item(int l, int n, int block, int wave) {
    const long row0 = (long)block * PIXB_WG_ROWS + (long)wave * PIXB_TILE, left = pixb_rows(l, n) - row0;
    return PixbItem{row0, left <= 0 ? 0 : left < PIXB_TILE ? (int)left : PIXB_TILE};
}
// the element of accumulator register i of lane `lane` inside its tile (the 32 x 32 C/D layout); the eight rows 8 g .. 8 g + 7
// of a column -- one SimNorm group of layer 3, whose rows are image * 16 + 4 y + x -- are registers 4 g .. 4 g + 3 of lanes
// c and c + 32
__host__ __device__ constexpr int pixb_acc_row(int lane, int i) { return 8 * (i / 4) + 4 * (lane / 32) + i % 4; }
__host__ __device__ constexpr int pixb_acc_col(int lane) { return lane % 32; }

// ---------------------------------------------------------------------------------------------------------------------------
// Chunking: a call of n images runs as passes over a workspace reserved for `chunk` images (pix_ws_floats(C) each, the spread
// route's layout and offsets); pass i encodes images [pixb_chunk_begin, + pixb_chunk_count).
__host__ __device__ inline int pixb_chunks(int n, int chunk) { return (n + chunk - 1) / chunk; }
__host__ __device__ inline int pixb_chunk_begin(int i, int chunk) { return i * chunk; }
__host__ __device__ inline int pixb_chunk_count(int n, int chunk, int i) {
    const int left = n - i * chunk;
    return left < chunk ? left : chunk;
}
inline size_t pixb_ws_bytes(int chunk, int C) { return (size_t)chunk * pix_ws_floats(C) * 4; }
