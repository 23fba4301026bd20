"""tdmpc2_amd/csrc/pixel_grad_route.h compiled with the host compiler (tests/route_shim.py): a C shim whose `pg_walk` checks the
header's maps against each other and against pixel_batch_route.h, element by element, and returns 0 or the line of the first check
that failed; the same source with a main() is the stand-alone program the sanitizer build runs."""
import ctypes as C

from tests import route_shim

SHIM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pixel_grad_route.h"
#define CHECK(c) do { if (!(c)) return __LINE__; } while (0)

extern "C" {
int pg_launches() { return PG_LAUNCHES; }
int pg_fwd_launches() { return PG_FWD_LAUNCHES; }
int pg_consts(int *out) { out[0] = PG_CHUNK; out[1] = PG_SUB; out[2] = PG_FOLD; out[3] = PG_DA_SEG; out[4] = PG_MAX_N; return 5; }
int pg_check_c(int n, int cin, int Cc, int dt, int seed) { return pg_check(PgDesc{n, cin, Cc, dt, seed, 0u}); }
unsigned long long pg_dy_off_c(int l, int n, int Cc) { return pg_dy_off(l, n, Cc); }
unsigned long long pg_part_base_c(int n, int Cc) { return pg_part_base(n, Cc); }
unsigned long long pg_bwd_ws_floats_c(int n, int cin, int Cc) { return pg_bwd_ws_floats(n, cin, Cc); }
unsigned long long pg_acts_floats_c(int n, int Cc) { return pg_acts_floats(n, Cc); }
unsigned long long pg_z_off_c(int n, int Cc) { return pg_z_off(n, Cc); }
unsigned long long pg_fwd_ws_floats_c(int cin, int Cc) { return pg_fwd_ws_floats(cin, Cc); }
unsigned long long pg_wp_off_c(int l, int cin, int Cc) { return pg_wp_off(l, cin, Cc); }
unsigned long long pg_part_off_c(int M, int Cc, long chunk, int m, int co) { return pg_part_off(M, Cc, chunk, m, co); }
unsigned long long pg_dy_elem_c(int l, int Cc, unsigned long long image, int c, int px) { return pg_dy_elem(l, Cc, image, c, px); }
long pg_chunks_c(int l, int n) { return pg_chunks(l, n); }
int pg_chunk_rows_c(int l, int n, long chunk) { return pg_chunk_rows(l, n, chunk); }
long pg_fold_groups_c(long chunks) { return pg_fold_groups(chunks); }
long pg_fold_group_c(long chunk) { return pg_fold_group(chunk); }
int pg_da_segs_c(int l, int Cc) { return pg_da_segs(l, Cc); }
int pg_da_steps_c(int l, int Cc) { return pg_da_steps(l, Cc); }

// every check of one (n, C, cin): 0, or the line that failed
int pg_walk(int n, int Cc, int cin) {
    for (int l = 0; l < PIX_LAYERS; ++l) {
        const int cin_l = pixb_cin(l, cin, Cc), K = pixb_k(l, cin_l), M = pg_dw_m(l, cin, Cc), ctiles = pixb_col_tiles(Cc);
        CHECK(M == K + 1);
        // ---- DW: every tile of a chunk belongs to exactly one (workgroup y, wave, trip); every element of the tiles is one register
        const int tiles = pg_dw_tiles(l, cin, Cc), gy = pg_dw_grid_y(l, cin, Cc);
        CHECK(l != 0 || gy == 1);
        std::vector<int> seen(tiles, 0), cover((size_t)M * Cc, 0);
        for (int y = 0; y < gy; ++y)
            for (int w = 0; w < PIXB_WAVES; ++w)
                for (int t = y * PIXB_WAVES + w; t < tiles; t += PIXB_WAVES * gy) {
                    seen[t]++;
                    const int tt = t / ctiles, ct = t % ctiles;
                    for (int lane = 0; lane < 64; ++lane)
                        for (int i = 0; i < PIXB_ACC; ++i) {
                            const int mr = tt * PIXB_TILE + pixb_acc_row(lane, i), col = ct * PIXB_TILE + pixb_acc_col(lane);
                            if (mr < M && col < Cc) cover[(size_t)mr * Cc + col]++;
                        }
                }
        for (int t = 0; t < tiles; ++t) CHECK(seen[t] == 1);
        for (size_t i = 0; i < cover.size(); ++i) CHECK(cover[i] == 1);
        // the taps are the Conv2d order and name the forward's source elements
        for (int m = 0; m < K; ++m) {
            const PixbTap t = pg_tap(l, m);
            CHECK((t.ci * pix_kernel(l) + t.ky) * pix_kernel(l) + t.kx == m && t.ci < cin_l && t.ky < pix_kernel(l) && t.kx < pix_kernel(l));
        }
        // ---- chunks: consecutive, whole, the last one short; rows of a chunk and their operand offsets
        const long rows = pixb_rows(l, n), chunks = pg_chunks(l, n);
        long total = 0;
        for (long c = 0; c < chunks; ++c) {
            const int cr = pg_chunk_rows(l, n, c);
            CHECK(cr >= 1 && cr <= PG_CHUNK && (c == chunks - 1 || cr == PG_CHUNK));
            CHECK(pg_fold_group(c) == c / PG_FOLD && pg_fold_group(c) < pg_fold_groups(chunks));
            const long r0 = c * PG_CHUNK;
            const int e0 = pixb_row_image(l, r0);
            PixbStage sg{};
            if (l == 0) {
                sg = pixb_l0_stage(r0, r0 + cr - 1);
                CHECK(sg.nA + sg.nB <= PIXB_L0_SLOTS);
            }
            for (int i = 0; i < cr; i += (cr > 40 ? 7 : 1)) {
                const long r = r0 + i;
                const int ra = pg_row_a(l, Cc, sg, e0, r), rb = pg_row_b(l, Cc, e0, r);
                CHECK(rb == (pixb_row_image(l, r) - e0) * Cc * pix_hw(l) + pixb_row_pixel(l, r) && rb >= 0);
                for (int m = 0; m < K; m += (K > 60 ? 13 : 1)) {
                    const PixbSrc s = pg_dw_src(l, r, m), f = pixb_src(l, r, pg_tap(l, m));
                    CHECK(s.image == f.image && s.ci == f.ci && s.y == f.y && s.x == f.x);
                    CHECK(s.y >= 0 && s.y < pix_side(l) && s.x >= 0 && s.x < pix_side(l) && s.image < n);
                    const int a = ra + pg_a_off(l, pg_tap(l, m));
                    if (l == 0) {
                        const int slot = pixb_l0_slot(sg, s.image, s.y);
                        CHECK(slot >= 0 && slot < sg.nA + sg.nB && a == pixb_l0_patch_off(s.ci, slot, s.x));
                    } else {
                        CHECK((size_t)a == (size_t)(s.image - e0) * pix_ws_floats(Cc) + pix_ws_off(l - 1, Cc) +
                                               ((size_t)s.ci * pix_side(l) + s.y) * pix_side(l) + s.x);
                    }
                }
            }
            total += cr;
        }
        CHECK(total == rows);
        CHECK(pg_part_floats(l, n, cin, Cc) == (size_t)chunks * M * Cc && pg_bwd_ws_floats(n, cin, Cc) >= pg_part_base(n, Cc) + pg_part_floats(l, n, cin, Cc));
        if (l == 0) continue;
        // ---- DA: the decoded tiles cover every (input pixel, channel) once
        const long q_rows = pg_da_rows(l, n);
        CHECK(q_rows == (long)n * pix_side(l) * pix_side(l));
        std::vector<int> qc((size_t)q_rows * Cc, 0);
        for (long b = 0; b < pg_da_blocks(l, n); ++b)
            for (int w = 0; w < PIXB_WAVES; ++w) {
                const PixbItem it = pg_da_item(l, n, b, w);
                for (int ct = 0; ct < ctiles; ++ct)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int i = 0; i < PIXB_ACC; ++i) {
                            const int tr = pixb_acc_row(lane, i), col = ct * PIXB_TILE + pixb_acc_col(lane);
                            if (tr < it.rows && col < Cc) qc[(size_t)(it.row0 + tr) * Cc + col]++;
                        }
            }
        for (size_t i = 0; i < qc.size(); ++i) CHECK(qc[i] == 1);
        // the source map is the transpose of the forward's: every valid (q, kk) is a forward (row, tap) whose source is q, and
        // there are as many of them as forward pairs; a tap between strides or outside the map is not valid
        const int KD = pg_da_k(l, Cc), S = pix_stride(l), side = pix_side(l), o = pix_out(l), k = pix_kernel(l);
        CHECK(KD == Cc * k * k && pg_da_steps(l, Cc) == (KD + 1) / 2 && pg_da_segs(l, Cc) == (pg_da_steps(l, Cc) + PG_DA_SEG - 1) / PG_DA_SEG);
        long valid = 0;
        for (int kk = 0; kk < KD; ++kk) {
            const PgDaK t = pg_da_decode(l, kk);
            CHECK((t.co * k + t.ky) * k + t.kx == kk && t.co < Cc && t.ky < k && t.kx < k);
        }
        for (long q = 0; q < q_rows; ++q)
            for (int kk = 0; kk < KD; kk = (kk + 1 == k * k && Cc > 1) ? (Cc - 1) * k * k : kk + 1) {  // the first and the last channel: co does not enter the geometry
                const PgDaK t = pg_da_decode(l, kk);
                const PgDaSrc s = pg_da_src(l, q, kk);
                const int px = (int)(q % (side * side)), y = px / side, x = px % side;
                const bool want = y >= t.ky && x >= t.kx && (y - t.ky) % S == 0 && (x - t.kx) % S == 0 && (y - t.ky) / S < o && (x - t.kx) / S < o;
                CHECK((s.valid != 0) == want);
                if (!s.valid) continue;
                if (t.co == 0) valid++;
                CHECK(s.image == (int)(q / (side * side)) && s.co == t.co && s.oy >= 0 && s.oy < o && s.ox >= 0 && s.ox < o);
                const PixbSrc f = pixb_src(l, (long)s.image * pix_hw(l) + s.oy * o + s.ox, PixbTap{0, t.ky, t.kx});
                CHECK(f.image == s.image && f.y == y && f.x == x);
                CHECK(pg_da_w_off(l, Cc, kk, 1) - pg_da_w_off(l, Cc, kk, 0) == k * k && pg_da_w_off(l, Cc, kk, 0) == (t.co * Cc * k + t.ky) * k + t.kx);
            }
        CHECK(valid == pixb_rows(l, n) * k * k);
    }
    // offsets: the dy regions follow each other, the partials come last
    for (int l = 0; l < PIX_LAYERS; ++l) CHECK(pg_dy_off(l + 1, n, Cc) == pg_dy_off(l, n, Cc) + (size_t)n * Cc * pix_hw(l));
    CHECK(pg_part_base(n, Cc) == pg_dy_off(PIX_LAYERS, n, Cc));
    CHECK(pg_acts_floats(n, Cc) == pg_z_off(n, Cc) + (size_t)n * 16 * Cc && pg_z_off(n, Cc) == (size_t)n * pix_ws_floats(Cc));
    return 0;
}
}
"""

MAIN = r"""
int main() {
    const int ns[] = {1, 2, 3, 17}, Cs[] = {8, 24, 32, 40, 64}, cins[] = {1, 9, 16};
    for (int n : ns) for (int c : Cs) for (int ci : cins) {
        const int rc = pg_walk(n, c, ci);
        if (rc) { std::printf("pg_walk(%d, %d, %d) failed at line %d\n", n, c, ci, rc); return 1; }
    }
    if (pg_dy_off(3, 1 << 20, 64) != (size_t)(1 << 20) * 64 * (841 + 169 + 36)) return 2;
    std::printf("ok\n");
    return 0;
}
"""

_u64, _i, _l = C.c_uint64, C.c_int, C.c_long
PROTOTYPES = {
    "pg_launches": ([], _i), "pg_fwd_launches": ([], _i), "pg_consts": ([C.POINTER(_i)], _i),
    "pg_check_c": ([_i] * 5, _i), "pg_dy_off_c": ([_i] * 3, _u64), "pg_part_base_c": ([_i] * 2, _u64),
    "pg_bwd_ws_floats_c": ([_i] * 3, _u64), "pg_acts_floats_c": ([_i] * 2, _u64), "pg_z_off_c": ([_i] * 2, _u64),
    "pg_fwd_ws_floats_c": ([_i] * 2, _u64), "pg_wp_off_c": ([_i] * 3, _u64), "pg_part_off_c": ([_i, _i, _l, _i, _i], _u64),
    "pg_dy_elem_c": ([_i, _i, _u64, _i, _i], _u64), "pg_chunks_c": ([_i, _i], _l), "pg_chunk_rows_c": ([_i, _i, _l], _i),
    "pg_fold_groups_c": ([_l], _l), "pg_fold_group_c": ([_l], _l), "pg_da_segs_c": ([_i, _i], _i), "pg_da_steps_c": ([_i, _i], _i),
    "pg_walk": ([_i] * 3, _i),
}


def build(tmpdir):
    return route_shim.build_shim(tmpdir, "pixel_grad_route", SHIM, PROTOTYPES)


def build_walk(tmpdir, sanitize):
    return route_shim.build_walk(tmpdir, "pixel_grad_route", SHIM + MAIN, sanitize=sanitize)
