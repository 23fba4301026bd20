"""The layered family's GEMM launches of one plan, as the host issues them -- every route from tdmpc2_amd/csrc/layer_route.h itself
(compiled with g++ behind the C shim below), the sequence and the handle's capacities from layered_host.cuh / tdmpc2_plan.hip.

Used by tests/test_layer_route.py (the route table of the benched geometries) and tests/test_tile_order.py (the dispatcher model of
the launches whose workgroups wait for each other)."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROUTE_SHIM = r"""
#include "layer_route.h"
static LayCtx ctx_of(const long *c, const int *knob) {
    return LayCtx{c[0], (int)c[1], c[2] != 0, c[3] != 0, c[4] != 0, (size_t)c[5], (size_t)c[6], c[7] != 0, (size_t)c[8], c[9] != 0,
                  (size_t)c[10], knob};
}
extern "C" void route(long rows_p, int rpe, int CT, int nk, int want, const long *c, const int *knob, long *out) {
    const LayRoute r = lay_route(LayIn{(size_t)rows_p, rpe, CT, nk, want}, ctx_of(c, knob));
    const long v[] = {r.w, r.nct, r.rt, r.sd, r.epi, r.nrowblk, r.ncolblk, r.ord.xcd_rows, r.ord.ncol_grid, r.ord.nblk, r.wo.parts,
                      r.wo.full, r.wo.max_tail, r.wo.per_xcd, r.wo.nblk, r.grid, (long)r.arrive, r.ln_after};
    for (int i = 0; i < 18; ++i) out[i] = v[i];
}
extern "C" int mid_ok_c(int split, int mid, int ksplit, int mws, int side, int row_env, long cus, int maxct, long rows_p) {
    return mid_ok(MidCtx{split != 0, mid != 0, ksplit, mws != 0, side != 0, row_env != 0, cus, maxct}, (size_t)rows_p) ? 1 : 0;
}
// in: rows, rows_p, rpe, n, rows_one_by_one, arrive_pending, mws_cap, then per problem CT, nk16, ln, actions, stats
extern "C" void mid_route_c(const long *in, const long *c, const int *knob, long *out) {
    MidIn m{(size_t)in[0], (size_t)in[1], (int)in[2], (int)in[3], {}, in[4] != 0, in[5] != 0, (size_t)in[6]};
    for (int i = 0; i < 2; ++i)
        m.pr[i] = MidProbIn{(int)in[7 + 5 * i], (int)in[8 + 5 * i], in[9 + 5 * i] != 0, in[10 + 5 * i] != 0, in[11 + 5 * i] != 0};
    const MidRoute r = mid_route(m, ctx_of(c, knob));
    long *o = out;
    *o++ = r.ws_ok; *o++ = r.split_xcd; *o++ = r.gblk; *o++ = r.nrow; *o++ = r.mr_threads; *o++ = r.serial; *o++ = r.rblk;
    for (int i = 0; i < 2; ++i) {
        const MidRoute::Prob &p = r.pr[i];
        *o++ = p.nk; *o++ = p.ncolblk; *o++ = p.nrowblk; *o++ = p.parts; *o++ = p.nblk; *o++ = p.epi; *o++ = p.reset; *o++ = (long)p.arrive;
        *o++ = p.nwg;
    }
}
extern "C" int knob_count() { return LK_COUNT; }
extern "C" void knob_spec(int i, int *out) { out[0] = LAY_KNOBS[i].def; out[1] = LAY_KNOBS[i].lo; out[2] = LAY_KNOBS[i].hi; }
"""

ROUTE_FIELDS = ("w", "nct", "rt", "sd", "epi", "nrowblk", "ncolblk", "xcd_rows", "ncol_grid", "ord_nblk", "parts", "full", "max_tail",
                "per_xcd", "wo_nblk", "grid", "arrive", "ln_after")
MID_FIELDS = ("ws_ok", "split_xcd", "gblk", "nrow", "mr_threads", "serial", "rblk")
MID_PROB_FIELDS = ("nk", "ncolblk", "nrowblk", "parts", "nblk", "epi", "reset", "arrive", "nwg")
LR_PLAIN, LR_MISH, LR_SIMNORM, LR_TWOHOT = 0, 1, 2, 3
CUS = 256


def build(tmpdir, extra_src=""):
    src = os.path.join(str(tmpdir), "route_shim.cpp")
    with open(src, "w") as f:
        f.write(ROUTE_SHIM + extra_src)
    so = os.path.join(str(tmpdir), "libroute_shim.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tdmpc2_amd", "csrc"), src, "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    ci, cl, pl, pi = ctypes.c_int, ctypes.c_long, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_int)
    lib.route.argtypes = [cl, ci, ci, ci, ci, pl, pi, pl]
    lib.mid_ok_c.argtypes = [ci, ci, ci, ci, ci, ci, cl, ci, cl]
    lib.mid_route_c.argtypes = [pl, pl, pi, pl]
    lib.knob_spec.argtypes = [ci, pi]
    return lib


def knob_defaults(lib):
    spec = (ctypes.c_int * 3)()
    out = []
    for i in range(lib.knob_count()):
        lib.knob_spec(i, spec)
        out.append(spec[0])
    return out


def _ru(x, m):
    return (x + m - 1) // m * m


class Handle:
    """What a layered, split-arithmetic handle created for E plans of `cfg` holds (tdmpc2_plan.hip: create, ksws_ensure), with the
    K-split mode set to `ksplit` after creation (tdmpc2_plan_set_tuning) and the arrival counters of the stage it is in."""

    def __init__(self, lib, cfg, E, ksplit=2, cus=CUS):
        self.lib, self.cfg, self.E, self.ksplit, self.cus = lib, cfg, E, ksplit, cus
        L, M, A, N = cfg.latent_dim, cfg.mlp_dim, cfg.action_dim, cfg.num_samples
        self.Kin, self.Mp = _ru(L + A, 32), M
        self.Ppad = _ru(max(cfg.num_pi_trajs, 1), 32)
        Rp = _ru(E * N, 128)
        self.maxct = (max(M, L) + 31) // 32
        self.stats_cap = Rp * ((self.maxct + 3) // 4) * 2
        self.arrive_cap = 64 * (Rp // 32) * 2
        ks_tiles = (Rp // 256) * ((self.maxct + 7) // 8) if Rp % 256 == 0 and self.maxct >= 8 else 0

        def slots(mode):
            cap = 8 * ((cus // 16 + 3) // 4 * 4) * 4 if mode == 2 else 8 * 32 * 4
            return min(cap, ks_tiles * 4) if ks_tiles and mode else 0
        self.ksws_slots = max(slots(2), slots(ksplit))  # created in mode 2, grown (never shrunk) by the mode set afterwards
        self.mws = (N + 127) // 128 * ((self.maxct + 7) // 8) <= cus
        self.mws_cap = cus * 128 * 256
        self.knob = (ctypes.c_int * lib.knob_count())(*knob_defaults(lib))
        self.arrive_off, self.pending = 0, False

    def ctx(self):
        return (ctypes.c_long * 11)(self.cus, self.ksplit, 1, 0, 1, self.arrive_off, self.arrive_cap, 1, self.stats_cap,
                                    int(self.ksws_slots > 0), self.ksws_slots)

    def mid_ok(self, rows_p):
        return bool(self.lib.mid_ok_c(1, 1, self.ksplit, int(self.mws), 1, 0, self.cus, self.maxct, rows_p))

    def gemm(self, rows_p, rpe, CT, nk, want):
        out = (ctypes.c_long * len(ROUTE_FIELDS))()
        self.lib.route(rows_p, rpe, CT, nk, want, self.ctx(), self.knob, out)
        r = dict(zip(ROUTE_FIELDS, out))
        self.arrive_off += r["arrive"]
        return r

    def mid(self, rows, rows_p, rpe, probs, one_by_one=False):
        """probs: [(CT, k16-blocks, ln, actions)] -- problem i uses statistics buffer i"""
        vals = [rows, rows_p, rpe, len(probs), int(one_by_one), int(self.pending), self.mws_cap]
        for i in range(2):
            CT, nk16, ln, act = probs[i] if i < len(probs) else (0, 0, False, False)
            vals += [CT, nk16, int(ln), int(act), 1]
        out = (ctypes.c_long * (len(MID_FIELDS) + 2 * len(MID_PROB_FIELDS)))()
        self.lib.mid_route_c((ctypes.c_long * len(vals))(*vals), self.ctx(), self.knob, out)
        m = dict(zip(MID_FIELDS, out[:len(MID_FIELDS)]))
        k = len(MID_PROB_FIELDS)
        m["pr"] = [dict(zip(MID_PROB_FIELDS, out[len(MID_FIELDS) + k * i:len(MID_FIELDS) + k * (i + 1)])) for i in range(len(probs))]
        for p in m["pr"]:
            if p["reset"]:
                self.arrive_off, self.pending = 0, False
            self.arrive_off += p["arrive"]
        return m


def route_name(r):
    """The kernel a per-layer route launches, as a kernel trace names it, with (grid, workgroup size)."""
    if r["w"]:
        return f"g_gemm_w<{r['epi']}, {int(r['parts'] > 1)}>", r["grid"], 512
    return f"g_gemm_s<{r['nct']}, {r['rt']}, {r['sd']}, {r['epi']}, 0>", r["grid"], 256


def plan_launches(lib, cfg, E, ksplit=2):
    """The GEMM launches of one plan's policy-prior pass and CEM iteration 0, in the host's issue order: [(label, kind, route)] with
    kind "gemm" (a per-layer route, LR_* in route["want"]) or "mid" (a few-row g_gemm_m + m_rows route).  Labels name the layer:
    <net>.l<layer> (pi, dyn, rew, q0, q1, term; "pi_rows." for the policy-prior rows), with "@t0" for the first layers at t = 0."""
    h = Handle(lib, cfg, E, ksplit)
    L, M, A, N, P, H = cfg.latent_dim, cfg.mlp_dim, cfg.action_dim, cfg.num_samples, cfg.num_pi_trajs, cfg.horizon
    kb_in, kb_z, kb_m = h.Kin // 16, _ru(L, 32) // 16, M // 16   # first layers that take the action / only the latent; the rest
    kb_short = (h.Kin - L) // 16                                # t = 0: the action columns (lay_cvec has the z0 products)
    ct_m, ct_l = (M + 31) // 32, (L + 31) // 32
    ct_bins, ct_pi = (max(cfg.num_bins, 1) + 31) // 32, (2 * A + 31) // 32
    out = []

    def gemm(label, rows_p, rpe, CT, nk, want):
        r = h.gemm(rows_p, rpe, CT, nk, want)
        r["want"] = want
        out.append((label, "gemm", r))

    def mid(label, rows, rows_p, rpe, probs, one_by_one=False):
        out.append((label, "mid", h.mid(rows, rows_p, rpe, probs, one_by_one)))

    # lay_cvec: the z0 products of the reward / dynamics first layers, one row per plan
    for net in ("rew", "dyn"):
        gemm(f"{net}.cvec", _ru(E, 128), 1, ct_m, L // 16, LR_PLAIN)
    rows_p = _ru(E * N, 128)
    pifold = P > 0 and E == 1 and h.mid_ok(rows_p)
    if P > 0 and not pifold:  # lay_pitraj
        rows, prp = E * h.Ppad, _ru(E * h.Ppad, 128)
        h.arrive_off, h.pending = 0, False
        for t in range(H):
            if h.mid_ok(prp):
                mid("pi_rows.l0", rows, prp, h.Ppad, [(ct_m, kb_z, True, False)])
                mid("pi_rows.l1", rows, prp, h.Ppad, [(ct_m, kb_m, True, False)])
                mid("pi_rows.l2", rows, prp, h.Ppad, [(ct_pi, kb_m, False, False)])
                if t < H - 1:
                    mid("pi_rows.dyn.l0", rows, prp, h.Ppad, [(ct_m, kb_in, True, False)])
                    mid("pi_rows.dyn.l1", rows, prp, h.Ppad, [(ct_m, kb_m, True, False)])
                    mid("pi_rows.dyn.l2", rows, prp, h.Ppad, [(ct_l, kb_m, True, False)])
            else:
                gemm("pi_rows.l0", prp, h.Ppad, ct_m, kb_z, LR_MISH)
                gemm("pi_rows.l1", prp, h.Ppad, ct_m, kb_m, LR_MISH)
                gemm("pi_rows.l2", prp, h.Ppad, ct_pi, kb_m, LR_PLAIN)
                if t < H - 1:
                    gemm("pi_rows.dyn.l0", prp, h.Ppad, ct_m, kb_in, LR_MISH)
                    gemm("pi_rows.dyn.l1", prp, h.Ppad, ct_m, kb_m, LR_MISH)
                    gemm("pi_rows.dyn.l2", prp, h.Ppad, ct_l, kb_m, LR_SIMNORM)
    # CEM iteration 0: l_sample has zeroed the counters
    rows = E * N
    h.arrive_off = 0
    if h.mid_ok(rows_p):  # lay_estimate_value_m
        h.pending = True
        for t in range(H):
            k0 = kb_short if t == 0 else kb_in
            if pifold:
                prp = _ru(P, 128)
                mid("pi_rows.l0", P, prp, h.Ppad, [(ct_m, kb_z, True, False)])
                mid("pi_rows.l1", P, prp, h.Ppad, [(ct_m, kb_m, True, False)])
                mid("pi_rows.l2", P, prp, h.Ppad, [(ct_pi, kb_m, False, False)])
            mid(f"dyn|rew.l0{'@t0' if t == 0 else ''}", rows, rows_p, N, [(ct_m, k0, True, False)] * 2)
            mid("dyn|rew.l1", rows, rows_p, N, [(ct_m, kb_m, True, False)] * 2)
            mid("dyn.l2|rew.l2", rows, rows_p, N, [(ct_l, kb_m, True, t + 1 < H), (ct_bins, kb_m, False, False)])
            if cfg.episodic:
                mid("term.l0", rows, rows_p, N, [(ct_m, kb_z, True, False)])
                mid("term.l1", rows, rows_p, N, [(ct_m, kb_m, True, False)])
                mid("term.l2", rows, rows_p, N, [(1, kb_m, False, False)])
        mid("pi.l0", rows, rows_p, N, [(ct_m, kb_z, True, False)])
        mid("pi.l1", rows, rows_p, N, [(ct_m, kb_m, True, False)])
        mid("pi.l2", rows, rows_p, N, [(ct_pi, kb_m, False, False)])
        mid("q0|q1.l0", rows, rows_p, N, [(ct_m, kb_in, True, False)] * 2)
        mid("q0|q1.l1", rows, rows_p, N, [(ct_m, kb_m, True, False)] * 2)
        mid("q0|q1.l2", rows, rows_p, N, [(ct_bins, kb_m, False, False)] * 2, one_by_one=True)
        return out
    for t in range(H):  # lay_estimate_value: the reward chain beside the dynamics chain
        k0, t0 = (kb_short, "@t0") if t == 0 else (kb_in, "")
        gemm(f"rew.l0{t0}", rows_p, N, ct_m, k0, LR_MISH)
        gemm("rew.l1", rows_p, N, ct_m, kb_m, LR_MISH)
        gemm("rew.l2", rows_p, N, ct_bins, kb_m, LR_TWOHOT)
        gemm(f"dyn.l0{t0}", rows_p, N, ct_m, k0, LR_MISH)
        gemm("dyn.l1", rows_p, N, ct_m, kb_m, LR_MISH)
        gemm("dyn.l2", rows_p, N, ct_l, kb_m, LR_SIMNORM)
        if cfg.episodic:
            gemm("term.l0", rows_p, N, ct_m, kb_z, LR_MISH)
            gemm("term.l1", rows_p, N, ct_m, kb_m, LR_MISH)
            gemm("term.l2", rows_p, N, 1, kb_m, LR_PLAIN)
    gemm("pi.l0", rows_p, N, ct_m, kb_z, LR_MISH)
    gemm("pi.l1", rows_p, N, ct_m, kb_m, LR_MISH)
    gemm("pi.l2", rows_p, N, ct_pi, kb_m, LR_PLAIN)
    for j in range(2):
        gemm(f"q{j}.l0", rows_p, N, ct_m, kb_in, LR_MISH)
        gemm(f"q{j}.l1", rows_p, N, ct_m, kb_m, LR_MISH)
        gemm(f"q{j}.l2", rows_p, N, ct_bins, kb_m, LR_TWOHOT if j == 0 else LR_PLAIN)
    return out


def kernel_list(launches):
    """[(label, kernel, grid, workgroup)] of the GEMM-side kernels the launches issue (g_gemm_m's m_rows included), grids in workgroups."""
    res = []
    for label, kind, r in launches:
        if kind == "gemm":
            res.append((label, *route_name(r)))
        else:
            res.append((label, "g_gemm_m", r["gblk"], 512))
            if r["nrow"]:
                res.append((label, f"m_rows<{r['mr_threads']}>", r["rblk"], r["mr_threads"]))
    return res
