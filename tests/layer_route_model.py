"""The layered family's GEMM launches of one plan, as the host issues them -- every route from tdmpc2_amd/csrc/layer_route.h itself
(compiled with g++ behind the C shim below), the handle's capacities from tdmpc2_amd/csrc/plan_layout.h itself (the same shim), the
sequence from layered_host.cuh.

Used by tests/test_layer_route.py (the route table of the benched geometries) and tests/test_tile_order.py (the dispatcher model of
the launches whose workgroups wait for each other)."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROUTE_SHIM = r"""
#include <cstring>

#include "layer_route.h"
#include "plan_layout.h"
using namespace tdk;
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
// env: one_stream, fuse_ln, ksplit, fewrow, cluster.  Returns the refusal's code (msg: its text), or 0 and the layout: sc (LAYOUT_FIELDS), then
// per buffer its id, name, bytes and whether it starts zeroed
extern "C" int plan_layout_c(const tdmpc2_plan_cfg *cfg, int num_cus, const int *env, char *msg, long *sc, int *ids, const char **names,
                             long *bytes, int *zero) {
    CreateEnv e;
    e.one_stream = env[0] != 0; e.fuse_ln = env[1] != 0; e.ksplit = env[2]; e.fewrow = env[3] != 0; e.cluster = env[4];
    const PlanLayout lo = plan_layout(*cfg, num_cus, e);
    strcpy(msg, lo.msg);
    if (lo.err) return lo.err;
    const long v[] = {lo.path, lo.precision, lo.layered, lo.split, lo.second_chain, lo.err_line, lo.Apad, lo.tiles, lo.nnets, lo.stride,
                      (long)lo.row_bytes, (long)lo.lds_bytes, (long)lo.cl_lds, lo.cl_max_clusters, lo.Kin, lo.Mp, lo.ldl, lo.Ppad, lo.ldpre,
                      (long)lo.cvec_rows, (long)lo.stats_cap, (long)lo.arrive_cap, (long)lo.ks_tiles, (long)lo.mws_cap, plan_maxct(*cfg), lo.nbuf};
    for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) sc[i] = v[i];
    for (int i = 0; i < lo.nbuf; ++i) { ids[i] = lo.buf[i].id; names[i] = lo.buf[i].name; bytes[i] = (long)lo.buf[i].bytes; zero[i] = lo.buf[i].zero; }
    return 0;
}
extern "C" long ksws_slots_c(long ks_tiles, int num_cus, int mode) { return (long)ksws_slots((size_t)ks_tiles, num_cus, mode); }
extern "C" long ks_slot_bytes() { return (long)(KS_SLOT_FLOATS * 4); }
extern "C" int pb_count() { return PB_COUNT; }
extern "C" int knob_count() { return LK_COUNT; }
extern "C" void knob_spec(int i, int *out) { out[0] = LAY_KNOBS[i].def; out[1] = LAY_KNOBS[i].lo; out[2] = LAY_KNOBS[i].hi; }
"""

ROUTE_FIELDS = ("w", "nct", "rt", "sd", "epi", "nrowblk", "ncolblk", "xcd_rows", "ncol_grid", "ord_nblk", "parts", "full", "max_tail",
                "per_xcd", "wo_nblk", "grid", "arrive", "ln_after")
LAYOUT_FIELDS = ("path", "precision", "layered", "split", "second_chain", "err_line", "Apad", "tiles", "nnets", "stride", "row_bytes",
                 "lds_bytes", "cl_lds", "cl_max_clusters", "Kin", "Mp", "ldl", "Ppad", "ldpre", "cvec_rows", "stats_cap", "arrive_cap",
                 "ks_tiles", "mws_cap", "maxct", "nbuf")
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
    lib.plan_layout_c.argtypes = [ctypes.c_void_p, ci, pi, ctypes.c_char_p, pl, pi, ctypes.POINTER(ctypes.c_char_p), pl, pi]
    lib.ksws_slots_c.argtypes = [cl, ci, ci]
    lib.ksws_slots_c.restype = lib.ks_slot_bytes.restype = cl
    return lib


class Refused(Exception):
    """plan_layout's refusal: args = (code, message)"""


def plan_layout(lib, plan_cfg, num_cus=CUS, one_stream=False, fuse_ln=True, ksplit=2, fewrow=True, cluster=2):
    """plan_layout (tdmpc2_amd/csrc/plan_layout.h) of a struct tdmpc2_plan_cfg (tdmpc2_amd.native.PlanCfg): the scalars by name
    (LAYOUT_FIELDS) and "bufs": {name: (bytes, starts zeroed)}; Refused(code, message) where create refuses the configuration."""
    n = lib.pb_count()
    env = (ctypes.c_int * 5)(int(one_stream), int(fuse_ln), ksplit, int(fewrow), cluster)
    msg = ctypes.create_string_buffer(512)
    sc, ids, names = (ctypes.c_long * len(LAYOUT_FIELDS))(), (ctypes.c_int * n)(), (ctypes.c_char_p * n)()
    nbytes, zero = (ctypes.c_long * n)(), (ctypes.c_int * n)()
    rc = lib.plan_layout_c(ctypes.byref(plan_cfg), num_cus, env, msg, sc, ids, names, nbytes, zero)
    if rc:
        raise Refused(rc, msg.value.decode())
    lo = dict(zip(LAYOUT_FIELDS, sc))
    lo["bufs"] = {names[i].decode(): (nbytes[i], bool(zero[i])) for i in range(lo["nbuf"])}
    assert len(lo["bufs"]) == lo["nbuf"] == len(set(ids[:lo["nbuf"]]))  # every entry its own name and handle field
    return lo


def layout_bytes(lib, lo, num_cus=CUS, ksplit=2):
    """Device bytes of a handle with this layout whose K-split mode is (or has been raised to) `ksplit`: the table plus the K-split
    workspaces, one per chain (ksws_ensure)."""
    slots = lib.ksws_slots_c(lo["ks_tiles"], num_cus, ksplit)
    return sum(b for b, _ in lo["bufs"].values()) + slots * lib.ks_slot_bytes() * (2 if lo["second_chain"] else 1)


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
    """What a layered, split-arithmetic handle created for E plans of `cfg` holds (plan_layout.h: plan_layout, ksws_slots), with the
    K-split mode set to `ksplit` after creation (tdmpc2_plan_set_tuning) and the arrival counters of the stage it is in."""

    def __init__(self, lib, cfg, E, ksplit=2, cus=CUS):
        self.lib, self.cfg, self.E, self.ksplit, self.cus = lib, cfg, E, ksplit, cus
        from tdmpc2_amd import native

        lo = plan_layout(lib, native.plan_cfg(cfg, cfg.iterations, E), cus)  # created with the default switches (K-split mode 2)
        assert lo["layered"] and lo["split"] and lo["second_chain"]
        for k in ("Kin", "Mp", "Ppad", "maxct", "stats_cap", "arrive_cap", "mws_cap"):
            setattr(self, k, lo[k])
        # grown (never shrunk) by the mode set afterwards
        self.ksws_slots = max(lib.ksws_slots_c(lo["ks_tiles"], cus, 2), lib.ksws_slots_c(lo["ks_tiles"], cus, ksplit))
        self.mws = "mws[0]" in lo["bufs"]
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
