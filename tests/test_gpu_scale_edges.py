"""-m gpu: the split arithmetic's per-record scales on every route.  The suite's fixtures give every net, ensemble member and hidden
layer the same record (kw 17, ka 5), so a kernel that reads a neighbour's record returns the same bits on all of them.  Here
a. export_packed() of handles filled by the per-layer binds and by tdmpc2_plan_refresh_weights equals the numpy restatement of the
   packer (tests/scale_common.py) byte for byte, segment by segment, on the weight sets of refresh_common.packed_inputs and on the
   staggered sets (`nonfinite`: NaN positions, not payloads); a difference names owner, member, layer, kind and element;
b. every entry point runs on a STAGGERED checkpoint (scale_common.stagger: every record differs from its neighbours;
   tests/test_scale_edges.py shows that one slipped exponent moves the fp64 oracle by at least 10 gates at these very inputs) against
   the fp64 oracle on the same weights, under the gate the entry point's whole-chain test already uses (scale_common, "entry
   points").  Fused family (c1, mt5, c1_ep at 128 samples): 64-row and forced 32-row workgroups, refit separate and folded, cluster
   off, one cluster per tile, two clusters per tile; the route each setting takes is asserted from fused_route.h
   (tests/fused_route_model.py).  Layered family (small, small_ep, small_mt): few-row path on and off, LayerNorm fused and as a row
   kernel, and one chain instead of two (plan and estimate_value); the kernels of each of the four settings are asserted from layer_route.h (tests/layer_route_model.py with the two knobs
   passed in).  That model describes plan() and estimate_value; td_target, policy_value, policy_loss and the model calls do not
   take the few-row path, so they run with LayerNorm fused and not, once each.  Two wider layered shapes reach the kernels the
   1M-class ones do not: latent 512 / mlp 256, 12 plans of 1024 samples with the K-split mode 1 takes g_gemm_w<1, 1> and
   g_gemm_w<2, 1> (the K-split tail), latent 64 / mlp 768, 16 plans of 1024 samples takes g_gemm_w<1, 0> -- the smallest shapes of
   a search over the route model -- both asserted, both through estimate_value with the head pairs going round over the plans.
TDMPC2_SCALE_EDGES_JSON=<file>: the worst err / gate per entry point, route and handle (profiles/scale_edges.json).

What bites, from scratch builds of the library, each run once on the MI355X against this file (125 tests when they ran) and against
tests/test_gpu_value_edges.py + tests/test_gpu_model_edges.py + tests/test_gpu_policy_loss.py (their 48M / 317M cases left out, 213
tests).  Every build reads inside the scale table; none is committed.
1. `asc_sel_stride = 0` in lay_ln_epi (layered_host.cuh; every head takes head 0's ascale): 42 tests fail here -- estimate_value
   and plan on three of the four layered routes, td_target / policy_value and policy_loss on all four, on small, small_ep and
   small_mt.  The older files PASS (213 of 213): ka is 5 on every head of their checkpoints.
2. `osc_sel_stride = 0` in the per-layer GEMM's parameters (layered_host.cuh; every head takes head 0's oscale): 36 tests fail here,
   the same entry points on the layered handles.  The older files fail 9 (the whole chain on four layered handles, policy_loss
   parity on four, one Python-boundary test): the last layers' kw of the fixtures differs by one between some heads.
3. ACT_SCALE for the record's ascale in the fused NormedLinear epilogue (fused_kernels.cuh; built for the 16-column action padding,
   so the older files ran without their c2 cases, 197 tests): 36 tests fail here -- every entry point on every route of c1, mt5 and
   c1_ep.  The older files PASS (197 of 197).
4. `N.scal[l]` for `N.scal[hd * 3 + l]` in k_rf_pack (refresh_kernels.cuh; every head packed with head 0's wscale): 99 tests fail
   here -- the byte comparison on the three split rows, and every entry point on every handle and route.  The older files fail 17
   (the whole chain on seven handles, policy_loss parity on seven, three Python-boundary tests), again through the last layers' kw."""
import json
import os

import numpy as np
import pytest
import torch

from tests import refresh_common as rc
from tests import scale_common as sc
from tests.gpu_common import dev, disc_pow

pytestmark = pytest.mark.gpu

FUSED_ROUTES = {   # id: (tuning, plans per plan() call, expected route of plan(): kind, folded refit, 32-row workgroups per tile)
    "rows64-fold0-cluster0": (dict(rows=64, fold=0, cluster=0), None, ("TILE", 0, 2)),
    "rows32-fold1-cluster0": (dict(rows=32, fold=1, cluster=0), None, ("TILE", 1, 1)),
    "cluster1": (dict(cluster=1), 1, ("CLUSTER", 1, 1)),
    "cluster2": (dict(cluster=2), 1, ("CLUSTER2", 1, 1)),   # (episodic models: one cluster per tile)
}
LAYERED_ROUTES = {"fewrow1-fuseln1": dict(fewrow=1, fuse_ln=1), "fewrow0-fuseln1": dict(fewrow=0, fuse_ln=1),
                  "fewrow1-fuseln0": dict(fewrow=1, fuse_ln=0), "fewrow0-fuseln0": dict(fewrow=0, fuse_ln=0),
                  "one-stream": dict(one_stream=1)}   # TDMPC2_ONE_STREAM at creation: one chain, the reward nets after the dynamics nets
RUNS = [(n, r) for n in sc.FUSED for r in FUSED_ROUTES] + [(n, r) for n in sc.LAYERED for r in LAYERED_ROUTES]
PER_TILE = [(n, r) for n, r in RUNS if not r.startswith("cluster")]   # estimate_value: no cluster route
CALLS = [(n, r) for n, r in PER_TILE if not r.startswith("fewrow0") and r != "one-stream"]    # the other calls: no few-row path either
LAYERED_KERNELS = {   # the GEMM-side kernels of a plan of small / small_ep / small_mt under each setting (layer_route.h)
    "fewrow1-fuseln1": {"g_gemm_m", "m_rows<256>", "g_gemm_s<1, 1, 4, 0, 0>"},
    "fewrow1-fuseln0": {"g_gemm_m", "m_rows<256>", "g_gemm_s<1, 1, 4, 0, 0>"},   # (the few-row path keeps its launches)
    "fewrow0-fuseln1": {"g_gemm_s<1, 1, 4, 0, 0>", "g_gemm_s<1, 1, 4, 1, 0>", "g_gemm_s<1, 1, 4, 2, 0>"},   # Mish / SimNorm epilogues
    "fewrow0-fuseln0": {"g_gemm_s<1, 1, 4, 0, 0>"},   # plain epilogues, LayerNorm in the row kernel
}
WIDE = {   # id: (overrides of "small", plans, K-split mode, kernels that must be among the plan's)
    "ksplit-tail": (dict(mlp_dim=256, latent_dim=512, num_samples=1024), 12, 1, {"g_gemm_w<1, 1>", "g_gemm_w<2, 1>"}),
    "wide": (dict(mlp_dim=768, latent_dim=64, num_samples=1024), 16, 1, {"g_gemm_w<1, 0>"}),
}
_scen, _runs, _worst, _libs = {}, {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _dump_worst():
    yield
    path = os.environ.get("TDMPC2_SCALE_EDGES_JSON")
    if path:
        with open(path, "w") as f:
            json.dump({"gates": "tests/scale_common.py, entry points", "worst_err_over_gate": [dict(entry=k[0], handle=k[1], route=k[2], worst=v)
                                                                                              for k, v in sorted(_worst.items())]}, f, indent=1)
            f.write("\n")


def scenario(name):
    if name not in _scen:
        _scen[name] = sc.Scenario(name)
    return _scen[name]


def d(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev())


class Run:
    """One split-arithmetic handle of a scenario with a route's tuning applied and the staggered checkpoint bound."""

    def __init__(self, name, route):
        from tdmpc2_amd.native import NativePlanner

        self.s = s = scenario(name)
        self.name, self.route, self.cfg = name, route, s.cfg
        self.max_envs = max(s.E, 2)
        self.tune = (FUSED_ROUTES[route][0] if s.path == 1 else LAYERED_ROUTES[route])
        if self.tune.get("one_stream"):
            os.environ["TDMPC2_ONE_STREAM"] = "1"   # read when the handle is created
        try:
            self.p = p = NativePlanner(s.cfg, s.I, dev(), max_envs=self.max_envs, path=s.path, precision=2)
        finally:
            os.environ.pop("TDMPC2_ONE_STREAM", None)
        assert p.path == s.path and p.precision == 2
        for k, fn in (("rows", p.set_rows_per_workgroup), ("fold", p.set_fold_refit), ("cluster", p.set_cluster), ("fewrow", p.set_fewrow),
                      ("fuse_ln", p.set_fuse_ln)):
            if k in self.tune:
                fn(self.tune[k])
        self.tsd = {k: torch.as_tensor(v) for k, v in s.sd.items()}
        p.bind_state_dict(self.tsd)
        self.kw_rows = {}
        if s.cfg.multitask:
            emb = self.tsd["_task_emb.weight"].to(torch.float32)
            norm = emb.norm(2, dim=-1, keepdim=True)
            emb = torch.where(norm > 1.0, emb * (1.0 / (norm + 1e-7)), emb)   # nn.Embedding(max_norm=1)
            self.emb = emb
            self.kw_rows = dict(task_emb_table=emb.to(dev()).contiguous(), act_mask_table=self.tsd["_action_masks"].to(torch.float32).to(dev()).contiguous())

    def plan_args(self, envs):
        """z0, disc_pow, task_emb, act_mask of the plans `envs` (device)."""
        s, c = self.s, self.s.c
        e = list(envs)
        emb = mask = None
        if s.cfg.multitask:
            t = torch.tensor([c["tasks"][i] for i in e])
            emb, mask = self.emb[t].to(dev()).contiguous(), self.tsd["_action_masks"][t].to(torch.float32).to(dev()).contiguous()
        return d(c["z0"][e]), disc_pow(s.cfg, [c["discounts"][i] for i in e]).to(dev()), dict(task_emb=emb, act_mask=mask)

    def done(self, *outs):
        torch.cuda.synchronize()
        assert self.p.take_fault() == 0, (self.name, self.route)
        for o in outs:
            assert torch.isfinite(o).all(), (self.name, self.route)


def _run(name, route):
    if (name, route) not in _runs:
        _runs[(name, route)] = Run(name, route)
    return _runs[(name, route)]


def _gated(entry, r, got, expect):
    """Every key of `expect` ({key: (v64, gate)}) against `got` ({key: numpy}); records and returns the worst err / gate."""
    worst, where = 0.0, None
    for k, (v64, gate) in expect.items():
        with np.errstate(all="ignore"):
            ratio = np.abs(np.asarray(got[k], np.float64).reshape(np.shape(v64)) - v64) / gate
        w = float(np.max(np.where(np.isnan(ratio), np.inf, ratio)))
        if w >= worst:
            worst, where = w, k
    key = (entry, r.name, r.route)
    _worst[key] = max(_worst.get(key, 0.0), worst if np.isfinite(worst) else 1e30)
    print(f"[{r.name} {r.route}] {entry}: worst err / gate {worst:.3f} ({where})")
    assert worst <= 1, (r.name, r.route, entry, where, worst)


# ---------------------------------------------------------------- a. bytes
def _compare(pl, sd, cfg, path, split, label, way):
    want = sc.restated_segments({k: v.detach().cpu().numpy() for k, v in sd.items()}, cfg, path, split)
    got = rc.blob_segments(pl.export_packed(), cfg, split)
    diff = (sc.first_difference_nan if label == "nonfinite" else sc.first_difference)(want, got)
    assert diff is None, f"{label}, {way}: {diff}"


@pytest.mark.parametrize("name,path,prec", rc.CASES, ids=rc.IDS)
def test_packed_bytes_equal_the_restatement(name, path, prec):
    from oracle import cases
    from tdmpc2_amd.native import NativePlanner

    c = cases.build_case(name)
    cfg, split = c["cfg"], prec == 2
    A, B = (NativePlanner(cfg, c["iterations"], dev(), max_envs=2, path=path, precision=prec) for _ in range(2))
    sets = list(rc.packed_inputs(c, dev()))
    s = scenario(name)
    sets.append(("staggered", rc.device_sd({"sd": s.sd}, dev())))
    assert sc.stagger_violations(sc.records(s.sd, cfg), cfg) == []
    for label, sd in sets:
        A.bind_state_dict(sd)   # the per-layer binds
        A.bind_encoder(sd)
        B.refresh_state_dict(sd)   # tdmpc2_plan_refresh_weights
        for way, pl in (("binds", A), ("refresh", B)):
            _compare(pl, sd, cfg, path, split, label, way)
            assert pl.take_fault() == 0
    A.close()
    B.close()


# ---------------------------------------------------------------- b. every entry point on a staggered checkpoint
def _route_libs(tmp_path_factory):
    if not _libs:
        from tests import fused_route_model as frm
        from tests import layer_route_model as lrm

        tmp = tmp_path_factory.mktemp("route_shims")
        _libs.update(frm=frm.build(tmp), lrm=lrm.build(tmp))
    return _libs


def _layered_kernels(lib, cfg, E, fewrow=1, fuse_ln=1, ksplit=2):
    """Kernel names of a plan from the layered route model with the handle's few-row and fused-LayerNorm knobs passed in."""
    import ctypes

    from tests import layer_route_model as lrm

    class Knobs(lrm.Handle):
        def ctx(self):
            c = list(super().ctx())
            c[2] = int(fuse_ln)   # LayCtx::fuse_ln
            return (ctypes.c_long * 11)(*c)

        def mid_ok(self, rows_p):
            return bool(self.lib.mid_ok_c(1, int(fewrow), self.ksplit, int(self.mws), 1, 0, self.cus, self.maxct, rows_p))

    keep = lrm.Handle
    lrm.Handle = Knobs
    try:
        return {k[1] for k in lrm.kernel_list(lrm.plan_launches(lib, cfg, E, ksplit))}
    finally:
        lrm.Handle = keep


@pytest.mark.parametrize("name,route", RUNS)
def test_the_route_is_the_one_named(name, route, tmp_path_factory):
    """Coverage shown, not assumed: the route models, compiled from the library's own route headers, on this handle's shape."""
    from tdmpc2_amd import native
    from tests import fused_route_model as frm
    from tests import layer_route_model as lrm

    s, libs = scenario(name), _route_libs(tmp_path_factory)
    if s.path == 1:
        tune, E1, (kind, fold, nst) = FUSED_ROUTES[route]
        if route == "cluster2" and s.cfg.episodic:
            kind = "CLUSTER"
        E = s.E if E1 is None else E1
        pc = native.plan_cfg(s.cfg, s.I, max(s.E, 2), path=1, precision=2)
        r = frm.route(libs["frm"], pc, E, **tune)
        assert (r["kind"], r["fold"], r["nst"]) == (getattr(frm, kind), fold, nst), r
        assert r["tiles"] == s.cfg.num_samples // (32 * nst)
        v = frm.route(libs["frm"], pc, E, entry=frm.VALUE, **tune)
        assert (v["kind"], v["nst"]) == (frm.TILE, nst)   # estimate_value: per-tile workgroups of the same height
    elif route == "one-stream":   # the second chain's buffers are what the switch takes away (plan_layout.h)
        pc = native.plan_cfg(s.cfg, s.I, max(s.E, 2), path=2, precision=2)
        assert lrm.plan_layout(libs["lrm"], pc)["second_chain"] == 1 and lrm.plan_layout(libs["lrm"], pc, one_stream=True)["second_chain"] == 0
    else:
        tune = LAYERED_ROUTES[route]
        assert _layered_kernels(libs["lrm"], s.cfg, s.E, **tune) == LAYERED_KERNELS[route]


@pytest.mark.parametrize("name,route", PER_TILE)
def test_estimate_value_on_a_staggered_checkpoint(name, route):
    r = _run(name, route)
    s = r.s
    z0, dp, kw = r.plan_args(range(s.E))
    got = r.p.estimate_value(z0, dp, d(s.v_actions), d(s.v_eps), d(s.v_qidx), **kw)
    r.done(got)
    assert sorted({int(h) for h in s.v_qidx.ravel()}) == list(range(s.cfg.num_q))   # between them the pairs use every head
    _gated("estimate_value", r, {"value": got.cpu().numpy()}, s.expect("estimate_value"))


@pytest.mark.parametrize("name,route", RUNS)
def test_plan_on_a_staggered_checkpoint(name, route):
    """plan() with the tape given and the stages kept: the values of EVERY iteration against the oracle's estimate_value on the
    actions that iteration sampled (the library's own, from the stage buffer) with the tape's noise and head pair."""
    r = _run(name, route)
    s, c = r.s, r.s.c
    per_call = FUSED_ROUTES[route][1] if s.path == 1 else None
    groups = [list(range(min(s.E, 2)))] if per_call is None else [[e] for e in range(s.E)]
    for envs in groups:
        z0, dp, kw = r.plan_args(envs)
        tape = {k: d(v[envs]) for k, v in c["tape"].items()}
        action, st = r.p.plan(z0, dp, d(c["prev_mean"][envs]).clone(), d(c["t0"][envs].astype(np.uint8)), tape=tape, debug=True, **kw)
        r.done(action, st["value"], st["actions"])
        acts, val = st["actions"].cpu().numpy(), st["value"].cpu().numpy()   # [E, I, H, N, A], [E, I, N]
        tp = c["tape"]
        v = {}
        for dt in (torch.float64, torch.float32):
            v[dt] = np.stack([s.value_of(s.sd, dt, acts[:, it], tp["pi_eps"][envs, it], tp["qidx"][envs, it], envs) for it in range(s.I)], 1)
        _gated("plan", r, {"value": val}, sc.Scenario.value_fields(v[torch.float64], v[torch.float32])[0])


@pytest.mark.parametrize("name,route", CALLS)
def test_td_target_and_policy_value_on_a_staggered_checkpoint(name, route):
    r = _run(name, route)
    s, cfg = r.s, r.s.cfg
    z, eps, rew, term = d(s.ch_z), d(s.ch_eps), d(s.ch_rew), d(s.ch_term)
    kw = dict(r.kw_rows, task_ids=d(s.ch_tasks.astype(np.int32))) if cfg.multitask else {}
    disc = d(s.disc_np) if cfg.multitask else s.discount
    td, pv = {}, {}
    for pair in s.ch_pairs:
        qi = torch.tensor(pair, dtype=torch.int32, device=dev())
        out = r.p.td_target(z, rew, term, disc, pi_eps=eps, qidx=qi, **kw)
        r.done(out)
        td[("td", pair)] = out.cpu().numpy()
        for target in (False, True):
            for red in ("min", "avg"):
                a, q = r.p.policy_value(z, use_target=target, reduce=red, pi_eps=eps, qidx=qi, **kw)
                r.done(a, q)
                pv[("q", target, red, pair)] = q.cpu().numpy()
        pv[("action",)] = a.cpu().numpy()
    _gated("td_target", r, td, s.expect("td_target"))
    _gated("policy_value", r, pv, s.expect("policy_value"))


@pytest.mark.parametrize("name,route", CALLS)
def test_policy_loss_on_a_staggered_checkpoint(name, route):
    r = _run(name, route)
    s, cfg = r.s, r.s.cfg
    T, B = sc.CHAIN_T, sc.CHAIN_B
    kw = dict(r.kw_rows, task_ids=d(s.ch_tasks_b.astype(np.int32))) if cfg.multitask else {}
    scale = torch.full((1,), 1.0, device=dev())
    res = r.p.policy_loss(d(s.ch_z.reshape(T, B, -1)), scale, rho=cfg.rho, entropy_coef=cfg.entropy_coef, tau=cfg.tau, update_scale=True,
                          pi_eps=d(s.ch_eps.reshape(T, B, -1)), qidx=torch.tensor(s.pl_qidx, dtype=torch.int32, device=dev()), want=("action", "q"), **kw)
    r.done(res["action"], res["q"], res["loss"])
    _gated("policy_loss", r, {"q": res["q"].cpu().numpy().reshape(-1), "action": res["action"].cpu().numpy().reshape(T * B, -1)}, s.expect("policy_loss"))


@pytest.mark.parametrize("name,route", CALLS)
def test_model_rollout_and_losses_on_a_staggered_checkpoint(name, route):
    r = _run(name, route)
    s, cfg = r.s, r.s.cfg
    kw = dict(r.kw_rows, task_ids=d(s.m_tasks.astype(np.int32))) if cfg.multitask else {}
    fields = ("zs", "reward_logits", "q_logits") + (("term_logit",) if cfg.episodic else ())
    z0, act = d(s.m_z0), d(s.m_act)
    take = lambda res: {k: (v.cpu().numpy()[..., 0] if k == "term_logit" else v.cpu().numpy()) for k, v in res.items()}
    on = r.p.model_rollout(z0, act, use_target=False, want=fields, **kw)
    tg = r.p.model_rollout(z0, act, use_target=True, want=("q_logits",), **kw)
    r.done(*on.values(), *tg.values())
    got = take(on)
    got["tq_logits"] = tg["q_logits"].cpu().numpy()
    _gated("model_rollout", r, got, s.expect("model_rollout"))
    res = r.p.model_losses(z0, act, d(s.m_next), d(s.m_rew), d(s.m_td), d(s.m_term) if cfg.episodic else None, rho=cfg.rho,
                           coefs=(20.0, 0.1, 0.1, 1.0), want=fields, step_means=True, **kw)
    r.done(*res.values())
    _gated("model_losses", r, take(res), s.expect("model_losses"))


# ---------------------------------------------------------------- the wide GEMM and its K-split tail
@pytest.mark.parametrize("wid", sorted(WIDE))
def test_estimate_value_on_the_wide_routes(wid, tmp_path_factory):
    """A staggered checkpoint of a shape the route model sends to g_gemm_w (and, K-split mode 1, to its K-split tail): the heads a plan
    reads are chosen by its qidx, so twelve / sixteen plans with the pairs going round read every head's record in one launch."""
    from tdmpc2_amd.native import NativePlanner

    over, E, ksplit, must = WIDE[wid]
    key = ("wide", wid)
    if key not in _scen:
        _scen[key] = sc.Scenario(wid, custom=("small", over, E))
    s = _scen[key]
    assert sc.stagger_violations(sc.records(s.sd, s.cfg), s.cfg) == []
    kernels = _layered_kernels(_route_libs(tmp_path_factory)["lrm"], s.cfg, E, ksplit=ksplit)
    assert must <= kernels, kernels
    p = NativePlanner(s.cfg, s.I, dev(), max_envs=E, path=2, precision=2)
    p.set_ksplit(ksplit)
    p.bind_state_dict({k: torch.as_tensor(v) for k, v in s.sd.items()})
    got = p.estimate_value(d(s.c["z0"]), disc_pow(s.cfg, s.c["discounts"]).to(dev()), d(s.v_actions), d(s.v_eps), d(s.v_qidx))
    torch.cuda.synchronize()
    assert p.take_fault() == 0 and torch.isfinite(got).all()
    assert sorted({int(h) for h in s.v_qidx.ravel()}) == list(range(s.cfg.num_q))

    class R:
        name, route = wid, f"ksplit{ksplit}"

    _gated("estimate_value", R, {"value": got.cpu().numpy()}, s.expect("estimate_value"))
    p.close()
