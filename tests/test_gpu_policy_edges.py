"""-m gpu: the policy prior (tdmpc2_plan_bind_policy / tdmpc2_plan_pi: k_pol_row, k_pol_gemv, k_enc_norm, k_pol_head, launch_pi)
against an fp64 reference at its shape, value and route edges (tests/policy_edges_common.py; tests/test_policy_edges.py checks the
reference, the probes, the route edges and the order emulation on the CPU).

Gate, per case and output: max|HIP - ref64| <= 4 max(max|ref32 - ref64|, 2^-23 max(1, max|ref64|)); head_band per value, in
policy_common.entropy_bound's form.  Every call goes through the C entry point into outputs eight rows longer than asked and
prefilled; the trailing rows must come back untouched.  A handle has only the policy bound (no planner nets).
Shape cases: 2A = 2 .. 128 output columns (A = 1, 63, 64; 2A > mlp_dim; 2A = 66), in0 = 33 / 67 / 101 / 4096 (k_pol_gemv's single
tail and a wave without a share, pol_layer's 16 / 4 / 1-step tails), mlp_dim 32 .. 4096 (1, 2, 3 and 8 features per thread, idle
threads in the block sums), chunks of the spread route with last chunks of 1, 2, 3, 5, 7 and 9 rows (R = 1, 2, 4, 8, idle rows, a
last workgroup row of one row), 257 rows.  Value probes: log_std at both ends of its squash, eps = 0, |eps| = 30, saturated
actions, masks of one lane and of none, the band where log(relu(1 - a^2) + 1e-6) amplifies an ulp of tanhf.
TDMPC2_POLICY_EDGES_JSON=<file>: the worst err / gate per case, rows, route and output from this run and the emulation's ratio from
the CPU are written there (profiles/policy_edges.json).

What bites, from fourteen scratch builds of the library (one token changed in each, arithmetic or an in-bounds index only), each
run once on the MI355X against this file (73 tests then) and against tests/test_gpu_policy.py (26 tests).  "fp64" = test_pi_against_fp64;
variants 1-7 and 11 also fail test_refusals_leave_the_handle_usable, which gates a nine-row call of the row family (the "+ 1"):
1. k_pol_gemv's single tail dropped (`k < k0`): fp64 on spread fails for in0 = 33 (all seven row counts), 67 and 101 (9 + 1); the
   older file PASSES (its widths are multiples of 32: kq is even).
2. `kq = in / 8` in k_pol_gemv: the same 9 + 1; the older file PASSES.
3. the partials added over seven waves: fp64 on spread fails for all 15 shape runs (the probes' output layer is its bias alone);
   the older file fails 9.
4. pol_layer's final tail dropped: fp64 on row fails for in0 = 33, 67, 101 (9 + 1); the older file fails 6 (through act_pi's encoder
   layers, whose observation widths are odd; no policy layer of it has a tail).
5. `size = A` despite a mask: fp64 fails on both routes for every multitask case (20 shape runs, head_saturated); the older file fails 9.
6. the idle lanes' `on ?` dropped from the log_prob sum: fp64 fails on both routes for every case with A < 64 (26 runs); the older file fails 16.
7. `0.5 * ldif` -> `ldif`: all 36 fp64 runs fail; the older file fails 19.
8. host: the head's eps offset `r0` for `r0 * A`: fp64 on spread fails for every chunked case with A > 1 (11), the single-row test
   at n = 19 and 49, the draws test (its replay) and head_saturated's route comparison; the older file PASSES (one chunk everywhere).
9. host: the emb offset `r0` for `r0 * T`: fp64 on spread fails for the chunked cases with T = 3, 5 and 96; the row family has T = 1
   (r0 * T = r0), so its single-row tests cannot see this one -- the single-row test on the T = 3 case was added for it and fails
   on this variant (a run of its own, after the fourteen); the older file PASSES.
10. `row0` left out of the Philox row: test_draws_across_chunks alone fails (eps_out differs from the row route's and repeats across
    chunks); the older file PASSES.
11. `y[lane]` for `y[A + lane]` (log_std read from the mean's columns): all 36 fp64 runs fail; the older file fails 19.
12. host: the z offset `r0` for `r0 * L`: fp64 on spread fails for every chunked shape case (11; a probe's outputs do not depend on z) and the single-row test at n = 19 and 49;
    the older file PASSES.
13. host: the mask offset `r0` for `r0 * A`: fp64 on spread fails for every chunked multitask case (8), the single-row test at 19 and
    49 and head_saturated's route comparison; the older file PASSES.
14. host: the entropy offset `0` for `r0`: fp64 on spread fails for every chunked case (12), the single-row test at 19 and 49 and
    head_saturated's route comparison; the older file PASSES.
Not observable, so not built: `fmaxf(1 - a^2, 0)` removed (|tanhf| <= 1: the difference is never negative) and the `1e-8` dropped
from `lp + 1e-8` (below half an ulp of lp wherever |lp| >= 1, which every probe row keeps; at |lp| < 1e-8 scaled_entropy is
ill-conditioned in the reference itself)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import policy_edges_common as pe
from tests import policy_route_model as pr
from tests.gpu_common import dev

pytestmark = pytest.mark.gpu

ENV = "TDMPC2_POLICY_EDGES_JSON"
SENTINEL = -77.25
ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = 1, 2, 4
ROUTES = {"auto": 0, "row": 1, "spread": 2}
_handles, _worst = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _dump_worst():
    yield
    for h in _handles.values():
        h.planner.close()
    _handles.clear()
    path = os.environ.get(ENV)
    if path:
        emul, rows = {}, []
        for (name, n, route, k), v in sorted(_worst.items()):
            if (name, n, route) not in emul:
                emul[(name, n, route)] = pe.ratios(pe.case(name), pe.emulate(pe.case(name), route, n), n)
            rows.append(dict(case=name, rows=n, route=route, output=k, gpu_err_over_gate=v, emulation_err_over_gate=emul[(name, n, route)][k]))
        with open(path, "w") as f:
            json.dump({"gate": "max|HIP - ref64| <= 4 max(max|ref32 - ref64|, 2^-23 max(1, max|ref64|)); head_band: per value, "
                               "max(1e-5 max(1, |v64|), 2 |ref32 - v64|)",
                       "worst_gpu_err_over_gate": max(r["gpu_err_over_gate"] for r in rows), "pi": rows}, f, indent=1)
            f.write("\n")


@pytest.fixture(scope="module")
def route_lib(tmp_path_factory):
    return pr.build(tmp_path_factory.mktemp("policy_route"))


def d(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dev())


def _planner(cfg, max_envs):
    from tdmpc2_amd.native import NativePlanner

    return NativePlanner(cfg, cfg.iterations, dev(), max_envs=max_envs)


def _pi_sd(c):
    return {k: torch.as_tensor(v) for k, v in c.sd.items() if k.startswith("_pi.")}


class Handle:
    """One planner per case with the policy prior bound and nothing else."""

    def __init__(self, c):
        self.c = c
        self.planner = _planner(c.cfg, c.max_envs)
        self.planner.bind_policy(_pi_sd(c))

    def pi(self, rows, route, z=None, eps="case", seed=0, only_action=False, eps_out=False):
        """tdmpc2_plan_pi on rows `rows` (a count: the first rows; or an index list) of the case, on `route`, into outputs of
        n + 8 rows prefilled with the sentinel -> dict of numpy arrays (the n rows asked for); auto is restored afterwards."""
        from tdmpc2_amd.native import PolicyOut, _ptr

        c, p = self.c, self.planner
        idx = np.arange(rows) if np.isscalar(rows) else np.asarray(rows)
        n, A = len(idx), c.A
        zt = d((c.z if z is None else z)[idx])
        et, mt = (d(c.emb[idx]), d(c.mask[idx])) if c.tasks is not None else (None, None)
        ept = d(c.eps[idx]) if isinstance(eps, str) else d(eps)
        names = ("action",) if only_action else pe.OUTPUTS + (("eps_out",) if eps_out else ())
        buf = {k: torch.full((n + 8, 1 if "entropy" in k else A), SENTINEL, device=dev()) for k in names}
        out = PolicyOut(**{k: buf[k].data_ptr() for k in names})
        p.set_policy_route(ROUTES[route])
        try:
            with torch.cuda.device(dev()):
                p._check(p.lib.tdmpc2_plan_pi(p._h, n, _ptr(zt), _ptr(et), _ptr(mt), _ptr(ept), C.c_uint64(seed), C.byref(out), p._stream()))
            res = {k: v.cpu().numpy() for k, v in buf.items()}
        finally:
            p.set_policy_route(0)
        for k, v in res.items():
            assert (v[n:] == np.float32(SENTINEL)).all(), (c.name, route, n, k)
        return {k: v[:n] for k, v in res.items()}


def handle(name) -> Handle:
    c = pe.case(name)
    if name not in _handles:
        if c.big:  # the 4096-wide cases: one such handle at a time
            for k in [k for k in _handles if pe.case(k).big]:
                _handles.pop(k).planner.close()
            torch.cuda.empty_cache()
        _handles[name] = Handle(c)
    return _handles[name]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b, keys=pe.OUTPUTS):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


# ------------------------------------------------------------------------------------------------ 1: cases against fp64
@pytest.mark.parametrize("name,rows,route", [(n, r, route) for n, r in pe.runs() for route in ("row", "spread")])
def test_pi_against_fp64(name, rows, route):
    c = pe.case(name)
    got = handle(name).pi(rows, route)
    ratio = pe.ratios(c, got, rows)
    for k, v in ratio.items():
        _worst[(name, rows, route, k)] = v
    print(f"[{name} n={rows}] {route}: err / gate " + " ".join(f"{k}={v:.3f}" for k, v in ratio.items()))
    for k in pe.OUTPUTS:
        assert np.isfinite(got[k]).all(), k
        assert ratio[k] <= 1.0, (name, rows, route, k, ratio[k])
    if c.tasks is not None:  # masked action dimensions are exactly 0
        off = c.mask[:rows] == 0
        for k in ("action", "mean", "log_std"):
            assert (got[k][off] == 0).all(), k
    if c.kind == "head_inside":
        zero = [r for r in range(rows) if not c.eps[r].any()]
        assert len(zero) == 2 and np.array_equal(bits(got["action"][zero]), bits(got["mean"][zero]))
    if c.kind == "head_saturated":
        none = ~(c.mask[:rows] > 0).any(-1)
        assert none.sum() == 2 and (got["scaled_entropy"][none] == 0).all()
        live = c.mask[:rows] > 0
        assert (np.abs(got["action"][live]) == 1).all() and (np.abs(got["mean"][live]) == 1).all()


@pytest.mark.parametrize("name,rows", pe.runs())
def test_auto_takes_the_route_the_model_says(name, rows, route_lib):
    """No entry point reports the route: auto's outputs carry the bits of the forced route the model names (and, where the two
    routes' bits differ at all, not the other one's)."""
    c = pe.case(name)
    kind = pr.route(route_lib, rows, c.in0, c.M, c.A, max(c.in0, c.M, 2 * c.A), pr.AUTO)["kind"]
    h = handle(name)
    auto, row, spread = h.pi(rows, "auto"), h.pi(rows, "row"), h.pi(rows, "spread")
    want, other = (row, spread) if kind == pr.POL_ROW else (spread, row)
    assert same_bits(auto, want), (name, rows, kind)
    if c.kind == "shape":
        assert not same_bits(row, spread) and not same_bits(auto, other), (name, rows)
    else:  # exact head inputs: the two routes agree bit for bit
        assert same_bits(row, spread), name


# ------------------------------------------------------------------------------------------------ 2: exact properties
@pytest.mark.parametrize("route", ["row", "spread"])
@pytest.mark.parametrize("name,n", [(pe.ROW_FAMILY, 9), (pe.ROW_FAMILY, 19), (pe.ROW_FAMILY, 49), ("mt_67_544_A63", 19)])
def test_rows_equal_their_single_row_calls(name, n, route):
    """Row r of an n-row call = the single-row call on row r, bit for bit, in all five outputs (strides, grid.y, the chunk offsets
    r0 L / r0 T / r0 A / r0, and k_pol_gemv's per-row chains not depending on R).  The row family has T = 1, where r0 T = r0: the
    T = 3 case is there for the task columns' stride."""
    h = handle(name)
    full = h.pi(n, route)
    for r in range(n):
        one = h.pi([r], route)
        for k in pe.OUTPUTS:
            assert np.array_equal(bits(one[k][0]), bits(full[k][r])), (name, n, route, r, k)


@pytest.mark.parametrize("route", ["row", "spread"])
def test_optional_outputs_may_be_null(route):
    h = handle(pe.ROW_FAMILY)
    full, only = h.pi(19, route), h.pi(19, route, only_action=True)
    assert list(only) == ["action"] and np.array_equal(bits(only["action"]), bits(full["action"]))


def test_draws_across_chunks():
    """n = 49 on max_envs = 16: the spread route's chunks draw the rows the row route draws (row0 in the Philox row)."""
    h = handle(pe.ROW_FAMILY)
    p, outs = h.planner, {}
    k0 = p.call_counter()
    for route in ("row", "spread"):
        p.set_call_counter(k0)
        outs[route] = h.pi(49, route, eps=None, seed=7, eps_out=True)
        assert p.call_counter() == k0 + 1
    assert same_bits(outs["row"], outs["spread"], ("eps_out",))
    e = outs["spread"]["eps_out"].reshape(-1)
    assert len(np.unique(e)) == 49 * h.c.A and np.isfinite(e).all()
    replay = h.pi(49, "spread", eps=outs["spread"]["eps_out"])
    assert same_bits(replay, outs["spread"])


@pytest.mark.parametrize("route", ["row", "spread"])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_nonfinite_latent_stays_in_its_row(bad, route):
    """A NaN or +inf in one row's z: that row's outputs are NaN (LayerNorm spreads it), every other row is bit-identical."""
    h = handle(pe.ROW_FAMILY)
    c, n, r = h.c, 9, 4   # row 4 shares its R = 8 workgroup with seven clean rows
    clean = h.pi(n, route)
    z = c.z.copy()
    z[r, c.L // 2] = bad
    got = h.pi(n, route, z=z)
    keep = np.arange(n) != r
    for k in pe.OUTPUTS:
        assert np.isnan(got[k][r]).all(), (k, got[k][r])
        assert np.array_equal(bits(got[k][keep]), bits(clean[k][keep])), k


# ------------------------------------------------------------------------------------------------ 3: refusals
@pytest.mark.parametrize("L,M,A,msg", [(32, 32, 0, "action_dim 0 "), (32, 32, 65, "action_dim 65 "), (40, 32, 4, "latent_dim %"),
                                       (32, 40, 4, "mlp_dim %"), (32, 48, 4, "mlp_dim %")])
def test_creation_refuses(L, M, A, msg):
    """What a handle cannot be created with never reaches the policy prior: A outside [1, 64], widths off the planner's 32-tiles
    (so the cases' L and M are multiples of 32)."""
    from tdmpc2_amd.native import NativeError

    with pytest.raises(NativeError, match=f"error {ERR_UNSUPPORTED}:.*{msg}"):
        _planner(pe.make_cfg(L, 0, M, A), 2)


def test_refusals_leave_the_handle_usable():
    from tdmpc2_amd.native import NativeError, PolicyOut, _ptr

    L, T = pe.REFUSED_BIND
    cfg = pe.make_cfg(L, T, 32, 2)
    p = _planner(cfg, 2)
    rng = np.random.default_rng(0)
    sd = {}
    for l, (o, i) in enumerate(((32, L + T), (32, 32), (4, 32))):
        sd[f"_pi.{l}.weight"] = torch.as_tensor((0.02 * rng.standard_normal((o, i))).astype(np.float32))
        for nm in ("bias", "ln.weight", "ln.bias")[:3 if l < 2 else 1]:
            sd[f"_pi.{l}.{nm}"] = torch.ones(o)
    with pytest.raises(NativeError, match=f"error {ERR_UNSUPPORTED}:.*{L + T}"):
        p.bind_policy(sd)
    z = torch.zeros(1, L, device=dev())
    act = torch.full((1, 2), SENTINEL, device=dev())
    e, m = torch.zeros(1, T, device=dev()), torch.ones(1, 2, device=dev())
    rc = p.lib.tdmpc2_plan_pi(p._h, 1, _ptr(z), _ptr(e), _ptr(m), None, C.c_uint64(0), C.byref(PolicyOut(action=act.data_ptr())), p._stream())
    assert rc == ERR_STATE and (act.cpu().numpy() == np.float32(SENTINEL)).all()   # nothing was bound, nothing ran
    p.close()

    h = handle(pe.ROW_FAMILY)
    c, q = h.c, h.planner
    before = h.pi(9, "spread")
    act = torch.full((9, c.A), SENTINEL, device=dev())
    rc = q.lib.tdmpc2_plan_pi(q._h, 0, _ptr(d(c.z[:9])), _ptr(d(c.emb[:9])), _ptr(d(c.mask[:9])), _ptr(d(c.eps[:9])), C.c_uint64(0),
                              C.byref(PolicyOut(action=act.data_ptr())), q._stream())
    assert rc == ERR_INVALID and b"n_rows 0" in q.lib.tdmpc2_last_error() and (act.cpu().numpy() == np.float32(SENTINEL)).all()
    for route in ("row", "spread"):
        got = h.pi(9, route)
        assert max(pe.ratios(c, got, 9).values()) <= 1.0
    assert same_bits(h.pi(9, "spread"), before)
