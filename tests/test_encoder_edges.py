"""CPU: what tests/test_gpu_encoder_edges.py stands on (tests/encoder_common.py) -- the two fp64 restatements of the state encoder
agree, the cases reach the edges they are named for, the value probes' pre-activations are exact, the library's limits are the
ones the cases assume, and the numpy emulation of the kernels' summation order stays within the gate's factor of the reference's
own fp32 error on every case (measured before any GPU run: DESIGN 3.4)."""
import os
import re

import numpy as np
import pytest

from tests import encoder_common as ec
from tests import policy_route_model as pr

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tdmpc2_amd", "csrc")


def _stages64(c):
    """fp64: per layer (pre-activation y, v = LayerNorm(y) g + b) of a case, from the fp32 inputs promoted"""
    x = np.asarray(c.obs, np.float64)
    if c.tasks is not None:
        x = np.concatenate([x, c.emb.astype(np.float64)], -1)
    out = []
    for l in range(len(c.widths)):
        p = f"_encoder.state.{l}."
        y = x @ np.asarray(c.sd[p + "weight"], np.float64).T + np.asarray(c.sd[p + "bias"], np.float64)
        n = (y - y.mean(-1, keepdims=True)) / np.sqrt(y.var(-1, keepdims=True) + 1e-5)
        v = n * np.asarray(c.sd[p + "ln.weight"], np.float64) + np.asarray(c.sd[p + "ln.bias"], np.float64)
        out.append((y, v))
        x = v * np.tanh(np.logaddexp(0.0, v))
    return out


def test_limits_are_the_librarys():
    src = open(os.path.join(CSRC, "encoder_params.h")).read()

    def const(name):
        return eval(re.search(rf"constexpr \w+ {name} = ([0-9 *]+);", src).group(1))

    assert const("ENC_WIDE") == ec.ENC_WIDE and const("ENC_MAX_LAYERS") == ec.ENC_MAX_LAYERS and const("ENC_THREADS") == ec.THREADS
    assert const("ENC_THREADS") * const("ENC_MAX_PER_THREAD") == ec.ENC_MAX_WIDTH
    assert const("ENC_GEMV_LDS_MAX") == ec.ENC_GEMV_LDS_MAX
    assert "ENC_MAX_IN = (int)(ENC_GEMV_LDS_MAX / 4) - 256" in src and ec.ENC_MAX_IN == 16128
    # the request k_enc_gemv's launch makes for the widest input is the limit itself; one more column is over it
    assert (ec.ENC_MAX_IN + 256) * 4 == ec.ENC_GEMV_LDS_MAX < (ec.ENC_MAX_IN + 1 + 256) * 4
    host = "".join(open(os.path.join(CSRC, f)).read() for f in ("plan_weights.hip", "plan_obs.hip"))
    assert "((size_t)L.in + 256) * 4" in host and host.count("> ENC_MAX_IN") == 2   # ensure_enc_alloc (bind, import: plan_weights.hip) and launch_encode (plan_obs.hip)


def test_cases_reach_their_edges():
    cs = [ec.case(n) for n in ec.NAMES]
    assert len({c.name for c in cs}) == len(cs)
    for c in cs:
        assert c.route == ("wide" if c.name.startswith("w_") else "narrow"), c.name
        assert c.E * c.widths[-1] >= ec.MIN_ELEMENTS and len(c.widths) <= ec.ENC_MAX_LAYERS and max(c.widths) <= ec.ENC_MAX_WIDTH
        assert c.route == "narrow" or c.E <= c.max_envs
        assert c.widths[-1] % 32 == 0
    shape = [c for c in cs if c.kind == "shape"]
    ins = {(c.route, (c.obs_dim + c.T,) + c.widths[:-1]) for c in shape}
    narrow_in = {k for r, t in ins if r == "narrow" for k in t}
    wide_in = {k for r, t in ins if r == "wide" for k in t}
    assert {k % 4 for k in narrow_in} == {0, 1, 2, 3} and {15, 16, 17, 19} <= narrow_in   # k_encode / pol_layer tails
    assert {k % 16 for k in narrow_in} >= {0, 1, 3, 15}
    assert 5 in wide_in and 9 in wide_in          # k_enc_gemv: waves without a share (in = 5: wave 3; in = 9: k0 = 9 = k1)
    assert 1025 in wide_in and ec.ENC_MAX_IN in wide_in and 1024 in narrow_in
    outs = {w for c in shape for w in c.widths}
    assert {63, 65, 511, 512, 513, 1023, 1024, 1025, 4095, 4096} <= outs
    assert {len(c.widths) for c in shape if c.route == "narrow"} >= {1, 6} and 6 in {len(c.widths) for c in shape if c.route == "wide"}
    assert {1, 2, ec.MAX_ENVS} <= {c.E for c in shape} and any(c.E == 3 * ec.MAX_ENVS + 1 and c.route == "narrow" for c in shape)
    assert any(c.T and c.route == "narrow" for c in shape) and any(c.T == 96 and c.E == c.max_envs and c.route == "wide" for c in shape)
    for kind in ("mish", "ln_const", "ln_offset", "ln_outlier", "simnorm", "task"):
        assert {c.route for c in cs if c.kind == kind} == {"narrow", "wide"}, kind


@pytest.mark.parametrize("name", ec.NAMES + [ec.PI_SPREAD])
def test_fp64_restatements_agree_and_emulation_within_gate(name):
    c = ec.case(name) if name != ec.PI_SPREAD else ec.pi_spread_case()
    z64, z32, gate = ec.refs(c)
    assert np.abs(ec.z64_oracle(c) - z64).max() <= 1e-12
    assert np.abs(z32 - z64).max() <= gate and np.isfinite(z64).all()
    np.testing.assert_allclose(z64.reshape(c.E, -1, 8).sum(-1), 1.0, atol=1e-12)
    ratio = float(np.abs(ec.emulate(c) - z64).max() / ec.ref_err(z64, z32))
    print(f"[{name}] {c.route}: emulation err / reference's fp32 err = {ratio:.2f}")
    assert ratio <= ec.FACTOR


def test_emulation_sees_a_dropped_tail_and_a_floored_split():
    """The emulation is of the ORDER: with k_encode's tail dropped or k_enc_gemv's split floored it leaves the gate by far."""
    c = ec.case("n_3_63_64")
    z64, z32, gate = ec.refs(c)
    real = ec._chains
    try:
        ec._chains = lambda x, wt, k0, k1: real(x, wt, k0, k0 + (k1 - k0) // 4 * 4)
        assert np.abs(ec.emulate(c) - z64).max() > 100 * gate
    finally:
        ec._chains = real
    assert np.abs(ec.emulate(c) - z64).max() <= gate


@pytest.mark.parametrize("route", ["n", "w"])
def test_value_probes(route):
    exact = lambda c, l=0: np.array_equal(_stages64(c)[l][0] * 32, np.round(_stages64(c)[l][0] * 32))  # noqa: E731
    c = ec.case(f"{route}_mish")
    v = _stages64(c)[0][1]
    assert exact(c) and v.min() < -39.9 and v.max() > 99.9 and (v < -30).any() and ((v > 44.4) & (v < 88.0)).any()
    assert ((v >= 19.9) & (v < 20.0)).any() and ((v > 20.0) & (v <= 20.1)).any() and len(np.unique(np.round(v[0]))) > 30
    c = ec.case(f"{route}_ln_const")
    y = _stages64(c)[0][0]
    assert exact(c) and (y.var(-1) == 0).all() and (y[0] == 0).all() and (y[1:] != 0).any()
    c = ec.case(f"{route}_ln_offset")
    y = _stages64(c)[0][0]
    assert exact(c) and (np.abs(y) > 9990).all() and (y.std(-1) < 3).all() and (y.std(-1) > 0.5).all()
    c = ec.case(f"{route}_ln_outlier")
    y = _stages64(c)[0][0]
    assert exact(c) and ((np.abs(y) == 60000).sum(-1) >= 1).all() and (np.median(np.abs(y), -1) <= 6).all()
    c = ec.case(f"{route}_simnorm")
    v = _stages64(c)[1][1].reshape(c.E, -1, 8)
    spread = v.max(-1) - v.min(-1)
    assert exact(c) and (spread > 100).any() and (spread[:, 0] == 0).all()                    # group 0: all equal
    assert (v[:, 1, :4] == v[:, 1, :1]).all() and (v[:, 1, 4:] == v[:, 1, 4:5]).all() and (v[:, 1, 0] != v[:, 1, 4]).any()  # ties
    assert (np.sort(v, -1)[:, :, -1] == np.sort(v, -1)[:, :, -2]).any()
    c = ec.case(f"{route}_task")
    y, emb = _stages64(c)[0][0], c.emb
    assert exact(c) and len({tuple(r) for r in emb}) == c.E
    sel = (np.arange(c.widths[0]) * 7 + 3) % (c.obs_dim + c.T)
    x = np.concatenate([c.obs, emb], -1)
    assert np.array_equal(np.abs(y), np.abs(x[:, sel])) and (sel >= c.obs_dim).sum() >= 8
    # reading the observation's columns in place of the task columns, or another row's task, moves z by far more than the gate
    z64, _, gate = ec.refs(c)
    for wrong in (np.concatenate([c.obs, c.obs[:, :c.T]], -1), np.concatenate([c.obs, np.roll(emb, 1, 0)], -1)):
        shifted = ec.Case("x", c.obs_dim + c.T, 0, c.widths, c.E, cfg=ec.make_cfg(c.widths[-1], 0), sd=c.sd, obs=wrong.astype(np.float32))
        assert np.abs(ec.pc.fp64_encode(shifted.cfg, shifted.sd, shifted.obs, None) - z64).max() > 1000 * gate


def test_row_copy_cases_take_the_route_they_are_named_for(tmp_path):
    lib = pr.build(tmp_path)
    for c in [ec.case(n) for n in ec.PI_NAMES] + [ec.pi_spread_case()]:
        in0, M, A = c.cfg.latent_dim + c.cfg.task_dim, c.cfg.mlp_dim, c.cfg.action_dim
        enc_w = max((c.obs_dim + c.T,) + c.widths)
        r = pr.route(lib, c.E, in0, M, A, max(in0, M, 2 * A, enc_w), pr.AUTO)
        assert c.route == "narrow" and c.E <= c.max_envs
        assert (r["kind"] == pr.POL_ROW) == (c.name != ec.PI_SPREAD), c.name
    ins = {k for n in ec.PI_NAMES for c in [ec.case(n)] for k in (c.obs_dim + c.T,) + c.widths[:-1]}
    assert {15, 16, 17, 19} <= ins and {k % 16 for k in ins} >= {0, 1, 3, 15} and any(ec.case(n).T for n in ec.PI_NAMES)
