"""-m gpu: the state encoder (tdmpc2_plan_bind_encoder / tdmpc2_plan_encode, and its row copy inside tdmpc2_plan_act_pi) against an
fp64 reference at its shape, value and route edges (tests/encoder_common.py; tests/test_encoder_edges.py checks the restatements,
the probes and the order emulation on the CPU).

Gate, per case: max|z - z64| <= 4 max(max|z_ref32 - z64|, 2^-23), z_ref32 = the oracle in fp32 on the CPU.  Every call goes through
the C entry point into a z eight rows longer than asked and prefilled; the trailing rows must come back untouched.
Shape cases: k-loop tails (in % 4, in % 16, a wave of k_enc_gemv without a share), the feature tiling f = tid + u 512 (outputs 63,
65, 511, 512, 513, 1023, 1024, 1025, 4095, 4096), the route chosen by a 1025-wide observation alone, the widest input a handle
accepts, depths 1 and 6, E = 1, 2, max_envs, 3 max_envs + 1.  Value probes (selection weights, integer observations: the
pre-activations are exact in any order, so a wrong index is an error of order 1): a Mish sweep over [-40, 100], LayerNorm on a
constant row, on 1e4 + small and on a row with one outlier, SimNorm groups spread over 100 / tied / all equal, row-distinct task columns.
Creation refuses simnorm_dim != 8 and latents that are no multiple of 32, so the simnorm_dim sweep and the latents 8, 16 and 72 are
pinned as refusals and the shapes that ended in them end in 32 / 96.
TDMPC2_ENCODER_EDGES_JSON=<file>: the worst err / gate per case and route from this run and the emulation's ratio from the CPU are
written there (profiles/encoder_edges.json).

What bites, from ten scratch builds of the library (one token changed in each, arithmetic or an in-bounds index only), each run
once on the MI355X against this file (78 tests; 72 when 1-7 ran, before the narrow probes went through act_pi) and against
tests/test_gpu_encoder.py (13 tests):
1. k_encode's `k < in` tail loop dropped: 11 narrow cases (every one with in % 4 != 0 in some layer, n_task among them), the
   non-finite test whose bad column is in the tail, and act_pi beyond the row route fail (14); the older file fails 6.
2. `kq = in / 4` in k_enc_gemv: 7 wide cases fail (every one with in % 4 != 0 in some layer); the older file fails 2.
3. `fminf(v, 20)` removed (k_encode, k_enc_norm): n_mish and w_mish fail (their sweep goes on to 45, 60, 89, 100: below 44.4 the
   clamp changes no bit, so a sweep that ends at 40 cannot see it); the older file PASSES.
4. SimNorm's max subtraction removed (k_encode, k_enc_norm): n_simnorm and w_simnorm fail; the older file PASSES.
5. `out - 1` in k_encode's variance: all 19 narrow cases and act_pi beyond the row route fail; the older file fails 7.
6. `xa[i]` for `xa[obs_dim + i]` on k_encode's task columns: the three narrow multitask cases, their single-row and non-finite
   tests fail (6); the older file fails 3.
7. pol_layer's final tail loop dropped: 10 row-copy cases fail (in % 4 != 0); the older file PASSES (it never runs act_pi).
8. `fminf(v, 20)` removed in pol_layer: the row copy of n_mish fails; 9. SimNorm's max subtraction removed in pol_layer: the row
   copy of n_simnorm fails.  Both were gaps until the narrow probes also ran through act_pi; the older file PASSES both.
10. `width - 1` in k_enc_norm's variance: all 13 wide cases and act_pi beyond the row route fail; the older file fails 2."""
import json
import os
import struct

import numpy as np
import pytest
import torch

from tests import encoder_common as ec
from tests import policy_route_model as pr
from tests.gpu_common import case_on_gpu, dev

pytestmark = pytest.mark.gpu

ENV = "TDMPC2_ENCODER_EDGES_JSON"
SENTINEL = -77.25
UNSUPPORTED = "error 2:"   # TDMPC2_ERR_UNSUPPORTED
_handles, _worst, _worst_pi = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _dump_worst():
    yield
    for h in _handles.values():
        h.planner.close()
    _handles.clear()
    path = os.environ.get(ENV)
    if path:
        rows = []
        for name, v in sorted(_worst.items()):
            c = ec.case(name)
            a, b, _ = ec.refs(c)
            rows.append(dict(case=name, route=c.route, E=c.E, gpu_err_over_gate=v,
                             emulation_err_over_ref_err=float(np.abs(ec.emulate(c) - a).max() / ec.ref_err(a, b))))
        with open(path, "w") as f:
            json.dump({"gate": "max|z - z64| <= 4 max(max|z_ref32 - z64|, 2^-23)", "emulation_bound": ec.FACTOR, "encode": rows,
                       "row_copy": [dict(case=k[0], output=k[1], gpu_err_over_gate=v) for k, v in sorted(_worst_pi.items())]}, f, indent=1)
            f.write("\n")


@pytest.fixture(scope="module")
def route_lib(tmp_path_factory):
    return pr.build(tmp_path_factory.mktemp("policy_route"))


def d(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dev())


def _planner(cfg, max_envs=ec.MAX_ENVS):
    from tdmpc2_amd.native import NativePlanner

    return NativePlanner(cfg, cfg.iterations, dev(), max_envs=max_envs)


class Handle:
    """One planner per case (a handle's encoder cannot change shape), the encoder bound, the policy prior on demand."""

    def __init__(self, c):
        self.c = c
        self.planner = _planner(c.cfg, c.max_envs)
        self.sd = {k: torch.as_tensor(v) for k, v in c.sd.items()}
        self.planner.bind_encoder(self.sd)
        assert self.planner.encoder_layers == len(c.widths)
        self.pi_bound = False

    def encode(self, obs, emb):
        """tdmpc2_plan_encode on the rows of obs into a z of rows + 8 prefilled with the sentinel -> z [rows, L] (numpy)."""
        from tdmpc2_amd.native import _ptr

        p, E, L = self.planner, int(obs.shape[0]), self.c.widths[-1]
        ot, et = d(np.asarray(obs, np.float32)), d(emb)
        z = torch.full((E + 8, L), SENTINEL, device=dev())
        with torch.cuda.device(dev()):
            p._check(p.lib.tdmpc2_plan_encode(p._h, E, _ptr(ot), self.c.obs_dim, _ptr(et), _ptr(z), p._stream()))
        res = z.cpu().numpy()
        assert (res[E:] == np.float32(SENTINEL)).all(), (self.c.name, E)
        return res[:E]

    def act_pi(self, eps):
        if not self.pi_bound:
            self.planner.bind_policy(self.sd)
            self.pi_bound = True
        c = self.c
        _, info = self.planner.act_pi(d(c.obs), d(c.emb), d(c.mask), eps=d(eps))
        return {k: info[k].cpu().numpy() for k in ("mean", "log_std")}


def handle(c) -> Handle:
    if c.name not in _handles:
        _handles[c.name] = Handle(c)
    return _handles[c.name]


# ------------------------------------------------------------------------------------------------ 1, 2: cases against fp64
@pytest.mark.parametrize("name", ec.NAMES)
def test_encode_against_fp64(name):
    c = ec.case(name)
    z64, _, gate = ec.refs(c)
    z = handle(c).encode(c.obs, c.emb)
    assert np.isfinite(z).all()
    err = float(np.abs(z - z64).max())
    _worst[name] = err / gate
    print(f"[{name}] {c.route}: max|HIP - fp64| = {err:.3e}, gate {gate:.3e}, err / gate = {err / gate:.3f}")
    assert err <= gate


# ------------------------------------------------------------------------------------------------ 3: exact properties
ROW_CASES = ["n_5_65_513_96", "n_mt_17p2_1024_1023_1024", "n_3_63_64_E49", "w_5_1025_64", "w_mt_39p96_4095_1376", "w_depth6"]


@pytest.mark.parametrize("name", ROW_CASES)
def test_rows_equal_their_single_row_calls(name):
    """Row r of a call with E rows = the E = 1 call on that row, bit for bit (obs | task_emb strides, grid.y, no cross-row state)."""
    c = ec.case(name)
    h, emb = handle(c), c.emb
    z = h.encode(c.obs, emb)
    for r in range(c.E):
        one = h.encode(c.obs[r:r + 1], None if emb is None else emb[r:r + 1])
        assert np.array_equal(one[0].view(np.uint32), z[r].view(np.uint32)), (name, r)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("name", ["n_3_63_64", "n_mt_17p2_1024_1023_1024", "w_5_1025_64", "w_mt_39p96_4095_1376"])
def test_nonfinite_observation_stays_in_its_row(name, bad):
    """A NaN or +inf in one row's observation: that row of z is all NaN (LayerNorm spreads it), every other row is bit-identical."""
    c = ec.case(name)
    h = handle(c)
    clean = h.encode(c.obs, c.emb)
    obs, r = c.obs.copy(), c.E - 1
    obs[r, c.obs_dim // 2] = bad
    z = h.encode(obs, c.emb)
    assert np.isnan(z[r]).all(), (name, bad, z[r][:8])
    keep = np.arange(c.E) != r
    assert np.array_equal(z[keep].view(np.uint32), clean[keep].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 4: the row copy
def _pi_check(c, route_lib, want_kind):
    cfg = c.cfg
    enc_w = max((c.obs_dim + c.T,) + c.widths)
    in0, M, A = cfg.latent_dim + cfg.task_dim, cfg.mlp_dim, cfg.action_dim
    r = pr.route(route_lib, c.E, in0, M, A, max(in0, M, 2 * A, enc_w), pr.AUTO)
    inside = enc_w <= ec.ENC_WIDE and r["kind"] == pr.POL_ROW   # launch_pi's choice
    assert inside == (want_kind == pr.POL_ROW), (c.name, r)
    eps = np.random.default_rng(5).standard_normal((c.E, A)).astype(np.float32)
    g64, g32 = ec.pi_refs(c, eps)
    out = handle(c).act_pi(eps)
    for k in ("mean", "log_std"):
        gate = ec.gate(g64[k], g32[k])
        err = float(np.abs(out[k] - g64[k]).max())
        _worst_pi[(c.name, k)] = err / gate
        print(f"[{c.name}] act_pi {k}: max|HIP - fp64| = {err:.3e}, gate {gate:.3e}, err / gate = {err / gate:.3f}")
        assert err <= gate, (c.name, k)


@pytest.mark.parametrize("name", ec.PI_NAMES)
def test_row_copy_against_fp64(name, route_lib):
    """act_pi on a narrow encoder with few rows: the encoder runs inside k_pol_row (pol_layer), checked through mean and log_std."""
    _pi_check(ec.case(name), route_lib, pr.POL_ROW)


def test_act_pi_beyond_the_row_route(route_lib):
    """257 rows leave the row route: launch_pi runs the encoder by its own launch into the handle's latents, then the spread policy."""
    _pi_check(ec.pi_spread_case(), route_lib, pr.POL_SPREAD)


# ------------------------------------------------------------------------------------------------ 5: refusals
def _enc_sd(obs_dim, widths, seed=0):
    rng, sd, fin = np.random.default_rng(seed), {}, obs_dim
    for l, out in enumerate(widths):
        sd[f"_encoder.state.{l}.weight"] = torch.as_tensor((0.02 * rng.standard_normal((out, fin))).astype(np.float32))
        for n in ("bias", "ln.weight", "ln.bias"):
            sd[f"_encoder.state.{l}.{n}"] = torch.ones(out)
        fin = out
    return sd


@pytest.mark.parametrize("latent,simnorm_dim,msg", [(64, 1, "simnorm_dim 1 "), (64, 2, "simnorm_dim 2 "), (64, 4, "simnorm_dim 4 "),
                                                    (64, 16, "simnorm_dim 16 "), (64, 64, "simnorm_dim 64 "), (1088, 16, "simnorm_dim 16 "),
                                                    (66, 3, "simnorm_dim 3 "), (128, 128, "simnorm_dim 128 "), (36, 8, "latent_dim 36"),
                                                    (8, 8, "latent_dim"), (16, 8, "latent_dim"), (72, 8, "latent_dim")])
def test_creation_refuses(latent, simnorm_dim, msg):
    """What a handle cannot be created with never reaches the encoder: SimNorm groups other than 8, latents off the planner's tiles."""
    from tdmpc2_amd.native import NativeError

    with pytest.raises(NativeError, match=UNSUPPORTED + ".*" + msg):
        _planner(ec.make_cfg(latent, 0, simnorm_dim))


def test_bind_and_call_refusals():
    from tdmpc2_amd.native import NativeError

    cfg = ec.make_cfg(64, 0)
    p = _planner(cfg, max_envs=2)

    def refused(sd, msg):
        with pytest.raises(NativeError, match=msg):
            p.bind_encoder(sd)
        p.obs_dim = 4
        with pytest.raises(NativeError, match="no encoder bound"):   # nothing was bound, nothing ran
            p.encode(torch.zeros(1, 4, device=dev()))

    refused(_enc_sd(4, (4097, 64)), UNSUPPORTED + ".*width 4097")
    refused(_enc_sd(4, (8,) * 6 + (64,)), "depth 7")
    refused(_enc_sd(ec.ENC_MAX_IN + 1, (64,)), UNSUPPORTED + f".*{ec.ENC_MAX_IN + 1} inputs, at most {ec.ENC_MAX_IN}")
    p.bind_encoder(_enc_sd(1030, (16, 64)))   # wide by its observation
    with pytest.raises(NativeError, match="takes 1030 inputs, the data brings 1029"):
        p.obs_dim = 1029
        p.encode(torch.zeros(1, 1029, device=dev()))
    p.obs_dim = 1030
    with pytest.raises(NativeError, match="max_envs = 2"):
        p.encode(torch.zeros(3, 1030, device=dev()))
    assert torch.isfinite(p.encode(torch.zeros(2, 1030, device=dev()))).all()
    p.close()


def test_import_packed_refuses_an_oversized_input():
    """A packed blob whose header names an encoder input beyond the LDS limit is refused before its encoder is allocated."""
    from tdmpc2_amd.native import NativeError

    c, _, planner = case_on_gpu("small")
    blob = bytearray(planner.export_packed())
    off_layers, off_in, off_out = 124, 128, 152   # struct PackHdr (tests/refresh_common.py: HDR_BYTES)
    if struct.unpack_from("<I", blob, off_layers)[0] == 0:
        struct.pack_into("<I", blob, off_layers, 1)
        struct.pack_into("<i", blob, off_out, c["cfg"].latent_dim)
    struct.pack_into("<i", blob, off_in, ec.ENC_MAX_IN + 1)
    fresh = _planner(c["cfg"], max_envs=2)
    with pytest.raises(NativeError, match=UNSUPPORTED + f".*at most {ec.ENC_MAX_IN}"):
        fresh.import_packed(bytes(blob))
    fresh.close()
