"""CPU test of what tdmpc2_plan_create decides before it touches the device (tdmpc2_amd/csrc/plan_layout.h, compiled with g++ behind
the shim of tests/layer_route_model.py): the refusals with their codes and messages, the byte totals against the handles the parent
commit created on an MI355X (tests/golden/create_bytes.json), and which buffers exist under which condition.  The GPU test at the
end closes the loop: what create allocates is what the header says."""
import json
import os

import pytest

from tdmpc2_amd import native
from tdmpc2_amd.config import named_config, planner_iterations
from tests import layer_route_model as lrm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 2  # enum tdmpc2_status
FUSED, LAYERED, FP32, SPLIT = native.PATH_FUSED, native.PATH_LAYERED, native.PREC_FP32, native.PREC_SPLIT_F16

FUSED_BUFS = {"cvec", "zscratch"}
CL_BUFS = {"cl_xbuf", "cl_zs", "cl_flags"}
CL2_BUFS = {"cl2_xbuf", "cl2_zs", "cl2_flags", "cl2_mail"}
LAYERED_BUFS = {"X", "HA", "HB", "LG", "G", "QT", "TERM", "qidx"}
# what TDMPC2_ONE_STREAM takes away: the second chain's activations and logits, its pre-activation buffer, and the few-row path's
# partial sums (create allocates them only where the second buffer set exists); its K-split workspace goes with them (ksws_ensure)
SECOND_CHAIN_BUFS = {"HA2", "HB2", "LG2", "PRE2", "mws[0]", "mws[1]"}
SPLIT_ONLY_BUFS = {"Z0X", "lay.cvec", "stats", "stats2", "arrive", "mws[0]", "mws[1]", "PRE", "PRE2"}
ZEROED = {"ticket", "cl_flags", "cl2_flags", "X", "HA", "HB", "beff", "Z0X", "HA2", "HB2", "arrive"}  # ("beff": layered family only)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return lrm.build(tmp_path_factory.mktemp("plan_layout"))


def c1(**over):
    """struct tdmpc2_plan_cfg of a c1 handle for one plan, with fields replaced"""
    c = native.plan_cfg(named_config("c1"), 6, 1)
    for k, v in over.items():
        setattr(c, k, v)
    return c


def named(name, E=1, path=native.PATH_AUTO, precision=native.PREC_AUTO, **over):
    cfg = named_config(name, **over)
    return native.plan_cfg(cfg, planner_iterations(cfg), E, 0, path, precision)


# ---------------------------------------------------------------------------------------------------------------- refusals
NVS = "num_valid_samples %d: 0, or the true sample count behind num_samples 512 rounded up to the row tile (>= num_elites %d, > num_pi_trajs 24)"
LAYERED_NEEDS = "layered planner kernels need latent_dim %% 32 == 0, mlp_dim %% 32 == 0 and num_samples %% 128 == 0 (got %d / %d / %d)"
# One case (or one per clause) for every check of create, in create's order: the smallest change to c1 (H3 N512 elites 64 P24 A6 L512
# M512 bins 101 q5) that trips it -> (code, the whole message).  The strings are those of tdmpc2_plan_create at commit 4dad628.
REFUSALS = [
    (dict(action_dim=0), UNSUPPORTED, "action_dim 0 outside [1, 64]"),
    (dict(action_dim=65), UNSUPPORTED, "action_dim 65 outside [1, 64]"),
    (dict(num_bins=-1), UNSUPPORTED, "num_bins -1 outside [0, 128]"),
    (dict(num_bins=129), UNSUPPORTED, "num_bins 129 outside [0, 128]"),
    (dict(num_q=1), UNSUPPORTED, "num_q 1 outside [2, 8]"),
    (dict(num_q=9), UNSUPPORTED, "num_q 9 outside [2, 8]"),
    (dict(horizon=0), UNSUPPORTED, "horizon 0 outside [1, 8]"),
    (dict(horizon=9), UNSUPPORTED, "horizon 9 outside [1, 8]"),
    (dict(num_samples=500), UNSUPPORTED, "num_samples 500 must be a multiple of 64 in [64, 1024]"),
    (dict(num_samples=0), UNSUPPORTED, "num_samples 0 must be a multiple of 64 in [64, 1024]"),
    (dict(num_samples=1088), UNSUPPORTED, "num_samples 1088 must be a multiple of 64 in [64, 1024]"),
    (dict(num_pi_trajs=-1), UNSUPPORTED, "num_pi_trajs -1 outside [0, 64]"),
    (dict(num_pi_trajs=65), UNSUPPORTED, "num_pi_trajs 65 outside [0, 64]"),
    (dict(num_pi_trajs=64, num_samples=64), UNSUPPORTED, "num_pi_trajs 64 outside [0, 64]"),  # (not fewer than the samples)
    (dict(num_elites=0), INVALID, "num_elites 0"),
    (dict(num_elites=513), INVALID, "num_elites 513"),
    (dict(num_valid_samples=63), INVALID, NVS % (63, 64)),                   # fewer than the elites
    (dict(num_valid_samples=513), INVALID, NVS % (513, 64)),                 # more than the rows
    (dict(num_valid_samples=24, num_elites=8), INVALID, NVS % (24, 8)),      # not more than the policy-prior rows
    (dict(num_valid_samples=384), INVALID, NVS % (384, 64)),                 # a whole 128-row tile of padding
    (dict(simnorm_dim=4), UNSUPPORTED, "simnorm_dim 4 (kernels are built for 8)"),
    (dict(multitask=1), INVALID, "multitask needs task_dim > 0"),
    (dict(multitask=1, task_dim=64, episodic=1), UNSUPPORTED, "termination head with task ids is not supported (reference world_model.py:136)"),
    (dict(iterations=0), INVALID, "iterations / max_envs must be positive"),
    (dict(max_envs=0), INVALID, "iterations / max_envs must be positive"),
    (dict(latent_dim=4), UNSUPPORTED, "latent_dim 4 / mlp_dim 512"),
    (dict(mlp_dim=4), UNSUPPORTED, "latent_dim 512 / mlp_dim 4"),
    (dict(latent_dim=516), UNSUPPORTED, "latent_dim 516 / mlp_dim 512"),
    (dict(path=FUSED, latent_dim=768), UNSUPPORTED, "fused planner kernels are built for latent_dim == mlp_dim == 512 (got 768 / 512)"),
    (dict(path=LAYERED, num_samples=448), UNSUPPORTED, LAYERED_NEEDS % (512, 512, 448)),
    (dict(latent_dim=520), UNSUPPORTED, LAYERED_NEEDS % (520, 512, 512)),    # (chosen automatically: not the fused width)
    (dict(path=9), INVALID, "unknown path 9"),
    (dict(path=-1), INVALID, "unknown path -1"),
    (dict(precision=7), INVALID, "unknown precision 7"),
    (dict(mlp_dim=4128), UNSUPPORTED, "the layered f16x2-split row kernels hold a row of at most 4096 columns in registers"),
    (dict(latent_dim=4128, mlp_dim=1024), UNSUPPORTED, "the layered f16x2-split row kernels hold a row of at most 4096 columns in registers"),
    # ---- two checks tripped: the earlier one is reported
    (dict(action_dim=0, num_bins=129), UNSUPPORTED, "action_dim 0 outside [1, 64]"),
    (dict(num_q=1, horizon=0), UNSUPPORTED, "num_q 1 outside [2, 8]"),
    (dict(num_samples=500, path=LAYERED), UNSUPPORTED, "num_samples 500 must be a multiple of 64 in [64, 1024]"),
    (dict(num_elites=0, simnorm_dim=4), INVALID, "num_elites 0"),
    (dict(multitask=1, episodic=1), INVALID, "multitask needs task_dim > 0"),
    (dict(iterations=0, latent_dim=4), INVALID, "iterations / max_envs must be positive"),
    (dict(path=FUSED, latent_dim=768, precision=7), UNSUPPORTED, "fused planner kernels are built for latent_dim == mlp_dim == 512 (got 768 / 512)"),
    (dict(path=9, precision=7), INVALID, "unknown path 9"),
    (dict(precision=7, mlp_dim=4128), INVALID, "unknown precision 7"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_a_refused_configuration_gets_creates_code_and_message(lib, case):
    over, code, msg = REFUSALS[case]
    with pytest.raises(lrm.Refused) as e:
        lrm.plan_layout(lib, c1(**over))
    assert e.value.args == (code, msg)


def test_the_lds_refusal_is_out_of_reach_of_an_accepted_configuration(lib):
    """create's last refusal, "LDS tile of %zu bytes exceeds 160 KiB" (fused family), cannot be tripped by a configuration that passes
    the checks in front of it: the tile is 64 rows of (512 + Apad) operands plus 8 KiB of LayerNorm scratch, 8 H A bytes of mean / std
    and 64 bytes, and action_dim <= 64, horizon <= 8 bound it by 160 832 bytes in either arithmetic.  So it has no refusal case; the
    largest tile is pinned instead, with its distance to the limit."""
    for prec in (SPLIT, FP32):
        lo = lrm.plan_layout(lib, c1(action_dim=64, horizon=8, precision=prec))
        assert lo["lds_bytes"] == 64 * 2320 + 8192 + 2 * 8 * 64 * 4 + 64 == 160832 <= 160 * 1024
    # the fp32 exception of the check before it is accepted (it is the split row kernels that hold a row in registers)
    assert lrm.plan_layout(lib, c1(mlp_dim=4128, precision=FP32))["layered"]


# ---------------------------------------------------------------------------------------------------------------- byte totals
with open(os.path.join(ROOT, "tests", "golden", "create_bytes.json")) as _f:
    RECORDED = json.load(_f)


def simulate_bytes(lib, lo, num_cus, modes):
    """tdmpc2_plan_device_bytes of a handle with this layout after create (K-split mode modes[0]) and tdmpc2_plan_set_tuning(KSPLIT,
    m) for the further modes: the table, plus per chain a K-split workspace of ksws_slots slots each time the mode wants more than
    the handle has (ksws_ensure: the smaller ones stay with the handle until destroy).  Nothing else: the unit scalar is an entry
    of the table, and the two timing buffers exist in -DGW_TIMING / -DSPLIT_TIMING builds with their variable set only."""
    total, have = sum(b for b, _ in lo["bufs"].values()), 0
    for m in modes:
        want = lib.ksws_slots_c(lo["ks_tiles"], num_cus, m)
        if want > have:
            total, have = total + want * lib.ks_slot_bytes() * (2 if lo["second_chain"] else 1), want
    return total


@pytest.mark.parametrize("row", range(len(RECORDED["rows"])))
def test_the_layout_adds_up_to_what_the_parent_allocated(lib, row):
    r = RECORDED["rows"][row]
    assert "refused" not in r and "does_not_fit" not in r  # (none of the recorded rows was; such a row would have no total)
    cus = RECORDED["num_cus"]
    lo = lrm.plan_layout(lib, native.PlanCfg(**r["cfg"]), cus)
    assert (lo["path"], lo["precision"]) == (r["path"], r["precision"])
    assert simulate_bytes(lib, lo, cus, [2]) == r["device_bytes"], (r["name"], r["max_envs"])
    assert ("device_bytes_ksplit1" in r) == bool(lo["layered"] and lo["split"])
    if "device_bytes_ksplit1" in r:
        assert simulate_bytes(lib, lo, cus, [2, 1]) == r["device_bytes_ksplit1"], (r["name"], r["max_envs"])
    assert lrm.layout_bytes(lib, lo, cus) == r["device_bytes"]


def test_the_recorded_table_has_the_rows_it_should():
    want = {(n, E, 0, 0) for n in ("c1", "c2", "c3", "c4", "c4_l1024", "mt5", "tiny", "small_ep") for E in (1, 4, 30)}
    want |= {("c1", 1, LAYERED, 0), ("c1", 1, 0, FP32), ("c3", 1, 0, FP32)}
    assert {(r["name"], r["max_envs"], r["path_arg"], r["precision_arg"]) for r in RECORDED["rows"]} == want
    assert len(RECORDED["rows"]) == len(want) and RECORDED["num_cus"] == 256
    for r in RECORDED["rows"]:  # the cfg recorded is the one NativePlanner builds today
        cname, over = ("small", dict(episodic=True)) if r["name"] == "small_ep" else (r["name"], {})
        c = named(cname, r["max_envs"], r["path_arg"], r["precision_arg"], **over)
        assert {k: getattr(c, k) for k in r["cfg"]} == r["cfg"], r["name"]


# ---------------------------------------------------------------------------------------------------------------- structure
def test_each_family_has_its_own_buffers_and_the_zeroed_ones_are_the_same(lib):
    fused = lrm.plan_layout(lib, named("c1"))
    lay = lrm.plan_layout(lib, named("c3"))
    assert (fused["path"], fused["layered"], lay["path"], lay["layered"]) == (FUSED, 0, LAYERED, 1)
    fb, lb = set(fused["bufs"]), set(lay["bufs"])
    common = {"bins", "actions", "value", "mean", "std", "ticket", "qidx_buf", "beff"}
    assert fb == common | FUSED_BUFS | CL_BUFS | CL2_BUFS
    assert lb == common | LAYERED_BUFS | SPLIT_ONLY_BUFS | SECOND_CHAIN_BUFS
    assert not fb & (LAYERED_BUFS | SPLIT_ONLY_BUFS | SECOND_CHAIN_BUFS) and not lb & (FUSED_BUFS | CL_BUFS | CL2_BUFS)
    assert {n for n, (_, z) in lay["bufs"].items() if z} == ZEROED & lb
    assert {n for n, (_, z) in fused["bufs"].items() if z} == (ZEROED - {"beff"}) & fb
    # the scalars of the other family stay zero; the error line goes with the paths that wait
    assert all(lay[k] == 0 for k in ("stride", "row_bytes", "lds_bytes", "cl_lds", "cl_max_clusters"))
    assert all(fused[k] == 0 for k in ("Kin", "Mp", "ldl", "Ppad", "ldpre", "cvec_rows", "stats_cap", "arrive_cap", "ks_tiles", "mws_cap"))
    assert fused["err_line"] and lay["err_line"] and not fused["second_chain"]


def test_one_stream_removes_the_second_chain_and_nothing_else(lib):
    for name in ("c3", "tiny", "c4"):
        for prec in (SPLIT, FP32):
            two = lrm.plan_layout(lib, named(name, precision=prec))
            one = lrm.plan_layout(lib, named(name, precision=prec), one_stream=True)
            assert two["second_chain"] and not one["second_chain"]
            gone = set(two["bufs"]) - set(one["bufs"])
            assert gone == (SECOND_CHAIN_BUFS if prec == SPLIT else {"HA2", "HB2", "LG2"}) and not set(one["bufs"]) - set(two["bufs"])
            assert all(one["bufs"][n] == two["bufs"][n] for n in one["bufs"])
            for k in lrm.LAYOUT_FIELDS:
                if k not in ("second_chain", "nbuf", "mws_cap"):
                    assert one[k] == two[k], k
            # ... and ksws2: one K-split workspace instead of two
            ks = lib.ksws_slots_c(two["ks_tiles"], 256, 1) * lib.ks_slot_bytes()
            table = lambda lo: sum(b for b, _ in lo["bufs"].values())  # noqa: E731
            assert simulate_bytes(lib, two, 256, [1]) - table(two) == 2 * ks and simulate_bytes(lib, one, 256, [1]) - table(one) == ks
    fused = lrm.plan_layout(lib, named("c1"))
    assert lrm.plan_layout(lib, named("c1"), one_stream=True) == fused  # (the switch is the layered family's)


def test_fp32_has_the_unit_scalar_and_none_of_the_split_only_buffers(lib):
    for name in ("c1", "c3", "tiny"):
        s, f = lrm.plan_layout(lib, named(name)), lrm.plan_layout(lib, named(name, precision=FP32))
        assert (s["precision"], f["precision"]) == (SPLIT, FP32) and s["path"] == f["path"]
        assert f["bufs"]["one"] == (4, False) and "one" not in s["bufs"]
        assert not set(f["bufs"]) & (SPLIT_ONLY_BUFS | CL_BUFS | CL2_BUFS)
        assert not f["err_line"] and f["ks_tiles"] == f["stats_cap"] == f["arrive_cap"] == f["cvec_rows"] == f["ldpre"] == f["cl_lds"] == 0
        assert set(s["bufs"]) - set(f["bufs"]) == (SPLIT_ONLY_BUFS if s["layered"] else CL_BUFS | CL2_BUFS)


@pytest.mark.parametrize("N,episodic,cus", [(512, 0, 256), (512, 0, 255), (512, 1, 256), (256, 0, 128), (256, 0, 127), (1024, 0, 256),
                                            (1024, 0, 512), (64, 0, 32), (64, 0, 31), (64, 0, 16), (64, 0, 15), (512, 0, 0)])
def test_the_cluster_buffers_exist_where_the_calls_fit_the_chip(lib, N, episodic, cus):
    """ks_rollout_cl: as many plans as fit the chip in one round of 8-workgroup clusters, one per 32 rows; ks_rollout_cl2: two
    clusters per 32 rows of ONE non-episodic plan -- every buffer of each or none.  (cus = 0: the runtime did not say -> 256.)"""
    lo = lrm.plan_layout(lib, c1(num_samples=N, episodic=episodic, max_envs=3), cus)
    per_env, CL, real = N // 32, 8, cus or 256
    envs = min(3, real // (per_env * CL))
    have = set(lo["bufs"])
    assert have & CL_BUFS == (CL_BUFS if envs >= 1 else set())
    assert lo["cl_max_clusters"] == envs * per_env and lo["err_line"] == (envs >= 1)
    assert have & CL2_BUFS == (CL2_BUFS if envs >= 1 and not episodic and 2 * per_env * CL <= real else set())
    if envs >= 1:
        assert lo["bufs"]["cl_flags"] == (envs * per_env * 64, True)


def test_the_few_row_workspaces_exist_on_either_side_of_their_condition(lib):
    """Two partial-sum workspaces of one 128 x 256 tile per CU, where one plan's tiles (128 rows x 8 column tiles of 32) fit the chip in
    one round and the second chain exists.  c3 at E = 1 has them (4 x 7 = 28 tiles).  On 256 CUs so does every accepted model (at most
    8 x 16 = 128 tiles: c4), so the other side is c4 (1024 rows, 4096 wide: 128 tiles) on a device of 120 CUs -- and 128 CUs is enough."""
    lo = lrm.plan_layout(lib, named("c3"))
    assert lo["mws_cap"] == 256 * 128 * 256 and lo["bufs"]["mws[0]"] == lo["bufs"]["mws[1]"] == (256 * 128 * 256 * 4, False)
    without = lrm.plan_layout(lib, named("c4"), 120)
    assert without["mws_cap"] == 0 and not {"mws[0]", "mws[1]"} & set(without["bufs"])
    edge = lrm.plan_layout(lib, named("c4"), 128)
    assert edge["mws_cap"] == 128 * 128 * 256 and {"mws[0]", "mws[1]"} <= set(edge["bufs"])
    assert lrm.plan_layout(lib, named("c4"), 127)["mws_cap"] == 0


def test_the_k_split_slot_rule(lib):
    """Mode 0 none; mode 2 at most cus / 16 (rounded up to 4) tail tiles per XCD x 8 XCDs x 4 parts; mode 1 32 tail tiles per XCD;
    never more than 4 parts of every 256 x 256 tile of the handle's largest call; none where the wide tile never applies."""
    assert [lib.ksws_slots_c(1000, 256, m) for m in (0, 1, 2)] == [0, 1024, 512]
    assert [lib.ksws_slots_c(16, 256, m) for m in (0, 1, 2)] == [0, 64, 64]
    assert [lib.ksws_slots_c(0, 256, m) for m in (0, 1, 2)] == [0, 0, 0]
    assert lib.ksws_slots_c(1000, 0, 2) == 512 and lib.ksws_slots_c(1000, 304, 2) == 8 * 20 * 4 and lib.ksws_slots_c(1000, 64, 2) == 128
    assert lrm.plan_layout(lib, named("tiny"))["ks_tiles"] == 0                     # 2 column tiles: no wide tile
    assert lrm.plan_layout(lib, named("c3"))["ks_tiles"] == 2 * 7                   # 512 rows x 56 column tiles
    assert lrm.plan_layout(lib, named("c3", 3))["ks_tiles"] == 6 * 7
    assert lrm.plan_layout(lib, c1(path=LAYERED, num_samples=128))["ks_tiles"] == 0  # 128 rows: not a whole 256-row tile


# ---------------------------------------------------------------------------------------------------------------- on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "c1", "c3"])
def test_create_allocates_what_the_layout_says(lib, name):
    """tdmpc2_plan_device_bytes right after create == the layout's total for the device's real CU count (nothing is launched)."""
    import torch

    cfg = named_config(name)
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    p = native.NativePlanner(cfg, planner_iterations(cfg), torch.device("cuda", 0), max_envs=1)
    try:
        lo = lrm.plan_layout(lib, native.plan_cfg(cfg, planner_iterations(cfg), 1), cus)
        assert (p.path, p.precision) == (lo["path"], lo["precision"])
        assert p.device_bytes == lrm.layout_bytes(lib, lo, cus)
    finally:
        p.close()
