"""-m gpu: rgb training batches in the library.  With `native_pixel_encoder`, TDMPC2.model_losses / update_info encode the
(H + 1) B frame stacks with one tdmpc2_plan_encode_pix_batch call.  The wiring is exact (the same latents and the same calls as
encoding by hand), the result follows the PyTorch-ROCm module branch under one seed (same ShiftAug draws), update_info returns
the reference's keys, and a batch larger than the reserved chunk gives the bits of one pass.
TDMPC2_PIXEL_BATCH_JSON=<file>: the observed differences against the module branch are merged into that file."""
import numpy as np
import pytest
import torch

from tests import model_common as mc
from tests.test_gpu_pixel_batch import record
from tests.test_gpu_pixel_encoder import Z_GATE

pytestmark = pytest.mark.gpu

LOSS_KEYS = ("consistency_loss", "reward_loss", "value_loss", "termination_loss", "total_loss")
B, H, C, CIN = 2, 3, 32, 9


def _dev():
    return torch.device("cuda", 0)


def _agent(episodic=False, native=True):
    """c1-sized rgb agent: synthetic weights (tdmpc2_amd.synth) under the default-initialised conv encoder."""
    from tdmpc2_amd import synth
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.tdmpc2 import TDMPC2

    cfg = named_config("c1", episodic=episodic, horizon=H)
    cfg.latent_dim, cfg.num_channels, cfg.obs = 16 * C, C, "rgb"
    cfg.obs_shape = {"rgb": (CIN, 64, 64)}
    torch.manual_seed(0)
    agent = TDMPC2(cfg, device=_dev())
    sd = agent.model.state_dict()
    scfg = cfg.replace()
    scfg.obs_shape = {"state": (17,)}  # (synth sizes a state encoder as well; its keys are not this model's and are skipped)
    for k, v in synth.make_state_dict(scfg, 0).items():
        if k in sd and torch.is_tensor(sd[k]) and tuple(sd[k].shape) == tuple(v.shape):
            sd[k] = torch.as_tensor(v)
    agent.load({"model": sd})
    agent.native_pixel_encoder = native
    return agent


def _batch(cfg):
    g = torch.Generator().manual_seed(11)
    rng = np.random.default_rng(12)
    obs = torch.randint(0, 256, (H + 1, B, CIN, 64, 64), generator=g, dtype=torch.uint8).to(_dev())
    d = lambda a: torch.as_tensor(a).to(_dev())
    return dict(obs=obs, action=d(rng.uniform(-1, 1, (H, B, cfg.action_dim)).astype(np.float32)),
                reward=d(rng.standard_normal((H, B, 1)).astype(np.float32)),
                terminated=d((rng.random((H, B, 1)) < 0.2).astype(np.float32)),
                pi_eps=d(rng.standard_normal((H, B, cfg.action_dim)).astype(np.float32)),
                qidx=d(np.array([min(3, cfg.num_q - 1), 1], np.int32)))


def _losses(agent, b, seed=7):
    torch.manual_seed(seed)
    return agent.model_losses(b["obs"], b["action"], b["reward"], b["terminated"], None, pi_eps=b["pi_eps"], qidx=b["qidx"], want=("zs",))


def test_wiring_is_exact():
    agent = _agent()
    b = _batch(agent.cfg)
    res = _losses(agent, b)
    planner = agent.planner()
    assert planner.pix_batch_chunk == agent.pixel_batch_images == 256
    # by hand: the shifts drawn per time step, one encode_pix_batch call, then the same two library calls with the same pins
    torch.manual_seed(7)
    shift = torch.cat([planner.draw_shift(B, _dev()) for _ in range(H + 1)])
    z = planner.encode_pix_batch(b["obs"].reshape((H + 1) * B, CIN, 64, 64).contiguous(), shift).reshape(H + 1, B, -1)
    z0, next_z = z[0], z[1:].contiguous()
    td = agent._td_target(next_z, b["reward"], b["terminated"], None, pi_eps=b["pi_eps"], qidx=b["qidx"])
    want = agent.model_losses_latent(z0, next_z, b["action"], b["reward"], td, b["terminated"], None, want=("zs",))
    assert torch.isfinite(res["zs"]).all() and torch.equal(res["zs"], want["zs"]) and torch.equal(res["zs"][0], z0)
    assert torch.equal(res["td_targets"], td)
    for k in LOSS_KEYS:
        assert torch.equal(res[k], want[k]), k


def test_follows_the_module_branch_under_one_seed():
    nat, ref = _agent(native=True), _agent(native=False)
    assert nat.native_pixel_encoder and not ref.native_pixel_encoder
    b = _batch(nat.cfg)
    a = _losses(nat, b)
    s_nat = torch.cuda.get_rng_state(_dev())
    m = _losses(ref, b)
    assert torch.equal(torch.cuda.get_rng_state(_dev()), s_nat)  # both branches advance the generator alike
    dz = (a["zs"][0] - m["zs"][0]).abs().max().item()
    td_a, td_m = a["td_targets"].cpu().numpy().reshape(-1), m["td_targets"].cpu().numpy().reshape(-1)
    dtd = (np.abs(td_a - td_m) / np.maximum(1, np.abs(td_m))).max()
    got, want = np.array([float(a[k]) for k in LOSS_KEYS]), np.array([float(m[k]) for k in LOSS_KEYS])
    print(f"z0 max |diff| {dz:.3e}; td rel {dtd:.3e}; losses {got} vs {want}")
    record({"model_losses_native_vs_module": {"z0_max_abs": dz, "td_targets_max_rel": float(dtd),
                                              **{k: float(abs(x - y)) for k, x, y in zip(LOSS_KEYS, got, want)}}})
    assert dz <= Z_GATE
    # the tolerances tests/test_gpu_model.py::test_model_losses_from_observations holds the same quantities to (no fp64 distance
    # of a reference enters here: both sides are this package)
    assert dtd <= mc.RTOL
    assert (np.abs(got - want) <= mc.tol(want, 0.0)).all()


@pytest.mark.parametrize("episodic", [False, True], ids=["plain", "episodic"])
def test_update_info_keys(episodic):
    agent = _agent(episodic=episodic)
    b = _batch(agent.cfg)
    torch.manual_seed(3)
    info = agent.update_info(b["obs"], b["action"], b["reward"], b["terminated"] if episodic else None, None)
    keys = {"consistency_loss", "reward_loss", "value_loss", "termination_loss", "total_loss", "pi_loss", "pi_entropy",
            "pi_scaled_entropy", "pi_scale"}
    if episodic:
        keys |= {"termination_rate", "termination_f1"}
    assert set(info) == keys
    assert all(v.dim() == 0 and np.isfinite(float(v)) for v in info.values())


def test_a_batch_larger_than_the_chunk():
    one, passes = _agent(), _agent()
    passes.pixel_batch_images = 4  # 8 frames: two passes
    b = _batch(one.cfg)
    a, c = _losses(one, b), _losses(passes, b)
    assert passes.planner().pix_batch_chunk == 4 and one.planner().pix_batch_chunk == 256
    assert torch.equal(a["zs"], c["zs"]) and torch.equal(a["td_targets"], c["td_targets"])
    for k in LOSS_KEYS:
        assert torch.equal(a[k], c[k]), k
