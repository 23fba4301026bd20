"""GPU: the pixel-observation encoder in HIP (tdmpc2_plan_bind_pixel_encoder / encode_pix / run_pix, pixel_kernels.cuh)
against the reference's own conv output, against the pinned PyTorch module on both sides of the route threshold, plan_pix
against plan(encode_pix(obs)), the agent's native_pixel_encoder route, a captured hipGraph, and the refusals."""
import numpy as np
import pytest
import torch

from tests.helpers import ACT_ATOL

pytestmark = pytest.mark.gpu
Z_GATE = 1e-5


def _dev():
    return torch.device("cuda", 0)


def _cfg(C, **over):
    from tdmpc2_amd.config import named_config

    cfg = named_config("c1", **over)
    cfg.latent_dim, cfg.num_channels = 16 * C, C  # 32: the 5M model (fused family); 16: a 256-wide latent (layered family)
    cfg.obs = "rgb"
    return cfg


def _planner(cfg, max_envs, seed=0):
    from tdmpc2_amd import synth
    from tdmpc2_amd.native import NativePlanner

    p = NativePlanner(cfg, cfg.iterations, _dev(), max_envs=max_envs)
    p.bind_state_dict({k: torch.as_tensor(v) for k, v in synth.make_state_dict(cfg, seed).items()})
    return p


def _conv(cin, C, seed):
    from tdmpc2_amd import layers

    torch.manual_seed(seed)
    m = layers.conv((cin, 64, 64), C, act=layers.SimNorm(8)).to(_dev()).eval()
    return m, {f"_encoder.rgb.{k}": v for k, v in m.state_dict().items()}


def test_encode_pix_matches_the_reference_conv_output():
    from oracle import make_golden_host as mg
    from tdmpc2_amd.native import NativePlanner
    from tests.helpers import GOLDEN_DIR

    g = np.load(f"{GOLDEN_DIR}/pixel_modules.npz")
    sd = {f"_encoder.rgb.{k}": torch.as_tensor(np.asarray(v)).float() for k, v in mg.conv_state(g).items()}
    x = mg.pixel_input()
    torch.manual_seed(mg.CONV_SEED)
    shift = NativePlanner.draw_shift(2, "cpu")  # the draw the reference's ShiftAug made on the CPU
    p = _planner(_cfg(32), 2)
    p.bind_pixel_encoder(sd)
    z = p.encode_pix(x.to(_dev()).contiguous(), shift.to(_dev()))
    err = (z.cpu() - torch.as_tensor(g["conv"])).abs().max().item()
    assert err <= Z_GATE, err


@pytest.mark.parametrize("C", [32, 16])
@pytest.mark.parametrize("cin", [9, 3])
def test_encode_pix_matches_the_torch_module(C, cin):
    from tdmpc2_amd.native import NativePlanner

    m, sd = _conv(cin, C, seed=C + cin)
    p = _planner(_cfg(C), 256)
    p.bind_pixel_encoder(sd)
    for E in (1, 2, 7, 64, 256):
        x8 = torch.randint(0, 256, (E, cin, 64, 64), device=_dev(), dtype=torch.uint8)
        torch.manual_seed(E)
        with torch.no_grad():
            ref = m(x8.float())
        torch.manual_seed(E)
        shift = NativePlanner.draw_shift(E, _dev())
        for obs in (x8, x8.float()):
            z = p.encode_pix(obs, shift)
            err = (z - ref).abs().max().item()
            assert err <= Z_GATE, (E, obs.dtype, err)


@pytest.mark.parametrize("C", [32, 16])
@pytest.mark.parametrize("E", [1, 4])
@pytest.mark.parametrize("tape", [False, True])
def test_plan_pix_equals_plan_of_encode_pix(C, E, tape):
    cfg = _cfg(C)
    _, sd = _conv(9, C, seed=7)
    obs = torch.randint(0, 256, (E, 9, 64, 64), device=_dev(), dtype=torch.uint8)
    shift = torch.randint(0, 7, (E, 2), device=_dev(), dtype=torch.int32)
    disc = torch.tensor([[0.99 ** h for h in range(cfg.horizon + 1)]] * E, device=_dev(), dtype=torch.float32)
    t0 = torch.ones(E, dtype=torch.uint8, device=_dev())
    outs = []
    for fused in (True, False):  # fresh handles: the same call counter, hence the same Philox draws
        p = _planner(cfg, E)
        p.bind_pixel_encoder(sd)
        kw = dict(tape=p.export_noise(seed=3, call=p.call_counter(), n_envs=E)) if tape else {}
        prev = torch.zeros(E, cfg.horizon, cfg.action_dim, device=_dev())
        if fused:
            a = p.plan_pix(obs, shift, disc, prev, t0, seed=11, **kw)
        else:
            z = p.encode_pix(obs, shift)
            a = p.plan(z, disc, prev, t0, seed=11, **kw)
        torch.cuda.synchronize()
        outs.append((a.clone(), prev.clone()))
    assert torch.isfinite(outs[0][0]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _agents():
    from tdmpc2_amd.tdmpc2 import TDMPC2

    out = []
    for native in (True, False):
        cfg = _cfg(32)
        cfg.obs_shape = {"rgb": (9, 64, 64)}
        torch.manual_seed(0)
        agent = TDMPC2(cfg, device=_dev())
        for prm in agent.model._reward[2].parameters():
            torch.nn.init.normal_(prm, std=0.05)
        agent.native_pixel_encoder = native
        agent.sync_planner_weights()
        out.append(agent)
    return out


def test_agent_native_pixel_route_follows_the_torch_route():
    from tdmpc2_amd.native import NativePlanner

    nat, ref = _agents()
    assert not ref.native_pixel_encoder  # the default stays the PyTorch module
    g = torch.Generator().manual_seed(5)
    frames = [torch.randint(0, 256, (9, 64, 64), generator=g, dtype=torch.uint8) for _ in range(8)]
    # latents: the library's encoder vs the module, same shifts
    nat.planner()
    torch.manual_seed(1)
    shift = NativePlanner.draw_shift(1, _dev())
    z_nat = nat.planner().encode_pix(frames[0].to(_dev()).unsqueeze(0).contiguous(), shift)
    torch.manual_seed(1)
    with torch.no_grad():
        z_ref = ref.model.encode(frames[0].to(_dev()).unsqueeze(0), None)
    assert (z_nat - z_ref).abs().max().item() <= Z_GATE
    # an 8-step act() loop: same device RNG state after every step, actions within the suite's gate
    for step, obs in enumerate(frames):
        torch.manual_seed(100 + step)
        a = nat.act(obs, t0=step == 0)
        s_nat = torch.cuda.get_rng_state(_dev())
        torch.manual_seed(100 + step)
        b = ref.act(obs, t0=step == 0)
        s_ref = torch.cuda.get_rng_state(_dev())
        assert torch.equal(s_nat, s_ref), step
        assert (a - b).abs().max().item() <= ACT_ATOL, (step, a.tolist(), b.tolist())


def test_run_pix_replays_from_a_hip_graph():
    cfg = _cfg(32)
    _, sd = _conv(9, 32, seed=2)
    p = _planner(cfg, 2)
    p.bind_pixel_encoder(sd)
    E = 2
    obs = torch.randint(0, 256, (E, 9, 64, 64), device=_dev(), dtype=torch.uint8)
    shift = torch.randint(0, 7, (E, 2), device=_dev(), dtype=torch.int32)
    disc = torch.tensor([[0.99 ** h for h in range(cfg.horizon + 1)]] * E, device=_dev(), dtype=torch.float32)
    t0 = torch.ones(E, dtype=torch.uint8, device=_dev())
    tape = p.export_noise(seed=1, call=0, n_envs=E)
    prev0 = torch.zeros(E, cfg.horizon, cfg.action_dim, device=_dev())
    pm_eager = prev0.clone()
    a_eager = p.plan_pix(obs, shift, disc, pm_eager, t0, tape=tape).clone()
    pm_static, out = prev0.clone(), torch.empty_like(a_eager)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        p.plan_pix(obs, shift, disc, pm_static.clone(), t0, tape=tape, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        p.plan_pix(obs, shift, disc, pm_static, t0, tape=tape, out=out)
    for _ in range(2):
        pm_static.copy_(prev0)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a_eager) and torch.equal(pm_static, pm_eager)


def test_pixel_encoder_refusals_and_shift_clamping():
    from tdmpc2_amd.config import named_config
    from tdmpc2_amd.native import NativeError, NativePlanner

    _, sd = _conv(9, 32, seed=4)
    # run before bind
    p = _planner(_cfg(32), 2)
    obs = torch.randint(0, 256, (2, 9, 64, 64), device=_dev(), dtype=torch.uint8)
    shift = torch.full((2, 2), 6, device=_dev(), dtype=torch.int32)
    p.pix_channels = 9  # get past the binding's own check: the library must refuse
    with pytest.raises(NativeError, match="no pixel encoder bound"):
        p.encode_pix(obs, shift)
    p.pix_channels = None
    # multitask handle
    mt = NativePlanner(named_config("mt5"), 6, _dev(), max_envs=1)
    with pytest.raises(NativeError, match="single-task"):
        mt.bind_pixel_encoder(sd)
    # 16 C != latent_dim
    with pytest.raises(NativeError, match="latent_dim"):
        _planner(_cfg(16), 1).bind_pixel_encoder(sd)
    # wrong kernel size
    bad = dict(sd)
    bad["_encoder.rgb.4.weight"] = torch.zeros(32, 32, 3, 3, device=_dev())
    with pytest.raises(NativeError, match="kernel"):
        _planner(_cfg(32), 1).bind_pixel_encoder(bad)
    # Cin mismatch between the bound layer 0 and the call
    p.bind_pixel_encoder(sd)
    lib = p.lib
    z = torch.empty(2, 512, device=_dev())
    assert lib.tdmpc2_plan_encode_pix(p._h, 2, obs.data_ptr(), 0, 3, shift.data_ptr(), z.data_ptr(), p._stream()) == 1
    assert b"channels" in lib.tdmpc2_last_error()
    # clamping: a shift of 9 is a shift of 6
    z6 = p.encode_pix(obs, shift).clone()
    z9 = p.encode_pix(obs, torch.full((2, 2), 9, device=_dev(), dtype=torch.int32))
    assert torch.equal(z6, z9)
