"""-m gpu: `native_pixel_grad` -- WorldModel.encode of an rgb model through the pixel-gradient unit (autograd.pixel_encode).
The c1-sized rgb agent of tests/test_gpu_pixel_training.py (B 2, H 3, C 32, cin 9).  pixel_encode's gradients are the unit's, called by
hand, bit for bit; flag on and off advance the generator alike; the gradient of a fixed readout follows the fp64 module within the
measured gate of tests/test_gpu_pixel_grad.py; one `_update` step with the flag on follows the step with it off; with the flag off
`encode` is the module."""
import numpy as np
import pytest
import torch

from tests import model_common as mc
from tests import pixel_common as pc
from tests import pixel_grad_common as pg
from tests.test_gpu_layer_grad import FLOOR, MARGIN
from tests.test_gpu_pixel_training import B, C, CIN, H, _agent, _batch, _dev

pytestmark = pytest.mark.gpu
CONVS = (2, 4, 6, 8)
# test_gradient_follows_the_fp64_module: under torch.manual_seed(SEED) ShiftAug draws (dx, dy) = (3, 1), (0, 6) for the two images;
# OBS_SEED is the first observation seed for which, with those shifts and the agent's encoder weights, no pre-activation of a ReLU
# lies within 2^-16 max |pre| of zero (found by a search in fp64 on the CPU; the test asserts it before it compares anything)
SEED, OBS_SEED = 7, 18


def _params(seq):
    return [t for i in CONVS for t in (seq[i].weight, seq[i].bias)]


def test_pixel_encode_is_the_unit_called_by_hand():
    from tdmpc2_amd import autograd, native

    agent = _agent(native=False)
    seq = agent.model._encoder["rgb"]
    obs = _batch(agent.cfg)["obs"].reshape((H + 1) * B, CIN, 64, 64).contiguous()
    n = obs.shape[0]
    torch.manual_seed(3)
    shift = torch.cat([native.NativePlanner.draw_shift(B, _dev()) for _ in range(H + 1)])
    G = torch.randn(n, 16 * C, device=_dev())
    before = native.PIXEL_GRAD_CALLS
    z = autograd.pixel_encode(seq, obs, shift)
    assert z.requires_grad and native.PIXEL_GRAD_CALLS == before + 1
    (z * G).sum().backward()
    assert native.PIXEL_GRAD_CALLS == before + 2
    got = [p.grad.clone() for p in _params(seq)]
    # by hand
    desc = native.pixgrad_desc(n, CIN, C, 0)
    ab, fb, bb = native.pixgrad_workspace_bytes(desc)
    mk = lambda nbytes: torch.empty(nbytes // 4, dtype=torch.float32, device=_dev())  # noqa: E731
    acts, fwd_ws, bwd_ws = mk(ab), mk(fb), mk(bb)
    Ws, bs = [seq[i].weight.detach() for i in CONVS], [seq[i].bias.detach() for i in CONVS]
    tab = native.pixgrad_shift_table(_dev())
    native.pixgrad_forward(desc, obs, shift, tab, Ws, bs, fwd_ws, acts)
    assert torch.equal(z.detach(), acts[n * 1046 * C:].view(n, 16 * C))
    dW, db = [torch.empty_like(w) for w in Ws], [torch.empty_like(b) for b in bs]
    native.pixgrad_backward(desc, obs, shift, tab, Ws, acts, G, bwd_ws, dW, db)
    for l in range(4):
        assert torch.equal(got[2 * l], dW[l]) and torch.equal(got[2 * l + 1], db[l]), l
    # under no_grad: nothing saved, passes over one scratch buffer, the bits of one pass
    with torch.no_grad():
        for pass_images in (256, 3, 1):
            zz = autograd.pixel_encode(seq, obs, shift, pass_images=pass_images)
            assert not zz.requires_grad and torch.equal(zz, z.detach()), pass_images
    # only the layers that need a gradient are asked for
    for p in _params(seq):
        p.grad = None
    seq[2].weight.requires_grad_(False)
    seq[2].bias.requires_grad_(False)
    (autograd.pixel_encode(seq, obs, shift) * G).sum().backward()
    assert seq[2].weight.grad is None and torch.equal(seq[4].weight.grad, dW[1]) and torch.equal(seq[8].bias.grad, db[3])


def test_flag_on_and_off_advance_the_generator_alike_and_off_is_the_module():
    on, off = _agent(native=False), _agent(native=False)
    on.native_pixel_grad = True
    assert on.model.native_pixel_grad and not off.native_pixel_grad
    obs = _batch(on.cfg)["obs"]
    for x in (obs, obs[0]):   # the 5-D sequence branch and a single batch
        torch.manual_seed(SEED)
        with torch.no_grad():
            z_on = on.model.encode(x, None)
        s_on = torch.cuda.get_rng_state(_dev())
        torch.manual_seed(SEED)
        with torch.no_grad():
            z_off = off.model.encode(x, None)
        assert torch.equal(torch.cuda.get_rng_state(_dev()), s_on)
        torch.manual_seed(SEED)
        with torch.no_grad():
            want = torch.stack([off.model._encoder["rgb"](o) for o in x]) if x.ndim == 5 else off.model._encoder["rgb"](x)
        assert torch.equal(z_off, want)                      # flag off: the parent's path, bit for bit
        assert z_on.shape == z_off.shape and float((z_on - z_off).abs().max()) <= 1e-5   # same shifts: the encoder gate of the suite


def test_gradient_follows_the_fp64_module():
    from tdmpc2_amd import native

    agent = _agent(native=False)
    agent.native_pixel_grad = True
    seq = agent.model._encoder["rgb"]
    obs = torch.randint(0, 256, (B, CIN, 64, 64), generator=torch.Generator().manual_seed(OBS_SEED), dtype=torch.uint8).to(_dev())
    g = torch.Generator().manual_seed(2)
    G = torch.randn(B, 16 * C, generator=g, dtype=torch.float64)
    torch.manual_seed(SEED)
    shifts = [tuple(int(v) for v in r) for r in native.NativePlanner.draw_shift(B, _dev()).cpu()]
    case = dict(obs=obs.cpu(), shifts=shifts, C=C, cin=CIN, stack=True, Ws=[seq[i].weight.detach().cpu() for i in CONVS],
                Bs=[seq[i].bias.detach().cpu() for i in CONVS])
    # the fp64 module after ShiftAug on the table-resampled frames, with every pre-activation kept
    m = pc.module(case, torch.float64)
    x = torch.stack([pc.resample64(img, dx, dy)[0] for img, (dx, dy) in zip(case["obs"], shifts)])
    pres = {}
    for i in range(1, len(m)):
        x = m[i](x)
        if i in CONVS:
            pres[i] = x.detach()
    for i in CONVS[:3]:   # SEED / OBS_SEED are chosen so that this holds: no ReLU of the fp32 side can open or close differently
        assert float(pres[i].abs().min()) > 2.0 ** -16 * float(pres[i].abs().max()), i
    (x * G).sum().backward()
    ref = [t.grad for i in CONVS for t in (m[i].weight, m[i].bias)]
    # torch CPU fp32 autograd of the same tail, as the yardstick
    m32 = pc.module(case, torch.float32)
    y = torch.stack([pc.resample64(img, dx, dy)[0] for img, (dx, dy) in zip(case["obs"], shifts)]).float()
    for i in range(1, len(m32)):
        y = m32[i](y)
    (y * G.float()).sum().backward()
    yard = [t.grad for i in CONVS for t in (m32[i].weight, m32[i].bias)]
    torch.manual_seed(SEED)
    z = agent.model.encode(obs, None)
    (z * G.float().to(_dev())).sum().backward()
    ratios = {}
    for k, (p, r, t) in enumerate(zip(_params(seq), ref, yard)):
        ratios[f"{'dW' if k % 2 == 0 else 'db'}{k // 2}"] = pg.rel_err(p.grad.cpu(), r) / max(pg.rel_err(t, r), FLOOR)
    print({k: round(v, 2) for k, v in ratios.items()})
    for k, r in ratios.items():
        assert r <= MARGIN, (k, r)


def test_one_update_step_follows_the_flag_off_step():
    on, off = _agent(native=False), _agent(native=False)
    infos = []
    for agent, flag in ((on, True), (off, False)):
        agent.native_autograd = True
        agent.native_pixel_grad = flag
        b = _batch(agent.cfg)
        before = [p.detach().clone() for p in _params(agent.model._encoder["rgb"])]
        g = torch.Generator().manual_seed(21)
        pins = dict(td_pi_eps=b["pi_eps"], td_qidx=b["qidx"], qidx=b["qidx"].long(),
                    pi_eps=torch.randn(H + 1, B, agent.cfg.action_dim, generator=g).to(_dev()))
        torch.manual_seed(SEED)   # the ShiftAug draws of both sides
        info = agent._update(b["obs"], b["action"], b["reward"], None, None, pins=pins)
        infos.append({k: float(v) for k, v in info.items()})
        for p, q in zip(_params(agent.model._encoder["rgb"]), before):
            assert torch.isfinite(p).all() and not torch.equal(p.detach(), q)
    a, m = infos
    assert set(a) == set(m) and "grad_norm" in a
    got, want = np.array([a[k] for k in sorted(a)]), np.array([m[k] for k in sorted(a)])
    print(dict(zip(sorted(a), zip(got, want))))
    assert np.isfinite(got).all()
    assert (np.abs(got - want) <= mc.tol(want, 0.0)).all(), dict(zip(sorted(a), np.abs(got - want)))
    assert (np.abs(got - want) <= mc.RTOL * np.maximum(1, np.abs(want))).all()
