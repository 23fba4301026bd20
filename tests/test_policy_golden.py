"""CPU: the PyTorch-ROCm WorldModel.encode / WorldModel.pi (tdmpc2_amd/world_model.py) against the reference's own outputs in
tests/golden/policy.npz (tools/make_policy_golden.py) -- including info['entropy'] and info['scaled_entropy'] -- and the fixture
against a fresh run of the reference where its tree is present.

Gates: z, mean, action, log_std within 1e-5 (the encoder's Z_GATE).  entropy and scaled_entropy are ill-conditioned where tanh
saturates (log(relu(1 - tanh^2) + 1e-6) amplifies fp32 round-off), so each row is gated at max(1e-5 x max(1, |v|), 2 x |reference
fp32 - fp64|), with the fp64 value evaluated from the reference's formula on the fixture's inputs (tests/policy_common.py); the
1e-5 floor is relative because these sums of A terms reach a few thousand, where fp32's own spacing exceeds 1e-5."""
import numpy as np
import pytest
import torch

from tests import policy_common as pc


def _world_model(name):
    from oracle import cases
    from tdmpc2_amd import checkpoint
    from tdmpc2_amd.world_model import WorldModel

    c = cases.build_case(name)
    wm = WorldModel(c["cfg"]).eval()
    wm.load_state_dict(checkpoint.convert_state_dict({k: torch.as_tensor(v) for k, v in c["sd"].items()}))
    return c, wm


@pytest.mark.parametrize("name", pc.CASES)
def test_world_model_pi_matches_reference_golden(name, monkeypatch):
    c, wm = _world_model(name)
    g = pc.golden(name)
    task = None if g["tasks"] is None else torch.as_tensor(g["tasks"])
    monkeypatch.setattr(torch, "randn_like", lambda x, **kw: torch.as_tensor(g["eps"]).to(x.dtype).clone())
    with torch.no_grad():
        z = wm.encode(torch.as_tensor(g["obs"]), task)
        action, info = wm.pi(torch.as_tensor(g["z"]), task)
    assert np.abs(z.numpy() - g["z"]).max() <= pc.GATE
    for key, got in (("action", action), ("mean", info["mean"]), ("log_std", info["log_std"])):
        assert np.abs(got.numpy() - g[key]).max() <= pc.GATE, key
    assert info["action_prob"] == 1.0
    g64 = pc.fp64_pi(c["cfg"], c["sd"], g["z"], g["tasks"], g["eps"])
    for key in ("entropy", "scaled_entropy"):
        assert tuple(info[key].shape) == (len(g["z"]), 1), key
        err = np.abs(info[key].numpy().reshape(-1) - g[key].reshape(-1))
        assert (err <= pc.entropy_bound(g64, g, key)).all(), (key, err)
    if g["tasks"] is not None:  # rows of different tasks: masked action dimensions are exactly 0
        _, mask = pc.task_rows(c["sd"], g["tasks"])
        assert len({int(m.sum()) for m in mask}) > 1
        assert (g["action"][mask == 0] == 0).all() and (info["mean"].numpy()[mask == 0] == 0).all()


def test_fixture_regenerates_bit_for_bit():
    from oracle import ref_runner

    if not ref_runner.available():
        pytest.skip("the reference tree is not available here")
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("make_policy_golden", os.path.join(os.path.dirname(os.path.dirname(pc.GOLDEN_DIR)), "tools",
                                                  "make_policy_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    threads = torch.get_num_threads()
    try:
        fresh = gen.generate()
    finally:
        torch.set_num_threads(threads)
    stored = dict(np.load(os.path.join(pc.GOLDEN_DIR, "policy.npz")))
    assert sorted(fresh) == sorted(stored)
    for k in stored:
        assert fresh[k].dtype == stored[k].dtype and np.array_equal(fresh[k], stored[k]), k
