"""-m gpu: the replay buffer (tdmpc2_buffer_*, tdmpc2_amd.Buffer) against the plain-Python restatement of tests/buffer_common.py,
byte for byte: every access width, packed and split rows, wrap and eviction, bulk load, hipGraph replays, and update_info on a
sampled batch against update_info on the same batch gathered with torch indexing."""
import numpy as np
import pytest
import torch

from tests import buffer_common as bc
from tests.gpu_common import dev

pytestmark = pytest.mark.gpu


def _native(cap, S, fields, max_batch=0):
    from tdmpc2_amd.native import NativeBuffer

    return NativeBuffer(cap, S, fields, dev(), max_batch=max_batch)


def _episode(rng, fields, T):
    return [rng.integers(0, 256, (T, rb), dtype=np.uint8) for rb, _, _ in fields]


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev())


def _add(nat, ref, rows):
    nat.add([_t(r) for r in rows])
    ref.add(rows)


def _outs(fields, B, fill=0):
    return [torch.full((sc, B, rb), fill, dtype=torch.uint8, device=dev()) for rb, _, sc in fields]


def _sample(nat, fields, B, seed, outs=None):
    outs = _outs(fields, B) if outs is None else outs
    idx = torch.full((B,), -7, dtype=torch.int64, device=dev())
    nat.sample(outs, seed=seed, index_out=idx)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], idx.cpu().numpy()


def _same(got, want):
    (go, gi), (wo, wi) = got, want
    assert np.array_equal(gi, wi), (gi, wi)
    for f, (a, b) in enumerate(zip(go, wo)):
        assert a.shape == b.shape and np.array_equal(a, b), f"field {f}"


def _fields(S):
    H = S - 1
    # obs 20 B (4-byte path), wide obs 96 B (16-byte path), action 12 B, reward 4 B, terminated 4 B, int64 task 8 B, 3 B (byte path)
    return [(20, 0, S), (96, 0, S), (12, 1, H), (4, 1, H), (4, 1, H), (8, 0, 1), (3, 0, S)]


@pytest.mark.parametrize("B", [1, 8, 257])
@pytest.mark.parametrize("H", [1, 3])
def test_samples_equal_the_restatement_byte_for_byte(H, B):
    S = H + 1
    fields = _fields(S)
    nat, ref = _native(64, S, fields, max_batch=257), bc.RefBuffer(64, S, fields)
    rng = np.random.default_rng(10 * H + B)
    for T in (S, S - 1, S + 1, 7, 1):  # the S - 1 and 1-step episodes occupy storage and are never sampled
        _add(nat, ref, _episode(rng, fields, T))
    assert nat.stats() == ref.stats()
    assert len(ref.eligible()) == 3
    live = set()
    for first, n in ref.eligible():
        live |= set(range(first, first + n - S + 1))
    for call in range(2):
        got, want = _sample(nat, fields, B, seed=1234 + H), ref.sample(B, 1234 + H)
        _same(got, want)
        assert set(got[1]) <= live
    assert nat.stats() == ref.stats() and ref.call == 2


def test_misaligned_outputs_take_the_narrower_paths():
    S, B = 4, 8
    fields = [(96, 0, S), (96, 0, S), (96, 0, S)]
    nat, ref = _native(32, S, fields), bc.RefBuffer(32, S, fields)
    rng = np.random.default_rng(3)
    for T in (9, 5, 12):
        _add(nat, ref, _episode(rng, fields, T))
    n = S * B * 96
    raw = [torch.zeros(n + 32, dtype=torch.uint8, device=dev()) for _ in fields]
    assert all(r.data_ptr() % 16 == 0 for r in raw)
    outs = [r[off:off + n].view(S, B, 96) for r, off in zip(raw, (16, 4, 1))]  # 16-byte, 4-byte and byte accesses
    got = _sample(nat, fields, B, 5, outs)
    _same(got, ref.sample(B, 5))
    for r, off in zip(raw, (16, 4, 1)):  # nothing written outside the output
        assert int(r[:off].sum()) == 0 and int(r[off + n:].sum()) == 0


def test_frame_stacks_are_split_over_workgroups():
    S, B = 4, 2
    fields = [(9 * 64 * 64, 0, S), (4, 1, S - 1)]
    nat, ref = _native(16, S, fields), bc.RefBuffer(16, S, fields)
    rng = np.random.default_rng(4)
    for T in (7, 6, 5):  # the third wraps and evicts the front of the first
        _add(nat, ref, _episode(rng, fields, T))
    assert nat.stats() == ref.stats()
    for _ in range(2):
        _same(_sample(nat, fields, B, 99), ref.sample(B, 99))


def test_wrap_and_eviction():
    cap, S, B = 10, 4, 8
    fields = [(20, 0, S), (4, 1, S - 1)]
    nat, ref = _native(cap, S, fields), bc.RefBuffer(cap, S, fields)
    rng = np.random.default_rng(6)
    _add(nat, ref, _episode(rng, fields, 6))
    assert nat.stats() == ref.stats()
    _add(nat, ref, _episode(rng, fields, 6))  # wraps physically; the first keeps 4 live steps: exactly one start
    assert nat.stats() == ref.stats() and ref.eligible() == [(2, 4), (6, 6)]
    # a seed (chosen here, on the CPU) whose first call draws a slice that spans the physical end: logical 7..10 or 8..11
    seed = next(s for s in range(1000) if set(ref.starts(B, s, call=0)[0]) & {7, 8} and 2 in ref.starts(B, s, call=0)[0])
    got = _sample(nat, fields, B, seed)
    _same(got, ref.sample(B, seed))
    assert set(got[1]) & {7, 8} and 2 in got[1]
    _add(nat, ref, _episode(rng, fields, 1))  # one more step pops the first episode
    assert nat.stats() == ref.stats() and ref.eligible() == [(6, 6)]
    got = _sample(nat, fields, B, seed)
    _same(got, ref.sample(B, seed))
    assert set(got[1]) <= {6, 7, 8}


def test_refusals_on_a_live_handle():
    from tdmpc2_amd.native import NativeError

    fields = [(4, 0, 4)]
    nat = _native(10, 4, fields, max_batch=8)
    with pytest.raises(NativeError, match="no episode"):
        nat.sample(_outs(fields, 2))
    with pytest.raises(NativeError, match="longer than the capacity"):
        nat.add([torch.zeros(11, 4, dtype=torch.uint8, device=dev())])
    nat.add([torch.zeros(3, 4, dtype=torch.uint8, device=dev())])  # shorter than a slice: stored, not eligible
    assert nat.stats()["num_eps"] == 1
    with pytest.raises(NativeError, match="no episode"):
        nat.sample(_outs(fields, 2))
    nat.add([torch.zeros(4, 4, dtype=torch.uint8, device=dev())])
    with pytest.raises(NativeError, match="batch"):
        nat.sample(_outs(fields, 9))
    nat.sample(_outs(fields, 8))
    torch.cuda.synchronize()


def test_a_failed_allocation_strands_nothing():
    from tdmpc2_amd.native import NativeError

    free0 = torch.cuda.mem_get_info(dev())[0]
    nat = _native(1 << 40, 1 << 20, [(4096, 0, 4)])  # 4 PiB of storage: create only sizes it
    with pytest.raises(NativeError, match="device memory only"):
        nat.add([torch.zeros(4, 4096, dtype=torch.uint8, device=dev())])
    st = nat.stats()
    assert (st["num_eps"], st["cursor"], st["eligible"]) == (0, 0, 0)
    assert torch.cuda.mem_get_info(dev())[0] >= free0 - (64 << 20)


def test_load_equals_single_adds():
    cap, S, B, N, T = 40, 4, 8, 7, 9  # 63 steps into 40: the load itself evicts its first episodes
    fields = [(20, 0, S), (96, 0, S), (4, 1, S - 1)]
    a, b, ref = _native(cap, S, fields), _native(cap, S, fields), bc.RefBuffer(cap, S, fields)
    rng = np.random.default_rng(8)
    first = _episode(rng, fields, 5)
    a.add([_t(r) for r in first])
    _add(b, ref, first)
    rows = [rng.integers(0, 256, (N, T, rb), dtype=np.uint8) for rb, _, _ in fields]
    a.load([_t(r) for r in rows])
    for i in range(N):
        _add(b, ref, [r[i] for r in rows])
    assert a.stats() == b.stats() == ref.stats()
    for _ in range(2):
        want = ref.sample(B, 17)
        _same(_sample(a, fields, B, 17), want)
        _same(_sample(b, fields, B, 17), want)


def test_a_captured_sample_draws_fresh_slices_and_sees_later_episodes():
    cap, S, B = 64, 4, 8
    fields = [(20, 0, S), (4, 1, S - 1)]
    rng = np.random.default_rng(9)
    eps = [_episode(rng, fields, T) for T in (9, 6, 11)]
    nat = _native(cap, S, fields)
    for e in eps[:2]:
        nat.add([_t(r) for r in e])
    outs, idx = _outs(fields, B), torch.zeros(B, dtype=torch.int64, device=dev())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        nat.sample(outs, seed=77, index_out=idx)
    nat.add([_t(r) for r in eps[2]])  # added after the capture: the replays see it
    torch.cuda.synchronize()
    replays = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        replays.append(([o.cpu().numpy() for o in outs], idx.cpu().numpy()))
    fresh, ref = _native(cap, S, fields), bc.RefBuffer(cap, S, fields)
    for e in eps:
        _add(fresh, ref, e)
    for r in replays:  # eager calls 1 and 2 of a fresh buffer with the same seed and the same adds
        want = ref.sample(B, 77)
        _same(r, want)
        _same(_sample(fresh, fields, B, 77), want)
    assert not np.array_equal(replays[0][1], replays[1][1])
    assert (np.concatenate([r[1] for r in replays]) >= 15).any()  # a slice of the episode added after the capture
    assert nat.stats()["next_call"] == 2


def test_a_replay_that_meets_an_empty_table_touches_nothing():
    cap, S, B = 10, 4, 8
    fields = [(20, 0, S), (4, 1, S - 1)]
    nat = _native(cap, S, fields)
    rng = np.random.default_rng(11)
    nat.add([_t(r) for r in _episode(rng, fields, 6)])
    outs, idx = _outs(fields, B, fill=0xAB), torch.zeros(B, dtype=torch.int64, device=dev())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        nat.sample(outs, seed=1, index_out=idx)
    for _ in range(3):  # nine steps of episodes shorter than a slice evict the only eligible one
        nat.add([_t(r) for r in _episode(rng, fields, 3)])
    assert nat.stats()["eligible"] == 0
    g.replay()
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == -1).all()
    assert all(bool((o == 0xAB).all()) for o in outs)


def _agent(name, **over):
    from oracle import cases
    from tdmpc2_amd.tdmpc2 import TDMPC2

    c = cases.build_case(name)
    cfg = c["cfg"].replace(batch_size=16, buffer_size=200, **over)
    agent = TDMPC2(cfg, device=dev())
    agent.load({k: torch.as_tensor(v) for k, v in c["sd"].items()})
    return agent, cfg


@pytest.mark.parametrize("name", ["tiny", "tiny_mt", "small_ep_fire"])
def test_update_info_on_a_sampled_batch(name):
    """update_info(*buffer.sample()) equals, bit for bit, update_info on tensors gathered with torch indexing at index_out."""
    from tdmpc2_amd import Buffer

    a1, cfg = _agent(name)
    a2, _ = _agent(name)
    H, B, A, od = cfg.horizon, cfg.batch_size, cfg.action_dim, cfg.obs_shape["state"][0]
    rng = np.random.default_rng(13)
    buf = Buffer(cfg, device=dev(), seed=5)
    assert buf.capacity == 200 and buf.num_eps == 0
    full = {k: [] for k in ("obs", "action", "reward", "terminated", "task")}
    for i, T in enumerate((21, H, 30, H + 1, 17)):  # 72 + 2 H steps: no wrap, logical == physical
        td = {"obs": torch.as_tensor(rng.standard_normal((T, od)).astype(np.float32)),
              "action": torch.as_tensor(rng.uniform(-1, 1, (T, A)).astype(np.float32)),
              "reward": torch.as_tensor(rng.standard_normal(T).astype(np.float32))}
        if cfg.episodic:
            td["terminated"] = torch.as_tensor((rng.random(T) < 0.2).astype(np.float32))
        if cfg.multitask:
            td["task"] = torch.full((T,), i % len(cfg.tasks), dtype=torch.int64)
        assert buf.add(td) == i + 1 == buf.num_eps
        for k, v in td.items():
            full[k].append(v)
    full = {k: torch.cat(v).to(dev()) for k, v in full.items() if v}
    obs, action, reward, terminated, task, index = buf.sample(return_index=True)
    assert obs.shape == (H + 1, B, od) and action.shape == (H, B, A) and reward.shape == terminated.shape == (H, B, 1)
    assert obs.dtype == action.dtype == reward.dtype == torch.float32
    assert (task is None) == (not cfg.multitask)
    rows = index[None, :] + torch.arange(H + 1, device=dev())[:, None]
    t_obs, t_action = full["obs"][rows], full["action"][rows[1:]]
    t_reward = full["reward"][rows[1:]].unsqueeze(-1)
    t_term = full["terminated"][rows[1:]].unsqueeze(-1) if cfg.episodic else torch.zeros_like(t_reward)
    t_task = full["task"][rows[0]] if cfg.multitask else None
    assert torch.equal(obs, t_obs) and torch.equal(action, t_action) and torch.equal(reward, t_reward)
    assert torch.equal(terminated, t_term) and (task is None or (task.dtype == torch.int64 and torch.equal(task, t_task)))
    pi_eps = torch.as_tensor(rng.standard_normal((H + 1, B, A)).astype(np.float32))
    qidx = torch.tensor([0, 1], dtype=torch.int32, device=dev())
    # the same batch again through the method under test: a second buffer with the same episodes, seed and call
    buf2 = Buffer(cfg, device=dev(), seed=5)
    off = 0
    for T in (21, H, 30, H + 1, 17):
        buf2.add({k: v[off:off + T] for k, v in full.items()})
        off += T
    torch.manual_seed(1)
    got = a1.update_info_sampled(buf2, pi_eps=pi_eps, qidx=qidx)
    torch.manual_seed(1)
    want = a2.update_info(t_obs, t_action, t_reward, t_term if cfg.episodic else None, t_task, pi_eps=pi_eps, qidx=qidx)
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(torch.as_tensor(got[k]).cpu(), torch.as_tensor(want[k]).cpu()), k
