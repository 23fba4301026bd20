"""-m gpu: the weight refresh in one call and the target-Q soft update (ABI 14).  tdmpc2_plan_refresh_weights must reproduce the
per-layer binds, so the criterion has no tolerance: byte identity of tdmpc2_plan_export_packed (slabs, scale records, biases,
LayerNorm vectors, task-embedding columns, encoder); the policy prior's fp32 copy is compared through tdmpc2_plan_pi.  Both
are job tables over ONE packer, so the bytes themselves are pinned to recorded digests (tests/golden/packed_digests.json) and
the one-layer jobs of the per-layer binds are tested where a layer mask can go wrong.  The
soft update's lerp is gated per element against fp64, |out - ref64| <= 2^-23 (|t| + |o|) (tests/refresh_common.py), and its
pack against a handle freshly bound from the lerped tensors."""
import json
import os
import struct

import numpy as np
import pytest
import torch

from tests import refresh_common as rc
from tests.gpu_common import dev

pytestmark = pytest.mark.gpu

CASES, IDS = rc.CASES, rc.IDS
_cases = {}


def _case(name):
    from oracle import cases

    if name not in _cases:
        _cases[name] = cases.build_case(name)
    return _cases[name]


def _sd(c):
    return rc.device_sd(c, dev())


def _planner(c, path, prec):
    from tdmpc2_amd.native import NativePlanner

    return NativePlanner(c["cfg"], c["iterations"], dev(), max_envs=2, path=path, precision=prec)


def _bind(pl, sd):
    pl.bind_state_dict(sd)
    pl.bind_encoder(sd)
    if pl.policy_bound:
        pl.bind_policy(sd)


_perturb, _edge_weights = rc.perturb, rc.edge_weights


def _diff_owners(a, b, cfg, split):
    sa, sb = rc.blob_segments(a, cfg, split), rc.blob_segments(b, cfg, split)
    return {o for (o, x), (_, y) in zip(sa, sb) if x != y}


def _td(pl, c, sd):
    cfg = c["cfg"]
    z = torch.as_tensor(c["z0"]).to(dev())
    R = z.shape[0]
    r = torch.linspace(-1, 1, R, device=dev())
    term = torch.zeros(R, device=dev())
    eps = torch.randn(R, cfg.action_dim, generator=torch.Generator().manual_seed(5)).to(dev())
    qidx = torch.tensor([1, 0], dtype=torch.int32, device=dev())
    if not cfg.multitask:
        return pl.td_target(z, r, term, 0.99, pi_eps=eps, qidx=qidx)
    ids = torch.as_tensor(np.asarray(c["tasks"][:R]), dtype=torch.int32).to(dev())
    emb = torch.as_tensor(np.asarray(c["sd"]["_task_emb.weight"])).to(dev(), torch.float32)
    emb = emb / emb.norm(dim=1, keepdim=True).clamp(min=1.0)
    mask = torch.as_tensor(np.asarray(c["sd"]["_action_masks"])).to(dev(), torch.float32)
    disc = torch.full((emb.shape[0],), 0.99, device=dev())
    return pl.td_target(z, r, term, disc, pi_eps=eps, qidx=qidx, task_ids=ids, task_emb_table=emb.contiguous(),
                        act_mask_table=mask.contiguous())


# ---------------------------------------------------------------- 1. blob identity
@pytest.mark.parametrize("name,path,prec", CASES, ids=IDS)
def test_refresh_reproduces_the_binds_byte_for_byte(name, path, prec):
    c = _case(name)
    sd = _sd(c)
    A, B = _planner(c, path, prec), _planner(c, path, prec)
    _bind(A, sd)
    B.refresh_state_dict(sd)  # a never-bound handle becomes ready through this call alone
    assert A.export_packed() == B.export_packed()
    assert B.encoder_layers == A.encoder_layers and B.obs_dim == A.obs_dim
    _perturb(sd, 1)
    _bind(A, sd)
    B.refresh_state_dict(sd)
    first = A.export_packed()
    assert first == B.export_packed()
    for i, variant in enumerate(("zero_last", "ln_gain", "kw_clamps", "nonfinite")):
        sd = _sd(c)
        _edge_weights(sd, variant)
        _bind(A, sd)
        B.refresh_state_dict(sd)
        a = A.export_packed()
        assert a != first
        assert a == B.export_packed(), variant
    A.close()
    B.close()


# ---------------------------------------------------------------- 1b. the bytes themselves, pinned
@pytest.mark.parametrize("name,path,prec", CASES, ids=IDS)
def test_packed_bytes_match_the_recorded_digests(name, path, prec, request):
    """tests/golden/packed_digests.json (tools/make_packed_digests.py) holds, per weight set and segment owner, the SHA-256 of
    what the commit named in the file packed.  Both ways of filling a handle must still produce exactly those bytes."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", rc.PACKED_DIGESTS)) as f:
        rec = json.load(f)["rows"][request.node.callspec.id]
    c = _case(name)
    A, B = _planner(c, path, prec), _planner(c, path, prec)
    seen = []
    for label, sd in rc.packed_inputs(c, dev()):
        assert rc.sd_digest(sd) == rec[label]["input"], f"{label}: the INPUT tensors differ from the recorded ones, not the packer"
        A.bind_state_dict(sd)
        A.bind_encoder(sd)
        B.refresh_state_dict(sd)
        for way, pl in (("binds", A), ("refresh", B)):
            got = rc.owner_digests(pl.export_packed(), c["cfg"], prec == 2)
            assert got == rec[label]["owners"], (label, way, sorted(o for o in got if got[o] != rec[label]["owners"].get(o)))
        seen.append(label)
    assert sorted(seen) == sorted(rec) and len(seen) == 2 + len(rc.EDGE_VARIANTS)
    A.close()
    B.close()


# ---------------------------------------------------------------- 1c. one-layer jobs: where the layer mask can go wrong
ONE_LAYER = dict(argnames="name,path,prec", argvalues=[CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
FIELDS = ("weight", "bias", "ln.weight", "ln.bias")


def _bind_layer(pl, sd, net, layer):
    """tdmpc2_plan_bind_weights itself: one (net, layer), every ensemble member."""
    from tdmpc2_amd import native

    t = [sd.get(f"{native.NET_PREFIX[net]}.{layer}.{n}") for n in FIELDS]
    pl._check(pl.lib.tdmpc2_plan_bind_weights(pl._h, net, layer, *(native._ptr(x) for x in t), int(t[0].shape[-2]), int(t[0].shape[-1]),
                                              pl._stream()))


def _scales(blob, cfg, owner):
    """[head][layer] -> dict of the LayerScal record (the last segment of every ensemble member of a split handle)."""
    segs = [x for o, x in rc.blob_segments(blob, cfg, True) if o == owner]
    heads = int(cfg.num_q) if owner in ("q", "target_q") else 1
    per = len(segs) // heads
    names = ("wscale", "oscale", "maxbits", "kw", "ascale", "ka", "gmax", "bmax")
    return [[dict(zip(names, struct.unpack_from("<ffIifiII", segs[hd * per + per - 1], 32 * l))) for l in range(3)] for hd in range(heads)]


def _layer1_variant(c):
    """The ln_gain and kw_clamps weight sets in one, with edits of the same kinds on the layer-1 tensors this test re-binds
    (those two sets leave `_dynamics.1.*` alone): kw AND ka of layer 1 move in both nets."""
    v = _sd(c)
    _edge_weights(v, "ln_gain")
    _edge_weights(v, "kw_clamps")
    with torch.no_grad():
        v["_dynamics.1.ln.weight"][3] = 1e3
        v["_dynamics.1.weight"][5, 9] = 3e4
        v["_Qs.params.1.weight"][1, 2, 3] = 1e20
    return v


@pytest.mark.parametrize(**ONE_LAYER)
def test_rebinding_one_layer_leaves_its_neighbours(name, path, prec):
    from tdmpc2_amd import native

    c = _case(name)
    cfg, sd, v = c["cfg"], _sd(c), _layer1_variant(c)
    A = _planner(c, path, prec)
    _bind(A, sd)
    before = A.export_packed()
    mixed = {k: (v[k] if k.startswith(("_dynamics.1.", "_Qs.params.1.")) else t) for k, t in sd.items()}
    _bind_layer(A, mixed, native.NET_DYNAMICS, 1)
    _bind_layer(A, mixed, native.NET_Q, 1)
    after = A.export_packed()
    F = _planner(c, path, prec)
    _bind(F, mixed)
    assert after == F.export_packed()
    assert _diff_owners(before, after, cfg, True) == {"dynamics", "q"}
    for owner, hd in (("dynamics", 0), ("q", 1)):  # the member whose tensors were edited
        s0, s1 = _scales(before, cfg, owner)[hd], _scales(after, cfg, owner)[hd]
        assert (s1[0]["kw"], s1[2]["kw"]) == (s0[0]["kw"], s0[2]["kw"]) and s1[0] == s0[0]
        assert s1[1]["kw"] != s0[1]["kw"] and s1[1]["ka"] != s0[1]["ka"]
        assert s1[2]["oscale"] == 2.0 ** -(s1[2]["kw"] + s1[1]["ka"]) != s0[2]["oscale"]
    A.close()
    F.close()


@pytest.mark.parametrize(**ONE_LAYER)
def test_layer_order_of_the_binds_does_not_matter(name, path, prec):
    from tdmpc2_amd import native

    c = _case(name)
    sd = _sd(c)
    _edge_weights(sd, "ln_gain")  # scales that differ between the layers
    A, R = _planner(c, path, prec), _planner(c, path, prec)
    _bind(A, sd)
    for net, prefix in native.NET_PREFIX.items():
        if f"{prefix}.0.weight" in sd:
            for layer in (2, 1, 0):
                _bind_layer(R, sd, net, layer)
    R.bind_encoder(sd)
    assert R.export_packed() == A.export_packed()
    A.close()
    R.close()


@pytest.mark.parametrize(**ONE_LAYER)
def test_rebinding_one_encoder_layer_touches_the_encoder_only(name, path, prec):
    from tdmpc2_amd import native

    c = _case(name)
    cfg, sd = c["cfg"], _sd(c)
    A = _planner(c, path, prec)
    _bind(A, sd)
    before = A.export_packed()
    mixed = dict(sd)
    for n in FIELDS:
        mixed[f"_encoder.state.0.{n}"] = sd[f"_encoder.state.0.{n}"] * 1.5 + 0.25
    t = [mixed[f"_encoder.state.0.{n}"] for n in FIELDS]
    A._check(A.lib.tdmpc2_plan_bind_encoder(A._h, 0, A.encoder_layers, *(native._ptr(x) for x in t), int(t[0].shape[0]), int(t[0].shape[1]),
                                            A._stream()))
    after = A.export_packed()
    assert _diff_owners(before, after, cfg, True) == {"encoder"}
    F = _planner(c, path, prec)
    _bind(F, mixed)
    assert after == F.export_packed()
    A.close()
    F.close()


@pytest.mark.parametrize(**ONE_LAYER)
def test_policy_bind_alone_moves_the_copy_only(name, path, prec):
    c = _case(name)
    cfg, sd = c["cfg"], _sd(c)
    A, F = _planner(c, path, prec), _planner(c, path, prec)
    _bind(A, sd)  # `_pi` is packed here ...
    A.bind_policy(sd)
    blob = A.export_packed()
    z = torch.as_tensor(c["z0"]).to(dev())
    eps = torch.randn(z.shape[0], cfg.action_dim, generator=torch.Generator().manual_seed(2)).to(dev())
    before = A.pi(z, eps=eps)[0].clone()
    new = _sd(c)
    _perturb(new, 3, scale=0.05)
    A.bind_policy(new)  # ... and only the prior's fp32 copy follows the new tensors
    assert A.export_packed() == blob
    _bind(F, new)
    F.bind_policy(new)
    (aa, ia), (af, i_f) = A.pi(z, eps=eps), F.pi(z, eps=eps)
    assert torch.equal(aa, af) and not torch.equal(aa, before)
    for k in ("mean", "log_std", "entropy", "scaled_entropy"):
        assert torch.equal(ia[k], i_f[k]), k
    A.close()
    F.close()


# ---------------------------------------------------------------- 2. the policy prior's fp32 copy
@pytest.mark.parametrize("name,path,prec", [CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
def test_refresh_covers_the_bound_policy_copy(name, path, prec):
    c = _case(name)
    cfg, sd = c["cfg"], _sd(c)
    A, B = _planner(c, path, prec), _planner(c, path, prec)
    for pl in (A, B):
        _bind(pl, sd)
        pl.bind_policy(sd)
    z = torch.as_tensor(c["z0"]).to(dev())
    eps = torch.randn(z.shape[0], cfg.action_dim, generator=torch.Generator().manual_seed(2)).to(dev())
    before = B.pi(z, eps=eps)[0].clone()
    _perturb(sd, 3, scale=0.05)
    _bind(A, sd)
    B.refresh_state_dict(sd)
    (aa, ia), (ab, ib) = A.pi(z, eps=eps), B.pi(z, eps=eps)
    assert torch.equal(aa, ab) and not torch.equal(ab, before)
    for k in ("mean", "log_std", "entropy", "scaled_entropy"):
        assert torch.equal(ia[k], ib[k]), k
    A.close()
    B.close()


# ---------------------------------------------------------------- 3. partial table
@pytest.mark.parametrize("name,path,prec", [CASES[0], CASES[4]], ids=[IDS[0], IDS[4]])
def test_partial_table_touches_only_its_net(name, path, prec):
    from tdmpc2_amd import native

    c = _case(name)
    sd = _sd(c)
    B = _planner(c, path, prec)
    B.refresh_state_dict(sd)
    before = B.export_packed()
    _perturb(sd, 4)
    B.refresh_state_dict(sd, nets=(native.NET_Q,))
    after = B.export_packed()
    assert _diff_owners(before, after, c["cfg"], prec == 2) == {"q"}
    # ... and Q's segments are the ones a bind of the new tensors gives
    A = _planner(c, path, prec)
    _bind(A, sd)
    want = rc.blob_segments(A.export_packed(), c["cfg"], prec == 2)
    got = rc.blob_segments(after, c["cfg"], prec == 2)
    assert all(x == y for (o, x), (_, y) in zip(want, got) if o == "q")
    A.close()
    B.close()


# ---------------------------------------------------------------- 4. soft update
TQ = "_target_Qs_params."


def _np(sd, prefix):
    return {k[len(prefix):]: v.detach().cpu().numpy().copy() for k, v in sd.items() if k.startswith(prefix)}


@pytest.mark.parametrize("name,path,prec", CASES, ids=IDS)
def test_soft_update_lerps_in_place_and_packs_the_result(name, path, prec):
    c = _case(name)
    cfg, sd = c["cfg"], _sd(c)
    split = prec == 2
    with torch.no_grad():
        for k in sd:
            if k.startswith(TQ):  # a target that is not the online ensemble
                sd[k].add_(0.05 * torch.randn(sd[k].shape, generator=torch.Generator().manual_seed(11)).to(dev()))
    B = _planner(c, path, prec)
    B.refresh_state_dict(sd)
    ptrs = {k: v.data_ptr() for k, v in sd.items()}
    worst = -np.inf
    for step, tau in enumerate((0.01, 0.01, 0.01, 0.7)):
        with torch.no_grad():
            for k in sd:
                if k.startswith("_Qs.params."):  # the online ensemble moves between updates
                    sd[k].add_(0.01 * torch.randn(sd[k].shape, generator=torch.Generator().manual_seed(20 + step)).to(dev()))
        B.refresh_state_dict(sd)  # as a training loop does after its optimiser step
        t_prev, o = _np(sd, TQ), _np(sd, "_Qs.params.")
        B.soft_update_target(sd, tau)
        t_new = _np(sd, TQ)
        for k in rc.Q_KEYS:  # (a) per element against the fp64 lerp of the previous values
            ex = rc.gate_excess(t_new[k], rc.lerp64(t_prev[k], o[k], tau), t_prev[k], o[k])
            worst = max(worst, ex)
            assert ex <= 0.0, (step, k, ex)
        assert not np.array_equal(t_new["0.weight"], t_prev["0.weight"])
    print(f"[{name}] soft update: worst excess over the gate {worst:.3e} (<= 0 passes)")
    assert {k: v.data_ptr() for k, v in sd.items()} == ptrs  # in place: the state dict save() writes stays the truth
    # (b) the packed target is the pack of the tensors the caller now holds
    A = _planner(c, path, prec)
    _bind(A, sd)
    blob = B.export_packed()
    assert blob == A.export_packed()
    # (d) td_target on the updated handle = td_target of the freshly bound one
    assert torch.equal(_td(B, c, sd), _td(A, c, sd))
    # (c) tau = 0: nothing moves; tau = 1: the target's segments are the online Q's pack
    keep = _np(sd, TQ)
    B.soft_update_target(sd, 0.0)
    assert all(np.array_equal(v.view(np.uint32), _np(sd, TQ)[k].view(np.uint32)) for k, v in keep.items())
    assert B.export_packed() == blob
    B.soft_update_target(sd, 1.0)
    assert all(torch.equal(sd[TQ + k], sd["_Qs.params." + k]) for k in rc.Q_KEYS)
    segs = rc.blob_segments(B.export_packed(), cfg, split)
    assert [x for o, x in segs if o == "target_q"] == [x for o, x in segs if o == "q"]
    assert _diff_owners(B.export_packed(), blob, cfg, split) == {"target_q"}
    A.close()
    B.close()


def test_soft_update_against_the_reference_fixture():
    """Each of the fixture's three steps, started from the reference's own fp32 tensors of the step before, against the
    reference's fp64 under the same gate."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", rc.GOLDEN))
    c = _case("tiny")
    target, online = rc.tiny_inputs()
    assert str(g["digest.target"]) == rc.digest(target)
    sd = _sd(c)
    B = _planner(c, 0, 0)
    B.refresh_state_dict(sd)
    cur, worst = target, -np.inf
    for k in range(1, rc.STEPS + 1):
        o = online[k - 1]
        assert str(g[f"digest.online.{k}"]) == rc.digest(o)
        with torch.no_grad():
            for key in rc.Q_KEYS:
                sd[TQ + key].copy_(torch.as_tensor(cur[key]))
                sd["_Qs.params." + key].copy_(torch.as_tensor(o[key]))
        B.soft_update_target(sd, float(g["tau"]))
        for key in rc.Q_KEYS:
            s = rc.scale_of(cur[key], o[key])
            ref = rc.decode64(g[f"t32.{k}/{key}"], g[f"r64.{k}/{key}"], s)
            ex = rc.gate_excess(sd[TQ + key].cpu().numpy(), ref, cur[key], o[key], slack=rc.TAIL_ERR)
            worst = max(worst, ex)
            assert ex <= 0.0, (k, key, ex)
        cur = {key: g[f"t32.{k}/{key}"] for key in rc.Q_KEYS}
    print(f"soft update vs the reference's fp64: worst excess over the gate {worst:.3e} (<= 0 passes)")
    B.close()


# ---------------------------------------------------------------- 5. graph
@pytest.mark.parametrize("name,path,prec", [CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
def test_refresh_soft_update_td_target_in_a_graph(name, path, prec):
    """refresh + soft update + td_target captured as one linear chain; the source tensors change in place, the replay equals
    the eager sequence on the new values (the table's pointers are those of the capture)."""
    c = _case(name)
    sd = _sd(c)
    G, E = _planner(c, path, prec), _planner(c, path, prec)
    z = torch.as_tensor(c["z0"]).to(dev())
    R = z.shape[0]
    r, term = torch.linspace(-1, 1, R, device=dev()), torch.zeros(R, device=dev())
    eps = torch.randn(R, c["cfg"].action_dim, generator=torch.Generator().manual_seed(5)).to(dev())
    qidx = torch.tensor([1, 0], dtype=torch.int32, device=dev())

    def seq(pl, d):
        pl.refresh_state_dict(d)
        pl.soft_update_target(d, 0.25)
        return pl.td_target(z, r, term, 0.99, pi_eps=eps, qidx=qidx)

    sd_g = {k: v.clone() for k, v in sd.items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        seq(G, sd_g)  # first call: storage is allocated here, outside the capture
        for k, v in sd.items():
            sd_g[k].copy_(v)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out_g = seq(G, sd_g)
    _perturb(sd, 9)
    for k, v in sd.items():
        sd_g[k].copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    want = seq(E, sd)
    torch.cuda.synchronize()
    assert torch.equal(out_g, want)
    assert all(torch.equal(sd_g[k], sd[k]) for k in sd)  # the replay lerped the graph's tensors as the eager call lerped its own
    assert G.export_packed() == E.export_packed()
    G.close()
    E.close()


# ---------------------------------------------------------------- 6. boundary
def _agent(name):
    from tdmpc2_amd.tdmpc2 import TDMPC2

    c = _case(name)
    agent = TDMPC2(c["cfg"].replace(), device=dev(), max_envs=1)
    agent.load({"model": {k: torch.as_tensor(np.asarray(v)) for k, v in c["sd"].items()}})
    return c, agent


@pytest.mark.parametrize("name", ["c1", "small_ep"])
def test_native_refresh_flag_gives_the_default_path_s_action(name):
    from oracle import planner_oracle as po
    from tdmpc2_amd import synth

    acts = []
    for flag in (False, True):
        c, agent = _agent(name)
        agent.native_refresh = flag
        agent.noise_tape = {k: v.unsqueeze(0).to(agent.device).contiguous() for k, v in po.env_tape(c["tape"], 0).items()}
        obs = torch.as_tensor(synth.make_obs(c["cfg"], c["n_envs"], seed=3)[0])
        agent.act(obs, t0=True)  # the handle exists
        with torch.no_grad():
            g = torch.Generator().manual_seed(6)
            for p in agent.model.parameters():
                p.add_((0.01 * torch.randn(p.shape, generator=g)).to(p.device))
        agent.sync_planner_weights()
        acts.append(agent.act(obs, t0=True).clone())
        agent._planner.close()
    assert torch.equal(acts[0], acts[1])


def test_soft_update_target_q_of_the_agent():
    c, agent = _agent("c1")
    with torch.no_grad():
        for p in agent.model._Qs.parameters():
            p.add_(0.03)
    st = agent.model.state_dict()
    t_prev = {k: st[TQ + k].cpu().numpy().copy() for k in rc.Q_KEYS}
    o = {k: st["_Qs.params." + k].cpu().numpy() for k in rc.Q_KEYS}
    agent.soft_update_target_Q()  # whatever native_refresh says
    st = agent.model.state_dict()
    tau = float(agent.cfg.tau)
    for k in rc.Q_KEYS:
        out = st[TQ + k].cpu().numpy()
        assert rc.gate_excess(out, rc.lerp64(t_prev[k], o[k], tau), t_prev[k], o[k]) <= 0.0, k
        assert not np.array_equal(out, t_prev[k])
    # the handle's target ensemble is the pack of the model's buffers
    from tdmpc2_amd.native import NativePlanner

    A = NativePlanner(agent.cfg, agent.cfg.iterations, dev(), max_envs=1, log_std_min=agent._planner_log_std[0],
                      log_std_dif=agent._planner_log_std[1])
    sd = {k: v for k, v in st.items() if torch.is_tensor(v)}
    A.bind_state_dict(sd)
    A.bind_encoder(sd)
    assert A.export_packed() == agent.planner().export_packed()
    A.close()


def test_refusals_leave_the_handle_usable():
    from tdmpc2_amd import native
    from tdmpc2_amd.native import NativeError

    c = _case("c1")
    sd = _sd(c)
    B = _planner(c, 1, 2)
    B.refresh_state_dict(sd)
    blob = B.export_packed()
    INVALID = "tdmpc2_plan error 1:"
    for tau in (-0.1, 1.01, float("nan")):
        with pytest.raises(NativeError, match=INVALID + ".*tau"):
            B.soft_update_target(sd, tau)
    tab = B.weight_table(sd, nets=(native.NET_PI,))  # online Q missing from the table
    tgt = (native.C.c_void_p * 4 * 3)()
    for l in range(3):
        for i, (_, n) in enumerate(native.WEIGHT_FIELDS):
            if f"{TQ}{l}.{n}" in sd:
                tgt[l][i] = sd[f"{TQ}{l}.{n}"].data_ptr()
    assert B.lib.tdmpc2_plan_soft_update_target(B._h, native.C.byref(tab), tgt, 0.01, B._stream()) == 1
    assert b"online Q" in B.lib.tdmpc2_last_error()
    assert B.lib.tdmpc2_plan_refresh_weights(B._h, None, B._stream()) == 1  # null table
    tab = B.weight_table(sd)
    tab.net[native.NET_REWARD][1].b = None  # a named net must bring every layer
    assert B.lib.tdmpc2_plan_refresh_weights(B._h, native.C.byref(tab), B._stream()) == 1
    tab = B.weight_table(sd)
    tab.net[native.NET_TERMINATION][0].W = sd["_reward.0.weight"].data_ptr()  # termination entries, non-episodic handle
    assert B.lib.tdmpc2_plan_refresh_weights(B._h, native.C.byref(tab), B._stream()) == 1
    assert b"termination" in B.lib.tdmpc2_last_error()
    tab = B.weight_table(sd)
    tab.enc_out[1] = 256  # the encoder's shape through the cfg: the last layer must give latent_dim
    assert B.lib.tdmpc2_plan_refresh_weights(B._h, native.C.byref(tab), B._stream()) == 1
    # the binding refuses what it would otherwise have to copy
    with pytest.raises(NativeError, match="contiguous float32"):
        B.refresh_state_dict({**sd, "_pi.0.weight": sd["_pi.0.weight"].double()})
    with pytest.raises(NativeError, match="contiguous float32"):
        B.refresh_state_dict({**sd, "_pi.1.weight": sd["_pi.1.weight"].t()})
    with pytest.raises(NativeError, match="contiguous float32"):
        B.refresh_state_dict({**sd, "_pi.0.bias": sd["_pi.0.bias"].cpu()})
    with pytest.raises(NativeError, match="shape"):
        B.refresh_state_dict({**sd, "_pi.0.bias": sd["_pi.0.bias"][:-1].contiguous()})
    # nothing was enqueued by a refused call, and the handle still plans
    assert B.export_packed() == blob
    from oracle import planner_oracle as po
    from tests.gpu_common import plan_inputs

    model = po.OracleModel(c["cfg"], {k: torch.as_tensor(v) for k, v in c["sd"].items()})
    inp = plan_inputs(c, model)
    a = B.plan(inp["z0"], inp["disc_pow"], inp["prev_mean"], inp["t0"], tape=inp["tape"])
    assert torch.isfinite(a).all()
    B.close()
