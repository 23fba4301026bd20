"""CPU: the launch list of a weight refresh / soft update (tdmpc2_amd/csrc/refresh_route.h, compiled with the host compiler) is a
constant, small number of grouped launches: the same for every num_q, with or without termination head, target ensemble,
encoder and policy copy; within the bound the header states; and nothing is launched for nets the table does not name."""
import itertools

import pytest

from tests import refresh_route_model as m


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return m.build(tmp_path_factory.mktemp("refresh_route"))


def test_launch_list_does_not_depend_on_the_model(lib):
    base = m.DYN | m.REW | m.PI | m.Q
    for split in (1, 0):
        want = [m.RESET, m.SCAN, m.SCALES, m.PACK] if split else [m.PACK]
        for nq, term, tq, enc, pol in itertools.product((2, 5, 8), (0, 1), (0, 1), (0, 2, 6), (0, 1)):
            nets = base | (m.TERM if term else 0) | (m.TQ if tq else 0)
            r = m.route(lib, split, nets, enc_layers=enc, policy_copy=pol, num_q=nq, episodic=term)
            assert r["ops"] == want, (split, nq, term, tq, enc, pol, r)
            assert len(r["ops"]) <= r["max_ops"] == 4
            assert (r["nets"], r["enc_layers"], r["policy_copy"]) == (nets, enc, pol)
        # fewer launches for the exact-fp32 arithmetic
        assert len(m.route(lib, 0, base)["ops"]) < len(m.route(lib, 1, base)["ops"])


def test_partial_and_empty_tables(lib):
    for split in (1, 0):
        assert m.route(lib, split, 0)["ops"] == []                            # nothing named: nothing launched
        r = m.route(lib, split, m.Q)
        assert r["nets"] == m.Q and r["ops"] == m.route(lib, split, m.DYN | m.REW | m.PI | m.Q | m.TQ)["ops"]
        assert m.route(lib, split, 0, enc_layers=2)["ops"] == [m.PACK]        # the encoder alone has nothing to scale
        assert m.route(lib, split, m.Q, policy_copy=1)["policy_copy"] == 0    # the policy copy follows TDMPC2_NET_PI only
        assert m.route(lib, split, 0xFC0)["nets"] == 0                        # bits beyond the six nets name nothing


def test_soft_update_costs_a_one_net_refresh(lib):
    assert m.route(lib, 1, m.TQ, lerp=1)["ops"] == m.route(lib, 1, m.TQ)["ops"] == [m.RESET, m.SCAN, m.SCALES, m.PACK]
    assert m.route(lib, 0, m.TQ, lerp=1)["ops"] == [m.SCAN, m.PACK]           # exact fp32: the scan launch only lerps


def test_one_layer_binds(lib):
    """tdmpc2_plan_bind_weights names one net (one layer of it): it routes as a one-net table does.  tdmpc2_plan_bind_encoder is
    the encoder alone.  tdmpc2_plan_bind_policy is a policy-copy transpose with no net named: one pack launch, whatever the
    arithmetic, and the copy is touched although TDMPC2_NET_PI is not in `nets`."""
    for net in (m.DYN, m.REW, m.PI, m.TERM, m.Q, m.TQ):
        assert m.route(lib, 1, net)["ops"] == [m.RESET, m.SCAN, m.SCALES, m.PACK]
        assert m.route(lib, 0, net)["ops"] == [m.PACK]
    for split, nq, ep in itertools.product((1, 0), (2, 5, 8), (0, 1)):
        r = m.route(lib, split, 0, policy_alone=1, num_q=nq, episodic=ep)
        assert r["ops"] == [m.PACK] and (r["nets"], r["enc_layers"], r["policy_copy"]) == (0, 0, 1)
        assert m.route(lib, split, 0, enc_layers=1, num_q=nq, episodic=ep)["ops"] == [m.PACK]
    assert m.route(lib, 1, 0, policy_copy=1)["ops"] == []                      # the table's flag alone still names nothing
    assert m.route(lib, 1, m.Q, policy_copy=1, policy_alone=0)["policy_copy"] == 0


def test_grids(lib):
    assert [lib.scan_wblocks(n) for n in (0, 1, 4096, 4097, 512 * 4096, 10 ** 9)] == [1, 1, 1, 2, 512, 512]
    assert lib.pack_blocks(16, 528, 0) == 16 * 5 + 1 and lib.pack_blocks(16, 512, 64) == 16 * 4 + 1 + 16
    assert lib.pack_blocks(1, 16, 0) == 2
    assert lib.transpose_blocks(32, 11) == 1 and lib.transpose_blocks(33, 64) == 4
