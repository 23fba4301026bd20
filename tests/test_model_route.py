"""CPU test of tdmpc2_amd/csrc/model_route.h (compiled with g++: tests/model_route_model.py) against an independent Python model
over a grid of (family, B, H, num_q, output sets): every requested output is produced by exactly one stage, no stage is launched
whose outputs are all unwanted, grids cover all rows, row counts beyond the workspace are refused."""
import itertools

import pytest

from tests import model_route_model as mrm

BS = (1, 40, 64, 130, 256, 1024)
HS = tuple(range(9))
NQS = (2, 5, 8)
WANTS = (0, mrm.ZS, mrm.REW, mrm.REW_LOGITS | mrm.Q, mrm.Q_LOGITS, mrm.TERM, mrm.ZS | mrm.TERM, mrm.LOSSES, mrm.LOSSES | mrm.Q_LOGITS | mrm.ZS,
         mrm.ZS | mrm.REW_LOGITS | mrm.REW | mrm.Q_LOGITS | mrm.Q | mrm.TERM)
CAP = 2048  # layered workspace rows of the grid (max_envs x num_samples)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return mrm.build(tmp_path_factory.mktemp("model_route"))


@pytest.mark.parametrize("family", [mrm.FUSED, mrm.LAYERED])
@pytest.mark.parametrize("episodic", [False, True])
def test_route_matches_model(lib, family, episodic):
    for B, H, nq, want in itertools.product(BS, HS, NQS, WANTS):
        r = mrm.route(lib, family, B, H, nq, 101, episodic, want, CAP)
        e = mrm.expected(family, B, H, nq, 101, episodic, want, CAP)
        key = (family, episodic, B, H, nq, want)
        assert r["refuse"] == e["refuse"], key
        if e["refuse"]:
            assert r["launches"] == 0 and not any(s["run"] for s in r["st"]), key
            continue
        st = r["st"]
        assert r["chain"] == e["chains"], key
        # no stage without a consumer
        assert bool(st[mrm.DYN]["run"]) == (e["steps"] > 0) and st[mrm.DYN]["steps"] == e["steps"], key
        assert bool(st[mrm.HEADS]["run"]) == bool(e["chains"]), key
        assert bool(st[mrm.TERM_STAGE]["run"]) == e["term"], key
        assert bool(st[mrm.CONS]["run"]) == bool(st[mrm.TAIL]["run"]) == e["losses"], key
        # every requested output by exactly one stage
        for bit in (mrm.ZS, mrm.REW_LOGITS, mrm.REW, mrm.Q_LOGITS, mrm.Q, mrm.TERM, mrm.LOSSES):
            makers = [s for s in st if s["run"] and s["produces"] & bit]
            if want & bit and not (bit == mrm.ZS and H == 0) and not (H == 0 and bit in (mrm.REW_LOGITS, mrm.REW, mrm.Q_LOGITS, mrm.Q)):
                assert len(makers) == 1, (key, bit)   # (H = 0: zs[0] = z0 is a copy, the [0, B, ...] outputs are empty)
            else:
                assert len(makers) <= 1, (key, bit)
        assert not any(s["produces"] & ~want for s in st), key
        # grids cover all rows
        tiles = -(-B // mrm.TILE)
        if family == mrm.FUSED:
            if st[mrm.DYN]["run"]:
                assert st[mrm.DYN]["gx"] * mrm.TILE >= B and st[mrm.DYN]["gx"] == tiles
            if st[mrm.HEADS]["run"]:
                h = st[mrm.HEADS]
                assert (h["gx"], h["gy"], h["gz"]) == (tiles, H, len(e["chains"])) and h["launches"] == 1
            if st[mrm.TERM_STAGE]["run"]:
                t = st[mrm.TERM_STAGE]
                assert (t["gx"], t["gy"], t["gz"]) == (tiles, H + 1, 1)
        else:
            if st[mrm.HEADS]["run"]:
                assert st[mrm.HEADS]["rows"] == H * B <= CAP and st[mrm.HEADS]["gx"] * 4 >= H * B
            if st[mrm.TERM_STAGE]["run"]:
                t = st[mrm.TERM_STAGE]
                assert t["rows"] <= CAP and t["rows"] * t["chunks"] >= (H + 1) * B > t["rows"] * (t["chunks"] - 1)
        if e["losses"]:
            assert st[mrm.CONS]["rows"] == H * B and st[mrm.CONS]["gx"] * 4 >= H * B
            assert (st[mrm.TAIL]["gx"], st[mrm.TAIL]["gy"], st[mrm.TAIL]["gz"]) == (1, 1, 1)
        assert r["launches"] == sum(s["launches"] for s in st), key
        for ln_after in (0, 1):   # the launch count, against the host code's sequences counted independently
            r2 = mrm.route(lib, family, B, H, nq, 101, episodic, want, CAP, ln_after)
            assert r2["launches"] == mrm.expected_launches(family, B, H, nq, episodic, want, CAP, ln_after), (key, ln_after)


def test_refusals(lib):
    assert mrm.route(lib, mrm.FUSED, 256, 9, 5, 101, False, mrm.ZS, 0)["refuse"] == mrm.BAD_H
    assert mrm.route(lib, mrm.FUSED, 0, 3, 5, 101, False, mrm.ZS, 0)["refuse"] == mrm.BAD_B
    assert mrm.route(lib, mrm.FUSED, 256, 3, 5, 101, False, mrm.TERM, 0)["refuse"] == mrm.NOT_EPISODIC
    assert mrm.route(lib, mrm.FUSED, 256, 3, 5, 1, False, mrm.LOSSES, 0)["refuse"] == mrm.NO_BINS
    assert mrm.route(lib, mrm.FUSED, 256, 0, 5, 101, False, mrm.LOSSES, 0)["refuse"] == mrm.LOSSES_H0
    assert mrm.route(lib, mrm.LAYERED, 256, 5, 5, 101, False, mrm.ZS, 1024)["refuse"] == mrm.ROWS
    assert mrm.route(lib, mrm.LAYERED, 256, 4, 5, 101, False, mrm.ZS, 1024)["refuse"] == mrm.OK
    assert mrm.route(lib, mrm.FUSED, 4096, 8, 5, 101, False, mrm.ZS, 0)["refuse"] == mrm.OK   # the fused family takes any number of rows
    assert lib.rowloss_floats(256, 3, 5) == 8 * 3 * 256
