"""CPU: tdmpc2_amd/csrc/layer_grad_route.h, built with the host compiler (tests/layer_grad_common.build_route): for each GEMM
orientation at the edge shapes the decoded tiles cover every output element exactly once; the workspace size; the order of the
reduction (MFMA steps, partial chains, column parts); offsets past 2^32 elements; the refusals on the descriptor."""
import ctypes

import numpy as np
import pytest

from tests import layer_grad_common as lg


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    return lg.build_route(tmp_path_factory.mktemp("lgroute"))


@pytest.fixture(scope="module")
def const(route):
    out = (ctypes.c_int32 * 10)()
    route.constants(out)
    return dict(zip(lg.CONSTANT_KEYS, [int(v) for v in out]))


SHAPES = [(kind, s) for kind in (lg.LINEAR, lg.MISH, lg.SIMNORM) for s in lg.all_shapes(kind)]


@pytest.mark.parametrize("which", (lg.FWD, lg.DX, lg.DW), ids=("fwd", "dx", "dw"))
def test_tiles_cover_every_output_element_once(route, which):
    for kind, (G, sh, R, K, N) in SHAPES:
        words = lg.desc_words(kind, G, R, K, N, sh, 8 if kind == lg.SIMNORM else 0)
        assert route.check(words) == 0
        g = lg.route_gemm(route, which, words)
        M, Nc, L = {lg.FWD: (R, N, K), lg.DX: (R, K, N), lg.DW: (N, K, R)}[which]
        shared_dx = which == lg.DX and sh
        assert (g["M"], g["Nc"], g["L"]) == (M, Nc, L)
        assert (g["batch"], g["gsum"]) == ((1, G) if shared_dx else (G, 1))
        assert g["blocks"] == g["batch"] * -(-M // 64) * -(-Nc // 64)
        n_out = g["batch"] * M * Nc
        count = np.zeros(n_out, np.uint32)
        bad = route.cover(which, words, count.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n_out)
        assert bad == 0 and (count == 1).all(), (which, kind, G, sh, R, K, N)


def test_operand_offsets_address_the_tensors(route):
    """A(m, l), B(l, n), C(m, n) of each orientation are the elements of x, w, dlin the header's comment names."""
    G, R, K, N = 3, 5, 7, 11
    x, w, d = np.arange(G * R * K).reshape(G, R, K), np.arange(G * N * K).reshape(G, N, K), np.arange(G * R * N).reshape(G, R, N)
    out = (ctypes.c_uint64 * 3)()
    for sh in (False, True):
        words = lg.desc_words(lg.MISH, G, R, K, N, sh)
        xg = lambda g, r, k: r * K + k if sh else x[g, r, k]  # noqa: E731
        for g, r, n, k in ((0, 0, 0, 0), (2, 4, 10, 6), (1, 3, 2, 5)):
            route.offsets(lg.FWD, words, g, r, n, k, out)
            assert list(out) == [xg(g, r, k), w[g, n, k], d[g, r, n]]
            route.offsets(lg.DX, words, g, r, k, n, out)  # m = r, n = k, l = n
            assert list(out)[:2] == [d[g, r, n], w[g, n, k]]
            if not sh:
                assert out[2] == x[g, r, k]
            route.offsets(lg.DW, words, g, n, k, r, out)  # m = n, n = k, l = r
            assert list(out) == [d[g, r, n], xg(g, r, k), w[g, n, k]]
        if sh:  # the one dx of a shared input: group stride 0
            route.offsets(lg.DX, words, 0, 4, 6, 10, out)
            assert out[2] == 4 * K + 6


def test_reduction_order(route, const):
    """One accumulator sees l = 0, 1, 2, ... (k = 0 then k = 1 of every MFMA step, steps and trips in rising order); a partial
    chain ends every LG_SEG_TRIPS trips; the column sums split rows by r % LG_PARTS."""
    assert (const["KT"], const["KSTEP"], const["TILE"], const["BM"], const["BN"], const["THREADS"]) == (32, 2, 32, 64, 64, 256)
    for L in (1, 2, 3, 31, 32, 33, 65, 70, 518, 4096):
        out = (ctypes.c_int32 * (L + 64))()
        n = route.chain(L, out)
        assert n == L and list(out[:L]) == list(range(L))
    assert lg.SEG == 8 * const["KT"]  # the emulation's partial chains are the header's
    assert [route.col_part(r) for r in range(20)] == [r % const["PARTS"] for r in range(20)]
    g = (ctypes.c_uint64 * 3)()
    route.grids(lg.desc_words(lg.MISH, 5, 33, 8, 72), g)
    assert list(g) == [-(-5 * 33 // const["ROW_WAVES"]), 5 * 3, 3]


def test_workspace_size(route, const):
    out = (ctypes.c_uint64 * 3)()
    for kind, G, R, N in ((lg.LINEAR, 1, 1, 1), (lg.MISH, 1, 1, 2), (lg.SIMNORM, 5, 33, 72), (lg.MISH, 1, 96, 512), (lg.MISH, 3, 65536, 4096)):
        route.ws(lg.desc_words(kind, G, R, 8, N, False, 8), out)
        act = -(-G * R * N * 4 // const["ALIGN"]) * const["ALIGN"]
        assert list(out) == [0, act, act if kind == lg.LINEAR else 2 * act]


def test_offsets_past_2_32_elements(route):
    G, R, N, K = 5, 1 << 20, 4096, 2048
    assert route.off3(4, R - 1, N - 1, R, N) == 5 * R * N - 1 > 1 << 32
    out = (ctypes.c_uint64 * 3)()
    words = lg.desc_words(lg.MISH, G, R, K, N)
    route.offsets(lg.FWD, words, 4, R - 1, N - 1, K - 1, out)
    assert list(out) == [5 * R * K - 1, 5 * N * K - 1, 5 * R * N - 1] and out[0] > 1 << 32
    route.offsets(lg.DW, words, 4, N - 1, K - 1, R - 1, out)
    assert list(out) == [5 * R * N - 1, 5 * R * K - 1, 5 * N * K - 1]
    g = lg.route_gemm(route, lg.FWD, words)
    assert g["c_g"] == R * N and g["blocks"] == 5 * (R // 64) * (N // 64)


def test_descriptor_refusals(route):
    ok = dict(kind=lg.MISH, G=2, R=3, K=4, N=8, shared=False, sd=0)
    code = lambda **kw: route.check(lg.desc_words(**{**ok, **kw}))  # noqa: E731
    assert code() == 0
    assert code(kind=3) == 1 and code(kind=-1) == 1
    for dim in ("G", "R", "K", "N"):
        assert code(**{dim: 0}) == 2
    assert code(kind=lg.SIMNORM, sd=0) == 3 and code(kind=lg.SIMNORM, sd=3) == 3 and code(kind=lg.SIMNORM, sd=8) == 0
    assert code(G=1, shared=True) == 4 and code(shared=True) == 0
    assert code(G=1 << 20, R=1 << 20, N=1 << 20) == 5
