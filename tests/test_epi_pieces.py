"""Source checks of two rearrangements of tdmpc2_amd/csrc/fused_kernels.cuh that must not touch the arithmetic: the NormedLinear
epilogue epi_t can be taken in three pieces (statistics / math / tile store) through a compile-time mask over ONE body, and the
rollout kernel's action block is the function sample_actions.  (That the machine code of every kernel outside ks_rollout stayed
what it was is checked with tools/isa_digest.py; that ks_rollout kept its bits, by tests/test_gpu_rollout_bits.py.)"""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tdmpc2_amd", "csrc")


def _src():
    return open(os.path.join(CSRC, "fused_kernels.cuh")).read()


def test_epi_t_is_its_three_pieces_in_a_row():
    """one body for the math: the pieces are epi_t with a piece mask, and the whole epilogue is all three around its one barrier"""
    src = _src()
    assert "enum { EPI_PRE = 1, EPI_MATH = 2, EPI_STORE = 4, EPI_ALL = 7 };" in src
    for piece, mask in (("epi_pre", "EPI_PRE"), ("epi_math", "EPI_MATH"), ("epi_store", "EPI_STORE")):
        i = src.index(f"__device__ __forceinline__ void {piece}(")
        body = src[i:src.index("\n}\n", i)]
        assert re.search(rf"epi_t<\w+, CT, true, {mask}>\(", body), piece
    i = src.index("__device__ __forceinline__ void epi_t(")
    body = src[i:src.index("\n}\n", i)]
    order = [body.index("if constexpr (PIECES & EPI_PRE)"), body.index("if constexpr (PIECES == EPI_ALL)"),
             body.index("if constexpr (PIECES & EPI_MATH)"), body.index("if constexpr (PIECES & EPI_STORE)")]
    assert order == sorted(order)
    assert body.count("__syncthreads()") == 1  # the statistics barrier, only in the whole epilogue
    barrier = body[order[1]:order[2]]
    assert "__syncthreads()" in barrier
    # every caller of the whole epilogue still gets all three pieces: nobody passes a mask but the three wrappers
    assert len(re.findall(r"epi_t<[^>]*EPI_(?:PRE|MATH|STORE)>", src)) == 3


def test_the_rollout_samples_its_actions_through_one_function():
    src = _src()
    i = src.index("__global__ __launch_bounds__(64 * NW, 2) void ks_rollout(")
    kernel = src[i:src.index("\n}\n", i)]
    assert kernel.count("sample_actions(c, p, e, row0, mask, sm_mean, sm_std, t);") == 1
    assert "rng_normal2(" not in kernel and "put_action(" not in kernel  # the block moved, it was not copied
    j = src.index("__device__ __forceinline__ void sample_actions(")
    fn = src[j:src.index("\n}\n", j)]
    for text in ("for (int idx = tid; idx < TROWS * hp; idx += NTHR)", "rng_normal2(p.seed, p.call, SITE_SAMPLE, p.iter, e, pair, z[0], z[1]);",
                 "put_action(c, row, a, v[u]);"):
        assert text in fn, text
