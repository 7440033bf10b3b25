"""CPU: the group rule of the stream pull backward (maxk_pull_stream_buckets, include/maxk_hip.h).

The rule is a host function and needs no device when the CU count is passed.  It decides the
number of buckets; the bucket boundaries themselves are chosen on the GPU by the plan call from
the graph's in-degrees, so their properties (increasing, covering [0, num_cols), every width
<= cap) are checked against the built plan in test_pull_stream_gpu.py.  What can be checked
here is what makes such boundaries exist: n_buckets * cap >= num_cols.

The stream entry point takes no tile list, no accumulate flag and no MAXK_PULL_NO_REDUCE /
MAXK_PULL_REDUCE_ONLY: the hybrid's listed tiles keep calling maxk_sspmm_backward_pull_tiles.
"""
import ctypes

import pytest

REDDIT = (232965, 114615892)
NARROW = 0.125  # include/maxk_hip.h: the mean bucket may shrink by at most 12.5 %
LDS = 160 * 1024


@pytest.fixture(scope="module")
def L():
    from maxk_cuda_kernels import _capi
    return _capi.load()


def parts(k, shift):
    """pull_parts restated: the fewest H (k % (4H) == 0) whose kp = k / H fp64 slots and kp
    selector bytes per destination fit the LDS at 2^shift destinations."""
    H = 1
    while H <= k // 4 and k % (4 * H) == 0:
        if ((k // H) * 8 + k // H) << shift <= LDS:
            return H
        H *= 2
    return 0


def test_reddit_k8_refused_k16_accepted(L):
    V, E = REDDIT
    assert L.maxk_pull_stream_buckets(V, V, E, 256, 8, 256) == 0  # 114 groups: 256 would halve them
    assert L.maxk_pull_stream_buckets(V, V, E, 256, 16, 256) == 128  # 228 groups -> one round of 256
    assert L.maxk_pull_shift(16) == 11 and parts(16, 11) == 2


@pytest.mark.parametrize("cus", [64, 104, 228, 256, 304])
@pytest.mark.parametrize("k", [4, 8, 12, 16, 32, 64, 128, 256])
def test_rule_over_a_grid(L, k, cus):
    shift = L.maxk_pull_shift(k)
    cap, H = 1 << shift, parts(k, shift)
    assert H > 0
    for num_cols in [1, 700, cap, cap + 1, 20000, 89250, 132534, 232965, 500000, 1 << 20]:
        nb = L.maxk_pull_stream_buckets(num_cols, num_cols, 10 * num_cols, 256, k, cus)
        nb_min = -(-num_cols // cap)
        rounds = -(-nb_min * H // cus)
        if nb == 0:  # refused: whole rounds would narrow the mean bucket too much
            want = rounds * cus // H
            assert want < nb_min or (want - nb_min) > NARROW * want, (num_cols, k, cus)
            continue
        assert nb == rounds * cus // H
        assert nb * cap >= num_cols                      # boundaries with widths <= cap exist
        assert nb - nb_min <= NARROW * nb                # the mean width num_cols / nb
        assert nb * H <= rounds * cus < nb * H + H       # whole rounds of one workgroup per CU


def test_refusals(L):
    V, E = REDDIT
    f = L.maxk_pull_stream_buckets
    assert f(V, V, E, 256, 16, 256) == 128
    assert f(V, V, -1, 256, 16, 256) == 128               # edge count unknown: not checked
    for k in (1, 2, 6, 10, 18):
        assert f(V, V, E, 256, k, 256) == 0               # k % 4 != 0
    assert f(V, V, E, 255, 16, 256) == 0                  # dim_origin % 4 != 0
    assert f(V, V, 1 << 28, 256, 16, 256) == 0            # entry offsets past 32 bits
    # G of 2^31 bytes or more (2^32 included): the gather offsets leave the descriptor's reach
    rows31 = (1 << 31) // (256 * 4)
    assert f(rows31, V, E, 256, 16, 256) == 0 and f(rows31 - 1, V, E, 256, 16, 256) == 128
    assert f((1 << 32) // (256 * 4), V, E, 256, 16, 256) == 0
    # row bits + in-bucket column bits past 32: 2^22 rows need 22 bits, k = 16 has 11 column bits
    assert f((1 << 21) + 1, V, E, 64, 16, 256) == 0 and f(1 << 21, V, E, 64, 16, 256) == 128
    assert f(0, V, E, 256, 16, 256) == 0 and f(V, 0, E, 256, 16, 256) == 0
    assert f(V, V, E, 256, 0, 256) == 0 and f(V, V, E, 8, 16, 256) == 0


def test_binding_covers_the_entry_points():
    from maxk_cuda_kernels import _capi
    p, i32, i64, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    S = _capi.SIGNATURES
    assert S["maxk_pull_stream_buckets"] == (i64, [i64, i64, i64, i32, i32, i32])
    assert S["maxk_sspmm_backward_pull_stream"] == (
        ctypes.c_int, [p] * 6 + [i32, p] + [i64] * 3 + [i32, i32, p, sz, p])
    assert S["maxk_sspmm_backward_pull_stream_workspace_size"] == (sz, [i64, i64, i32, i32])
    assert S["maxk_pull_stream_plan"] == (
        ctypes.c_int, [p] * 3 + [i64] * 3 + [i32] * 3 + [p] * 4 + [sz, p])


def test_workspace_holds_no_tile_partials(L):
    """The stream path's workspace: G / row_div, slot-ordered selectors and their map; the
    tiled pull's adds slices x buckets x cap x k floats of partials."""
    V, _ = REDDIT
    al = lambda x: (x + 255) // 256 * 256  # noqa: E731
    stream = L.maxk_sspmm_backward_pull_stream_workspace_size(V, V, 256, 16)
    assert stream == al(V * 256 * 4) + 2 * al(V * 16)
    S = L.maxk_pull_slices(V, V, 256, 16)
    tiled = L.maxk_sspmm_backward_pull_workspace_size(V, V, 256, 16, S)
    assert tiled - stream == S * 114 * 2048 * 16 * 4
