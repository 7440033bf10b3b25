"""CPU guard of the later-rounds tests (tests/test_rounds_gpu.py).

Four kernels walk their work in grid-stride rounds and carry state from one round to the next:
linear_maxk_kernel (the cross-tile prefetch, the epilogue tile aliasing the slab buffer),
x16_topk_kernel (the next row's loads), x16_scatter_kernel (an LDS row per wave) and
x16_pack_kernel (s_bits / s_dup).  The GPU file sizes its inputs by the formulas below from the
grid caps parsed out of csrc/, so that every workgroup runs two full rounds and some a third;
here the constants are held to the values the formulas were written for, and the formulas to
that property: a retune fails here instead of silently un-reaching the loops.
"""
import functools

import pytest

import variant_cases as VC

TOPK_SHAPES = [(100, 10), (257, 33), (1024, 256)]            # (D, k) of the x16 encode
PACK_SHAPES = [(1024, 256, 1), (512, 96, 2), (257, 3, 64)]   # (D, k, vertices per pass group)
LM_SHAPES = [(36, 256, 32), (33, 256, 49), (36, 256, 48), (33, 100, 10), (36, 64, 64)]  # I, D, k


@functools.lru_cache(maxsize=None)
def K():
    k = dict(VC.constants())
    k["kWavesPerBlock"] = k["kBlock"] // k["kWave"]
    return k


def lm_tile_rows():
    return K()["kLmWaveRows"] * K()["kWavesPerBlock"]


def lm_sizes(cus):
    """(slots, n_tiles, V) of the fused layer: two full rounds of the grid of `slots`
    workgroups, three more tiles, the last of them 37 rows."""
    slots = K()["MAXK_LM_WGS_PER_CU"] * cus
    n_tiles = 2 * slots + 3
    return slots, n_tiles, lm_tile_rows() * (n_tiles - 1) + 37


def topk_round_rows():
    """Rows per round of x16_topk_kernel and x16_scatter_kernel: one row per wave."""
    return K()["MAXK_TOPK_BLOCKS"] * K()["kWavesPerBlock"]


def topk_rows_total(tail):
    """Two full rounds, 100 full workgroups of a third and one with `tail` live waves."""
    return 2 * topk_round_rows() + K()["kWavesPerBlock"] * 100 + tail


def pack_vpb(k):
    return min(K()["kX16PackMaxV"], K()["kX16PackBlock"] // k)


def pack_round_cols(k):
    return K()["MAXK_PACK_GRID"] * pack_vpb(k)


def pack_cols_total(k):
    return 2 * pack_round_cols(k) + 3


def test_constants():
    k = K()
    assert k["MAXK_TOPK_BLOCKS"] == 16384 and k["MAXK_PACK_GRID"] == 4096
    assert k["MAXK_LM_WGS_PER_CU"] == 2 and lm_tile_rows() == 64
    assert k["kX16PackBlock"] == 256 and k["kX16PackMaxV"] == 64
    assert k["kWavesPerBlock"] == 4 and topk_round_rows() == 65536


@pytest.mark.parametrize("cus", [1, 8, 64, 256, 304])
def test_fused_layer_reaches_a_third_round(cus):
    slots, n_tiles, V = lm_sizes(cus)
    tile = lm_tile_rows()
    assert -(-V // tile) == n_tiles > 2 * slots and 0 < V % tile < tile
    assert V > 2 * slots * tile                 # two full rounds ...
    assert n_tiles - 2 * slots == 3             # ... and a third that 3 workgroups start
    if cus == 256:
        assert V == 64 * 1026 + 37


@pytest.mark.parametrize("tail", [1, 2, 3])
def test_encode_reaches_a_third_round(tail):
    V, rnd, w = topk_rows_total(tail), topk_round_rows(), K()["kWavesPerBlock"]
    assert -(-V // w) > K()["MAXK_TOPK_BLOCKS"]  # the grid is capped
    assert 2 * rnd < V < 3 * rnd and V % w == tail and 0 < tail < w
    assert V * 1024 * 4 < 1 << 30                # the widest input stays below 1 GiB


@pytest.mark.parametrize("D,k,vpb", PACK_SHAPES)
def test_pack_reaches_a_third_round(D, k, vpb):
    assert pack_vpb(k) == vpb
    C, rnd = pack_cols_total(k), pack_round_cols(k)
    assert -(-C // vpb) > K()["MAXK_PACK_GRID"]  # the grid is capped
    assert 2 * rnd < C < 3 * rnd and C - 2 * rnd == 3
    assert C * k < 1 << 31                       # the binding's num_cols * k limit
