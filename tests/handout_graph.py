"""The hand-out graph of test_handout_gpu.py and test_partition_cpu.py (a helper, like numerics.py):
its rows are listed in test_handout_gpu.py's docstring."""
import functools

import numpy as np

R = 260
HUB_ROW, LAST_TOKEN_ROW, NEXT_ITEM_ROW = 147, 146, 148


def handout_degrees():
    rng = np.random.default_rng(909)
    deg = np.zeros(R, np.int64)
    deg[:140] = rng.integers(0, 3, 140)
    deg[1] = 0
    deg[[62, 63, 64]] = (2, 1, 2)
    deg[[125, 126, 127]] = (1, 2, 1)
    deg[140], deg[141] = 64, 65
    # rows 142..145 bring row 146's token to 511
    room = 511 - (142 + int(deg[:142].sum())) - 4
    assert room >= 4
    deg[142:146] = room // 4
    deg[142:142 + room % 4] += 1
    deg[LAST_TOKEN_ROW] = 5
    deg[HUB_ROW] = 2047 - (511 + 1 + 5)  # its token is 517, its last edge's 2047
    deg[NEXT_ITEM_ROW] = 3
    deg[149:250] = rng.integers(0, 4, 101)
    deg[149] += int(deg.sum()) % 2  # an even number of stubs
    return deg


@functools.lru_cache(maxsize=None)
def handout_csr():
    deg = handout_degrees()
    rng = np.random.default_rng(910)
    stubs = rng.permutation(np.repeat(np.arange(R), deg))
    a, b = stubs[0::2], stubs[1::2]
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    order = np.lexsort((dst, src))
    rp = np.zeros(R + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=R), out=rp[1:])
    return rp.astype(np.int32), dst[order].astype(np.int32)
