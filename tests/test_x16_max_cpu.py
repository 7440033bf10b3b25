"""CPU: the C ABI of the max aggregation on 16-bit selectors (include/maxk_hip.h, x16 max
aggregation): the entries are declared, exported and bound; the shape range, null buffers and a
short workspace are refused on the host, before any launch; the workspace queries equal their
documented formulas and never shrink with more edges.  No kernel is launched."""
import ctypes
import os

import pytest
import torch

from conftest import PKG
from test_boundary_cpu import declared_symbols

FWD, BWD = "maxk_spgemm_max_forward_x16", "maxk_spgemm_max_backward_x16"
P = ctypes.c_void_p(4096)  # a fake non-null, 256-B aligned device pointer: never dereferenced


@pytest.fixture(scope="module")
def lib():
    from maxk_cuda_kernels import _capi
    return _capi.load()


def call(lib, name, shape, p=P, ws=P, ws_bytes=0):
    """shape = (rows, cols, e, D, k, chunk); ws_bytes = 0 stops a call that passes every other
    check at the workspace check."""
    from maxk_cuda_kernels import _capi
    n_ptr = _capi.SIGNATURES[name][1].index(_capi._i64)
    return getattr(lib, name)(*[p] * n_ptr, *shape, ws, ws_bytes, None)


def al256(n):
    return (n + 255) // 256 * 256


def test_symbols_declared_exported_and_bound():
    import maxk_cuda_kernels as mk
    from maxk_cuda_kernels import _capi
    syms = declared_symbols()
    so = ctypes.CDLL(os.path.join(PKG, "lib", "libmaxk_hip.so"))
    for s in (FWD, BWD, FWD + "_workspace_size", BWD + "_workspace_size"):
        assert s in syms and hasattr(so, s) and s in _capi.SIGNATURES, s
    for name in ("spgemm_max_forward_x16", "spgemm_max_backward_x16"):
        assert callable(getattr(mk, name)) and name in mk.__all__


@pytest.mark.parametrize("name", (FWD, BWD))
def test_host_side_validation(lib, name):
    size = getattr(lib, name + "_workspace_size")
    for D, k, word in ((1025, 32, b"dim_origin"), (384, 257, b"dim_k"), (100, 101, b"dim_k"),
                       (384, 0, b"dim_k"), (0, 1, b"dim_origin")):
        assert call(lib, name, (10, 10, 5, D, k, 0)) == -1, (D, k)
        assert word in lib.maxk_last_error()
        assert size(10, 10, 5, D, k, 0) == 0
    assert call(lib, name, (10, 10, 5, 384, 16, 0), p=None) == -1  # null buffers, num_e > 0
    assert b"NULL" in lib.maxk_last_error()
    for D, k in ((1024, 256), (384, 16), (257, 3), (7, 7)):  # accepted up to the workspace
        shape = (10, 10, 5, D, k, 0)
        n = size(*shape)
        assert n > 0 and n % 256 == 0
        for short in (0, n - 1):
            assert call(lib, name, shape, ws_bytes=short) == -1
            assert b"workspace too small" in lib.maxk_last_error()
    assert call(lib, name, (10, 10, 5, 384, 16, 0), ws=ctypes.c_void_p(4096 + 16),
                ws_bytes=1 << 42) == -1
    assert b"256-B aligned" in lib.maxk_last_error()
    assert call(lib, name, (0, 0, 0, 1024, 256, 0), p=None, ws=None) == 0  # an empty problem
    assert lib.maxk_last_error() == b""


@pytest.mark.parametrize("D,k,RS", [(384, 16, 128), (1024, 256, 1536), (257, 3, 32), (100, 10, 64)])
def test_workspace_formulas(lib, D, k, RS):
    """Forward at a forced item size: records + two key rows and two row names per item, each
    part rounded up to 256 B.  Backward: maxk_sspmm_backward_x16's (the csc contribution rows)."""
    fsize, bsize = getattr(lib, FWD + "_workspace_size"), getattr(lib, BWD + "_workspace_size")
    R, C = 1000, 700
    for E in (0, 5000, 123457):
        for chunk in (64, 1000):
            cap = max(1, -(-(R + E) // chunk))
            assert fsize(R, C, E, D, k, chunk) == \
                al256(C * RS) + al256(cap * 2 * 8 * D) + 2 * al256(cap * 4)
        for chunk in (0, 64):
            assert bsize(R, C, E, D, k, chunk) == \
                lib.maxk_sspmm_backward_x16_workspace_size(R, C, E, D, k, chunk)
            assert bsize(R, C, E, D, k, chunk) >= 4 * (E + 1) * k
    # the auto items: key rows within max(the record table, 32 MiB), whatever the edge count
    for E in (10 ** 6, 10 ** 8, 2 ** 31 - 2):
        assert fsize(R, C, E, D, k, 0) <= al256(C * RS) + (32 << 20) + 2 * al256(4 * (32 << 20))


@pytest.mark.parametrize("chunk", [0, 64])
def test_workspace_query_monotone_in_edges(lib, chunk):
    es = sorted(set([0, 1, 63, 64, 65, 5000] + list(range(0, 400000, 997))
                    + [int(10 ** (4 + i * 5.33 / 200)) for i in range(200)] + [2 ** 31 - 2]))
    for D, k in ((384, 32), (1024, 256), (100, 10)):
        for name in (FWD, BWD):
            sizes = [getattr(lib, name + "_workspace_size")(1000, 1000, e, D, k, chunk) for e in es]
            assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), (name, D, k)


def test_binding_refuses_cpu_tensors():
    import maxk_cuda_kernels as mk
    import maxk_spgemm_function as MF
    rp = torch.tensor([0, 2, 3], dtype=torch.int32)
    col = torch.tensor([0, 1, 1], dtype=torch.int32)
    cv, ci = torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int16)
    arg, x = torch.zeros(2, 384, dtype=torch.int32), torch.zeros(2, 384)
    for f in (lambda: mk.spgemm_max_forward_x16(rp, col, cv, ci, 384),
              lambda: mk.spgemm_max_backward_x16(rp, col, ci, arg, x, 3),
              lambda: MF.maxk_spgemm_max(rp, col, cv, ci, 384)):
        with pytest.raises(RuntimeError, match="must be CUDA tensor"):
            f()
