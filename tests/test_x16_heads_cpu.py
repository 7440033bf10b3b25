"""CPU: the C ABI of the multi-head 16-bit-selector entries (include/maxk_hip.h, x16 multi-head
aggregation): they exist and are bound, the shape range 1 <= D <= 1024, 1 <= k <= min(D, 256),
1 <= H <= MAXK_MAX_HEADS is enforced on the host before any pointer is used, and the workspace
queries are positive and non-decreasing in num_e."""
import pytest

from maxk_cuda_kernels import _capi

ENTRIES = ("maxk_spgemm_forward_heads_x16", "maxk_edge_weight_grad_heads_x16",
           "maxk_sspmm_backward_heads_x16")
MAX_HEADS = 8


@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def call(lib, name, D, k, H):
    """The entry on an empty problem (no rows, no edges, NULL pointers)."""
    n_ptr = _capi.SIGNATURES[name][1].index(_capi._i64)
    return getattr(lib, name)(*[None] * n_ptr, 0, 0, 0, D, k, H, 0, None, 0, None)


def test_symbols_declared_exported_and_bound(lib):
    import maxk_cuda_kernels as mk
    for name in ENTRIES:
        for sym in (name, name + "_workspace_size"):
            assert hasattr(lib, sym) and sym in _capi.SIGNATURES, sym
        assert callable(getattr(mk, name[len("maxk_"):])) and name[len("maxk_"):] in mk.__all__
    assert mk.MAX_HEADS == MAX_HEADS


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("D,k,H", [(1025, 32, 2), (384, 257, 2), (384, 0, 2), (384, 16, 0),
                                   (384, 16, MAX_HEADS + 1)])
def test_range_is_refused(lib, name, D, k, H):
    assert call(lib, name, D, k, H) == -1
    msg = lib.maxk_last_error().decode()
    assert "[1,1024]" in msg or "min(dim_origin,256)" in msg or "num_heads must be in [1,8]" in msg
    assert ("num_heads" in msg) == (D == 384 and k == 16), msg
    assert getattr(lib, name + "_workspace_size")(10, 10, 10, D, k, H, 0) == 0


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("D,k,H", [(1024, 256, 8), (257, 1, 1), (7, 7, 3)])
def test_range_is_accepted(lib, name, D, k, H):
    assert call(lib, name, D, k, H) == 0, lib.maxk_last_error().decode()


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("chunk", (0, 64))
def test_workspace_sizes(lib, name, chunk):
    size = getattr(lib, name + "_workspace_size")
    assert size(5, 5, 0, 1024, 256, 8, chunk) > 0  # the largest shape is accepted
    for D, k, H in ((384, 32, 3), (1024, 256, 8), (100, 10, 1)):
        sizes = [size(1000, 1000, e, D, k, H, chunk) for e in range(0, 400000, 997)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), (D, k, H)
