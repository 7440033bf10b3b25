"""CPU: the C ABI of the 16-bit-selector path (include/maxk_hip.h, x16): the entries exist, the
workspace queries are positive and non-decreasing in num_e, and the shape range
1 <= D <= 1024, 1 <= k <= min(D, 256) is enforced on the host, before any pointer is used."""
import pytest

from maxk_cuda_kernels import _capi

FWD, BWD = "maxk_spgemm_forward_x16", "maxk_sspmm_backward_x16"
ENTRIES = ("maxk_topk_cbsr_x16", "maxk_topk_backward_x16", FWD, BWD)


@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def call(lib, name, D, k):
    """The entry on an empty problem (no rows, no edges, NULL pointers) of width D, k winners."""
    n_ptr = _capi.SIGNATURES[name][1].index(_capi._i64)
    if name == "maxk_topk_cbsr_x16":
        return lib.maxk_topk_cbsr_x16(None, D, None, None, None, 0, D, k, None)
    if name == "maxk_topk_backward_x16":
        return lib.maxk_topk_backward_x16(None, None, None, None, 0, D, k, None)
    return getattr(lib, name)(*[None] * n_ptr, 0, 0, 0, D, k, 0, None, 0, None)


def test_entries_exist(lib):
    import maxk_cuda_kernels as mk
    for name in ENTRIES + (FWD + "_workspace_size", BWD + "_workspace_size"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES, name
    for name in ("topk_cbsr_x16", "topk_cbsr_dense_x16", "topk_backward_x16",
                 "spgemm_forward_x16", "sspmm_backward_x16"):
        assert callable(getattr(mk, name)) and name in mk.__all__
    assert mk.MAX_DIM_X16 == 1024


@pytest.mark.parametrize("name", (FWD, BWD))
@pytest.mark.parametrize("chunk", (0, 64))
def test_workspace_sizes(lib, name, chunk):
    size = getattr(lib, name + "_workspace_size")
    assert size(5, 5, 0, 1024, 256, chunk) > 0  # the largest shape is accepted
    for D, k in ((384, 32), (1024, 256), (100, 10)):
        sizes = [size(1000, 1000, e, D, k, chunk) for e in range(0, 400000, 997)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), (D, k)


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("D,k", [(1025, 32), (384, 257), (100, 101), (384, 0), (0, 1)])
def test_range_is_refused(lib, name, D, k):
    assert call(lib, name, D, k) == -1
    msg = lib.maxk_last_error().decode()
    assert "[1,1024]" in msg or "min(dim_origin,256)" in msg, msg
    if name in (FWD, BWD):
        assert getattr(lib, name + "_workspace_size")(10, 10, 10, D, k, 0) == 0


@pytest.mark.parametrize("D", [7, 100, 256])
def test_reference_ranking_matches_oracle(D):
    """x16_ref.topk, the reference of the hard-row tests (tests/topk_rows.py), against the C
    oracle where the oracle reaches: values and columns bitwise, at every k of the sweep."""
    import numpy as np

    import oracle as O
    import topk_rows as TR
    import x16_ref as XR
    x, names = TR.rows(D, np.random.default_rng(5000 + D), names=True)
    assert len(names) == len(x) >= 48 and len(TR.finite(x)) >= 30
    for k in TR.x16_ks(D):
        val, idx = XR.topk(x, k)
        oval, oidx = O.topk(x, k)
        assert np.array_equal(idx, oidx.astype(np.int64)), (D, k)
        assert np.array_equal(val.view(np.uint32), oval.view(np.uint32)), (D, k)


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("D,k", [(1024, 256), (257, 1), (7, 7)])
def test_range_is_accepted(lib, name, D, k):
    assert call(lib, name, D, k) == 0, lib.maxk_last_error().decode()
