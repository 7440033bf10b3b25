"""CPU: the multi-head feature backward's C ABI surface (maxk_sspmm_backward_heads), its host
validation with fake pointers -- every rejection comes before any launch -- the workspace query
and the binding's route rule (heads_backward_route).  No kernel is launched.  Mirrors
test_heads_cpu.py, which covers the other two multi-head entries."""
import ctypes
import os

import pytest

from conftest import PKG
from test_boundary_cpu import declared_symbols

NAME = "maxk_sspmm_backward_heads"
SIZE = NAME + "_workspace_size"


@pytest.fixture(scope="module")
def L():
    from maxk_cuda_kernels import _capi
    return _capi.load()


def call(L, *shape, ws=None, ws_bytes=0, ptr=4096):
    """The entry with fake non-null device pointers (row_div NULL): rejected on the host, or not
    called with a launchable shape.  shape = (rows, cols, e, D, k, H, chunk)."""
    p = ctypes.c_void_p(ptr)
    return getattr(L, NAME)(p, p, p, p, None, p, p, p, p, *shape, ws, ws_bytes, None)


def test_symbols_declared_exported_and_bound():
    from maxk_cuda_kernels import _capi
    syms = declared_symbols()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libmaxk_hip.so"))
    for s in (NAME, SIZE):
        assert s in syms, s
        assert hasattr(lib, s), s
        assert s in _capi.SIGNATURES, s
    assert len(_capi.SIGNATURES[NAME][1]) == 19 and len(_capi.SIGNATURES[SIZE][1]) == 7
    import maxk_cuda_kernels as mk
    assert callable(mk.sspmm_backward_heads) and callable(mk.heads_backward_route)
    assert "sspmm_backward_heads" in mk.__all__ and "heads_backward_route" in mk.__all__
    assert mk.version() == 100  # an addition: the ABI version stays


def test_host_side_validation(L):
    #                 rows cols  e   D   k  H chunk
    for H in (0, 9, -1):
        assert call(L, 10, 10, 5, 64, 16, H, 0) == -1
        assert b"num_heads" in L.maxk_last_error()
        assert getattr(L, SIZE)(10, 10, 5, 64, 16, H, 0) == 0
    assert call(L, 10, 10, 5, 64, 65, 3, 0) == -1     # k > D
    assert b"dim_k" in L.maxk_last_error()
    assert call(L, 10, 10, 5, 64, 0, 3, 0) == -1      # k = 0
    assert b"dim_k" in L.maxk_last_error()
    assert call(L, 10, 10, 5, 257, 16, 3, 0) == -1    # D past the uint8 selector range
    assert b"dim_origin" in L.maxk_last_error()
    assert call(L, -1, 10, 5, 64, 16, 3, 0) == -1     # negative sizes
    assert b"num_rows" in L.maxk_last_error()
    assert call(L, 10, -1, 5, 64, 16, 3, 0) == -1
    assert b"num_cols" in L.maxk_last_error()
    assert call(L, 10, 10, -5, 64, 16, 3, 0) == -1
    assert b"num_e" in L.maxk_last_error()
    assert call(L, 10, 10, 5, 64, 16, 3, -1) == -1
    assert b"chunk_edges" in L.maxk_last_error()
    # null pointers: all of them with edges present; the output and col_ptr even without edges
    fn = getattr(L, NAME)
    assert fn(None, None, None, None, None, None, None, None, None, 10, 10, 5, 64, 16, 3, 0,
              None, 0, None) == -1
    assert b"NULL" in L.maxk_last_error()
    assert fn(None, None, None, None, None, None, None, None, None, 10, 10, 0, 64, 16, 3, 0,
              None, 0, None) == -1
    assert b"NULL" in L.maxk_last_error()
    p = ctypes.c_void_p(4096)
    for missing in range(9):
        if missing == 4:  # row_div may be NULL
            continue
        args = [p] * 9
        args[missing] = None
        assert fn(*args, 10, 10, 5, 64, 16, 3, 0, None, 0, None) == -1, missing
        assert b"NULL" in L.maxk_last_error(), missing
    # a table of 2^24 columns or more is rejected, with a message naming the argument
    for cols in (1 << 24, (1 << 24) + 1):
        assert call(L, 10, cols, 5, 64, 16, 3, 0) == -1
        assert b"num_cols" in L.maxk_last_error()


def test_no_columns_returns_ok(L):
    fn = getattr(L, NAME)
    assert fn(None, None, None, None, None, None, None, None, None, 10, 0, 0, 64, 16, 3, 0, None,
              0, None) == 0
    assert L.maxk_last_error() == b""
    # range errors are reported even then
    assert fn(None, None, None, None, None, None, None, None, None, 10, 0, 0, 64, 16, 9, 0, None,
              0, None) == -1
    assert b"num_heads" in L.maxk_last_error()


@pytest.mark.parametrize("shape", [(1000, 1000, 100000, 256, 16, 4, 0),
                                   (150, 700, 6000, 9, 7, 3, 64),
                                   (400, 400, 64000, 256, 96, 8, 0),
                                   (600, 600, 7000, 64, 3, 1, 0),
                                   (600, 600, 0, 64, 8, 2, 64)])
def test_workspace_query_is_the_csc_query_and_short_workspace(L, shape):
    rows, cols, e, D, k, H, chunk = shape
    n = getattr(L, SIZE)(*shape)
    assert n == L.maxk_sspmm_backward_csc_workspace_size(rows, cols, e, D, k, chunk)
    assert n > 0 and n % 256 == 0
    assert n >= (e + 1) * k * 4  # the contribution rows and the dummy row: nothing grows with H
    for other in (1, 8):
        assert getattr(L, SIZE)(rows, cols, e, D, k, other, chunk) == n
    # one byte short: rejected on the host, before anything could be launched (the device
    # pointers are fake: a launch would not return -1 with this message)
    ws = ctypes.c_void_p(1 << 20)
    assert call(L, *shape, ws=ws, ws_bytes=n - 1) == -1
    assert b"workspace too small" in L.maxk_last_error()
    assert call(L, *shape, ws=None, ws_bytes=n) == -1
    assert b"workspace too small" in L.maxk_last_error()
    assert call(L, *shape, ws=ctypes.c_void_p((1 << 20) + 16), ws_bytes=n) == -1
    assert b"256-B aligned" in L.maxk_last_error()
    assert getattr(L, SIZE)(10, -1, 5, 64, 16, 3, 0) == 0
    assert getattr(L, SIZE)(10, 10, 5, 64, 0, 3, 0) == 0


def test_route_rule(monkeypatch):
    """heads_backward_route: MAXK_HEADS_BWD forces a route; a forced MAXK_BWD_MODE (graph_only_mode
    returns None: the forced mode is what H calls run) means "calls"; so does a table the entry
    rejects, even when "heads" is forced.  Unforced, the rule of DESIGN.md 5.8: "heads" whether
    the H calls would run csc or bsort, except for a single head."""
    import maxk_cuda_kernels as mk
    monkeypatch.delenv("MAXK_HEADS_BWD", raising=False)
    monkeypatch.delenv("MAXK_BWD_MODE", raising=False)
    reddit = (16, 114_615_892, 232_965, 232_965)    # (k, num_e, num_cols, num_rows)
    products = (32, 123_718_280, 2_449_029, 2_449_029)
    products8 = (8,) + products[1:]
    assert mk.graph_only_mode(*reddit[:3]) == "csc" and mk.graph_only_mode(*products[:3]) == "csc"
    assert mk.graph_only_mode(*products8[:3]) == "bsort"
    for shape in (reddit, products, products8):
        assert mk.heads_backward_route(*shape) == "heads", shape
        for H in (2, 4, 8):
            assert mk.heads_backward_route(*shape, H) == "heads", shape
        assert mk.heads_backward_route(*shape, 1) == "calls", shape
        assert mk.heads_backward_route(*shape, num_heads=1) == "calls", shape
    for forced in ("heads", "calls"):
        monkeypatch.setenv("MAXK_HEADS_BWD", forced)
        for shape in (reddit, products, products8):
            assert mk.heads_backward_route(*shape) == forced
            assert mk.heads_backward_route(*shape, 1) == forced
        assert mk.heads_backward_route(16, 100, 1 << 24, 50) == "calls"
    monkeypatch.setenv("MAXK_HEADS_BWD", "neither")  # not a route: ignored
    assert mk.heads_backward_route(*reddit) == "heads"
    monkeypatch.delenv("MAXK_HEADS_BWD")
    for mode in ("csc", "atomic", "pull", "bsort"):
        monkeypatch.setenv("MAXK_BWD_MODE", mode)
        assert mk.graph_only_mode(*reddit[:3]) is None
        assert mk.heads_backward_route(*reddit) == "calls", mode
        assert mk.heads_backward_route(*reddit, 8) == "calls", mode
    monkeypatch.setenv("MAXK_BWD_MODE", "auto")
    assert mk.heads_backward_route(*reddit) == "heads"
    assert mk.heads_backward_route(16, 100, 1 << 24, 50) == "calls"
