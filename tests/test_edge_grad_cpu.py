"""CPU: the edge-weight gradient's reference helper, its C ABI surface and host validation.

tests/edge_grad_ref.py is the yardstick of test_edge_grad_gpu.py (the CPU oracle has no such
function), so it is pinned here against torch autograd on a dense float64 restatement of the
forward: A built from the CSR with values.requires_grad, ((A @ scatter(cbsr)) / div).backward(G).
No kernel is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import edge_grad_ref as R
from conftest import GOLDEN, PKG, load_golden
from test_boundary_cpu import declared_symbols

SYMBOLS = ("maxk_edge_weight_grad", "maxk_edge_weight_grad_workspace_size")


# ------------------------------------------------------------------------------- the yardstick
def autograd_edge_grad(rp, col, ev, cv, ci, G, div, D):
    """d <(A @ scatter(cbsr)) / div, G> / d values, dense, float64."""
    R_, C = rp.size - 1, cv.shape[0]
    rows = torch.from_numpy(R.edge_rows(rp))
    w = torch.from_numpy(ev.astype(np.float64)).requires_grad_(True)
    A = torch.zeros(R_, C, dtype=torch.float64).index_put(
        (rows, torch.from_numpy(col.astype(np.int64))), w, accumulate=True)
    X = np.zeros((C, D), np.float64)
    for c in range(C):
        for l in range(ci.shape[1]):
            if ci[c, l] < D:
                X[c, ci[c, l]] += np.float64(cv[c, l])
    out = (A @ torch.from_numpy(X)) / torch.from_numpy(div.astype(np.float64))[:, None]
    out.backward(torch.from_numpy(G.astype(np.float64)))
    return w.grad.numpy()


def rect_problem():
    """40 x 70, an empty row, a vertex with a repeated selector and one with a selector >= D."""
    from test_parity_gpu import rand_graph
    rng = np.random.default_rng(4070)
    D, k = 24, 6
    rp, col = rand_graph(rng, 40, 9, empty=1, cols=70)
    assert (np.diff(rp) == 0).any()
    ev = rng.uniform(0.5, 1.5, col.size).astype(np.float32)
    cv = rng.standard_normal((70, k)).astype(np.float32)
    ci = np.stack([rng.choice(D, k, replace=False) for _ in range(70)]).astype(np.uint8)
    read = np.unique(col)
    a, b = int(read[0]), int(read[1])
    ci[a, 3] = ci[a, 0]  # a repeated selector
    ci[b, 2] = 200       # a selector >= D
    G = rng.standard_normal((40, D)).astype(np.float32)
    div = np.maximum(np.diff(rp), 1).astype(np.float32)
    return rp, col, ev, cv, ci, G, div, D


def tiny_problem():
    z = load_golden(os.path.join(GOLDEN, "tiny_d64_k4.npz"))
    return (z["row_ptr"], z["col_idx"], z["val"], z["topk_val"], z["topk_idx"], z["g"], z["deg"],
            int(z["D"]))


@pytest.mark.parametrize("problem", [tiny_problem, rect_problem], ids=["tiny_d64_k4", "rect40x70"])
def test_reference_agrees_with_autograd(problem):
    rp, col, ev, cv, ci, G, div, D = problem()
    er = R.edge_grad_ref(rp, col, cv, ci, G, div)
    ag = autograd_edge_grad(rp, col, ev, cv, ci, G, div, D)
    assert er.ref.shape == ag.shape == (col.size,)
    rel = np.abs(er.ref - ag) / np.maximum(np.abs(ag), np.finfo(np.float64).tiny)
    rel = np.where(er.ref == ag, 0.0, rel)
    print(f"\nedge_grad_ref vs autograd: max relative difference {rel.max():.3g}")
    assert rel.max() <= 1e-12
    # n counts the selectors below D; an edge into the vertex with one >= D has one fewer
    k = ci.shape[1]
    assert np.array_equal(er.n, (ci[col] < D).sum(1)) and er.n.max() == k
    assert (er.s_abs >= np.abs(er.ref) * (1 - 1e-12)).all()
    b = R.bound(er)
    assert b.shape == er.ref.shape and (b[er.n > 0] > 0).all() and (b[er.n == 0] == 0).all()


def test_reference_without_division_and_n0():
    """div=None leaves the sums undivided; a vertex whose selectors are all >= D gives n = 0,
    reference 0 and bound 0 -- even with NaN values behind them."""
    rp, col, ev, cv, ci, G, div, D = rect_problem()
    c0 = int(col[0])
    ci, cv = ci.copy(), cv.copy()
    ci[c0], cv[c0] = 250, np.nan
    a = R.edge_grad_ref(rp, col, cv, ci, G, div)
    b = R.edge_grad_ref(rp, col, cv, ci, G, None)
    rows = R.edge_rows(rp)
    assert np.allclose(a.ref * div[rows], b.ref, rtol=1e-14, atol=0)
    hit = col == c0
    assert hit.any() and (a.n[hit] == 0).all() and (a.ref[hit] == 0).all()
    assert (R.bound(a)[hit] == 0).all() and np.isfinite(a.ref).all()


# ------------------------------------------------------------------------------- the C ABI
def test_symbols_declared_exported_and_bound():
    from maxk_cuda_kernels import _capi
    syms = declared_symbols()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libmaxk_hip.so"))
    for s in SYMBOLS:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert s in _capi.SIGNATURES, s
    import maxk_cuda_kernels as mk
    assert callable(mk.edge_weight_grad)
    assert mk.version() == 100  # an addition: the ABI version stays


def call(L, *shape, ws=None, ws_bytes=0, ptr=16):
    """maxk_edge_weight_grad with fake non-null device pointers: rejected on the host or not
    called with a launchable shape."""
    p = ctypes.c_void_p(ptr)
    return L.maxk_edge_weight_grad(p, p, p, p, p, None, p, *shape, ws, ws_bytes, None)


def test_host_side_validation():
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    #               rows cols  e   D   k  chunk
    assert call(L, 10, 10, 5, 64, 0, 0) == -1      # k = 0
    assert b"dim_k" in L.maxk_last_error()
    assert call(L, 10, 10, 5, 64, 65, 0) == -1     # k > D
    assert b"dim_k" in L.maxk_last_error()
    for D in (257, 258):                           # D past the uint8 selector range
        assert call(L, 10, 10, 5, D, 16, 0) == -1
        assert b"dim_origin" in L.maxk_last_error()
    assert call(L, -1, 10, 5, 64, 16, 0) == -1     # negative sizes
    assert call(L, 10, 10, -5, 64, 16, 0) == -1
    assert call(L, 10, 10, 5, 64, 16, -1) == -1
    # null pointers with edges present
    assert L.maxk_edge_weight_grad(None, None, None, None, None, None, None, 10, 10, 5, 64, 16,
                                   0, None, 0, None) == -1
    assert b"NULL" in L.maxk_last_error()
    # num_e == 0 launches nothing and succeeds, whatever the pointers
    assert L.maxk_edge_weight_grad(None, None, None, None, None, None, None, 10, 10, 0, 64, 16,
                                   0, None, 0, None) == 0
    assert L.maxk_last_error() == b""
    # range errors are reported even then
    assert L.maxk_edge_weight_grad(None, None, None, None, None, None, None, 10, 10, 0, 64, 65,
                                   0, None, 0, None) == -1


@pytest.mark.parametrize("shape", [(1000, 1000, 100000, 256, 16, 0), (150, 700, 6000, 9, 7, 64),
                                   (400, 400, 64000, 256, 96, 0), (600, 600, 7000, 64, 3, 0)])
def test_workspace_query_and_short_workspace(shape):
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    n = L.maxk_edge_weight_grad_workspace_size(*shape)
    assert n > 0 and n % 256 == 0
    k, cols = shape[4], shape[1]
    assert n >= cols * 6 * k  # one record [k f32 | k u16] per column
    # one byte short: rejected on the host, before anything could be launched (the device
    # pointers are fake: a launch would not return -1 with this message)
    ws = ctypes.c_void_p(4096)
    assert call(L, *shape, ws=ws, ws_bytes=n - 1) == -1
    assert b"workspace too small" in L.maxk_last_error()
    assert call(L, *shape, ws=None, ws_bytes=n) == -1
    assert b"workspace too small" in L.maxk_last_error()
    assert call(L, *shape, ws=ctypes.c_void_p(4096 + 16), ws_bytes=n) == -1
    assert b"256-B aligned" in L.maxk_last_error()
    assert L.maxk_edge_weight_grad_workspace_size(-1, 10, 5, 64, 16, 0) == 0
    assert L.maxk_edge_weight_grad_workspace_size(10, 10, 5, 64, 0, 0) == 0
