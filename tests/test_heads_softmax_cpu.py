"""CPU: the multi-head GAT edge softmax's reference helper, its C ABI surface, host validation
and the routing rule.

tests/heads_softmax_ref.py is the yardstick of test_heads_softmax_gpu.py, so it is pinned here
against torch autograd of a multi-head PyTorch composition on a CSR (scores [H, V], one
leaky_relu, a scatter_reduce(amax) and an index_add_ per head dimension at once) in float64, on
a small graph with an empty row, a hub and an unread column.  No kernel is launched."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import heads_softmax_ref as HS
import numerics as N
from conftest import PKG
from test_boundary_cpu import declared_symbols

FWD = "maxk_gat_edge_softmax_heads"
BWD = "maxk_gat_edge_softmax_heads_backward"
SYMBOLS = (FWD, BWD, FWD + "_workspace_size", BWD + "_workspace_size")


# ------------------------------------------------------------------------------- the yardstick
def small_graph():
    from test_parity_gpu import rand_graph
    rng = np.random.default_rng(2101)
    rp, col = rand_graph(rng, 40, 5, hubs=((3, 35),), empty=2)
    g = N.make_graph(rng, rp, col, 40, unread=11)
    assert (np.diff(g.rp) == 0).any() and not (g.col == 11).any()
    return g


def composition(rp, col, s_dst, s_src, slope, gw):
    """(w [H, E], grad_s_dst [H, R], grad_s_src [H, C]) of all heads at once, float64."""
    H, R = s_dst.shape
    rows = torch.repeat_interleave(torch.arange(R), torch.from_numpy(np.diff(rp).astype(np.int64)))
    c = torch.from_numpy(col.astype(np.int64))
    sd = torch.from_numpy(s_dst.astype(np.float64)).requires_grad_(True)
    ss = torch.from_numpy(s_src.astype(np.float64)).requires_grad_(True)
    l = torch.nn.functional.leaky_relu(sd[:, rows] + ss[:, c], slope)      # [H, E]
    idx = rows.expand(H, -1)
    m = torch.zeros(H, R, dtype=torch.float64).scatter_reduce(1, idx, l.detach(), "amax",
                                                              include_self=False)
    p = torch.exp(l - m[:, rows])
    s = torch.zeros(H, R, dtype=torch.float64).index_add_(1, rows, p)
    w = p / s[:, rows]
    w.backward(torch.from_numpy(gw.astype(np.float64)))
    return w.detach().numpy(), sd.grad.numpy(), ss.grad.numpy()


@pytest.mark.parametrize("slope", [0.2, 0.0, 1.0])
def test_reference_agrees_with_autograd(slope):
    g = small_graph()
    H = 5
    rng = np.random.default_rng(2102)
    s_dst = rng.standard_normal((H, g.R)).astype(np.float32)
    s_src = rng.standard_normal((H, g.C)).astype(np.float32)
    gw = rng.standard_normal((H, g.col.size)).astype(np.float32)
    f = HS.gat_forward_heads(g.rp, g.col, s_dst, s_src, slope)
    b = HS.backward_heads(g.rp, g.col, f, gw, slope, g.C)
    w, gd, gs = composition(g.rp, g.col, s_dst, s_src, slope, gw)
    assert f.w.shape == f.bound.shape == (H, g.col.size)
    assert b.g_dst.shape == b.g_dst_bound.shape == (H, g.R)
    assert b.g_src.shape == b.g_src_bound.shape == (H, g.C)
    scale = np.abs(gw).max()
    rel = np.abs(f.w - w) / np.maximum(np.abs(w), 1e-30)
    print(f"\nheads_softmax_ref vs autograd, slope {slope}: w {rel.max():.3g}, "
          f"g_dst {np.abs(b.g_dst - gd).max():.3g}, g_src {np.abs(b.g_src - gs).max():.3g}")
    assert rel.max() <= 1e-12
    assert np.abs(b.g_dst - gd).max() <= 1e-12 * scale
    assert np.abs(b.g_src - gs).max() <= 1e-12 * scale
    # structure per head: exact zeros with bound 0 where nothing is added, positive bounds on w
    deg = np.diff(g.rp)
    assert (b.g_dst[:, deg == 0] == 0).all() and (b.g_dst_bound[:, deg == 0] == 0).all()
    assert (b.g_src[:, g.unread] == 0).all() and (b.g_src_bound[:, g.unread] == 0).all()
    assert (f.bound > 0).all()
    # a head of the stack is the single-head reference of its slice, and slicing keeps the first
    import edge_softmax_ref as ER
    one = ER.gat_forward(g.rp, g.col, s_dst[3], s_src[3], slope)
    assert np.array_equal(one.w, f.w[3]) and np.array_equal(one.bound, f.bound[3])
    two = HS.heads_slice(b, 2)
    assert two.g_src.shape == (2, g.C) and len(two.heads) == 2
    assert np.array_equal(two.g_dst, b.g_dst[:2])


# ------------------------------------------------------------------------------- the C ABI
def test_symbols_declared_exported_and_bound():
    from maxk_cuda_kernels import _capi
    syms = declared_symbols()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libmaxk_hip.so"))
    for s in SYMBOLS:
        assert s in syms and hasattr(lib, s) and s in _capi.SIGNATURES, s
    # head-major like every heads entry: num_heads leads the sizes; the size queries take it first
    i32, i64, p, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float
    tail = [i32, i64, i64, i64, i32, p, ctypes.c_size_t, p]
    assert _capi.SIGNATURES[FWD] == (ctypes.c_int, [p] * 4 + [f32, p] + tail)
    assert _capi.SIGNATURES[BWD] == (ctypes.c_int, [p] * 6 + [f32] + [p] * 4 + tail)
    for s in (FWD, BWD):
        assert _capi.SIGNATURES[s + "_workspace_size"] == (ctypes.c_size_t,
                                                           [i32, i64, i64, i64, i32])
    import maxk_cuda_kernels as mk
    for name in ("gat_edge_softmax_heads", "gat_edge_softmax_heads_backward",
                 "heads_softmax_route"):
        assert callable(getattr(mk, name)) and name in mk.__all__
    assert mk.version() == 100  # an addition: the ABI version stays
    import maxk_layers as ML
    assert issubclass(ML.GATEdgeSoftmaxHeads, torch.autograd.Function)


def test_binding_refuses_cpu_tensors(monkeypatch):
    """No fallback: a CPU tensor is an error in the binding, the autograd function and the
    layer helper under either route."""
    import maxk_cuda_kernels as mk
    import maxk_layers as ML
    rp = torch.tensor([0, 2, 3], dtype=torch.int32)
    col = torch.tensor([0, 1, 1], dtype=torch.int32)
    e, v = torch.zeros(2, 3), torch.zeros(2, 2)
    g = ML.CSRGraph(rp, col)
    calls = [lambda: mk.gat_edge_softmax_heads(rp, col, v, v),
             lambda: mk.gat_edge_softmax_heads_backward(rp, col, v, v, e, e),
             lambda: ML.GATEdgeSoftmaxHeads.apply(rp, col, v, v, 0.2)]
    for route in ("heads", "calls"):
        monkeypatch.setenv("MAXK_HEADS_SOFTMAX", route)
        for call_ in calls + [lambda: ML.gat_edge_softmax_heads(g, v, v)]:
            with pytest.raises(RuntimeError, match="must be CUDA tensor"):
                call_()


P = ctypes.c_void_p(4096)  # a fake non-null, 256-B aligned device pointer: never dereferenced


def call(L, name, H, shape, slope=0.2, p=P, ws=P, ws_bytes=1 << 42):
    """The entry `name` with every pointer p: rejected on the host, or not called with a
    launchable shape.  shape = (rows, cols, e, chunk)."""
    if name == FWD:
        return L.maxk_gat_edge_softmax_heads(p, p, p, p, slope, p, H, *shape, ws, ws_bytes, None)
    return L.maxk_gat_edge_softmax_heads_backward(p, p, p, p, p, p, slope, p, p, p, p, H, *shape,
                                                  ws, ws_bytes, None)


@pytest.mark.parametrize("name", [FWD, BWD])
def test_host_side_validation(name):
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    size = getattr(L, name + "_workspace_size")
    for H in (0, 9, -1):  # num_heads outside [1, MAXK_MAX_HEADS]
        assert call(L, name, H, (10, 10, 5, 0)) == -1
        assert b"num_heads must be in [1,8]" in L.maxk_last_error()
        assert call(L, name, H, (10, 10, 0, 0)) == -1  # even without edges
        assert size(H, 10, 10, 5, 0) == 0
    #                        rows cols  e  chunk
    for shape, word in (((-1, 10, 5, 0), b"num_rows"), ((10, -1, 5, 0), b"num_cols"),
                        ((10, 10, -5, 0), b"num_e"), ((10, 10, 5, -1), b"chunk_edges")):
        assert call(L, name, 3, shape) == -1, shape  # negative sizes
        assert word in L.maxk_last_error()
        assert size(3, *shape) == 0
    assert call(L, name, 3, (10, 10, 5, 0), p=None) == -1  # null pointers with edges present
    assert b"NULL" in L.maxk_last_error()
    for slope in (-0.1, 1.5, math.nan):
        assert call(L, name, 3, (10, 10, 5, 0), slope=slope) == -1, slope
        assert b"negative_slope must be in [0, 1]" in L.maxk_last_error()
        assert call(L, name, 3, (10, 10, 0, 0), slope=slope) == -1, slope  # even without edges
    assert call(L, name, 3, (0, 0, 5, 0)) == -1  # edges and nothing to hold them
    assert b"edges present" in L.maxk_last_error()
    for H in range(1, 9):  # every value in the range is accepted up to the workspace check
        assert call(L, name, H, (10, 10, 5, 0), ws_bytes=0) == -1
        assert b"workspace too small" in L.maxk_last_error()


def test_no_edges_forward_succeeds():
    """num_e == 0: the forward launches nothing and succeeds, whatever the pointers."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    assert call(L, FWD, 3, (10, 10, 0, 0), p=None, ws=None, ws_bytes=0) == 0
    assert L.maxk_last_error() == b""
    assert call(L, FWD, 8, (0, 0, 0, 64), p=None, ws=None, ws_bytes=0) == 0
    # the backward has both gradients to zero then: a null one is an error
    assert call(L, BWD, 3, (10, 10, 0, 0), p=None, ws=None, ws_bytes=0) == -1
    assert b"grad_s_dst / grad_s_src" in L.maxk_last_error()


SHAPES = [(600, 600, 7000, 0), (600, 600, 7000, 64), (150, 700, 6000, 0), (1, 1, 1, 0),
          (232965, 232965, 114615892, 0), (2449029, 2449029, 123718280, 0)]


@pytest.mark.parametrize("name", [FWD, BWD])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_workspace_query_and_short_workspace(name, shape):
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    size = getattr(L, name + "_workspace_size")
    single = getattr(L, name.replace("_heads", "") + "_workspace_size")(*shape)
    sizes = [size(H, *shape) for H in range(1, 9)]
    assert all(n > 0 and n % 256 == 0 for n in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))  # non-decreasing in H
    rows, cols, e, _ = shape
    assert sizes[0] == single  # one head is the single-head entry
    for H, n in zip(range(1, 9), sizes):
        HP = 2 if H <= 2 else 4 if H <= 4 else 8
        # ss_t, and gzT (past 2^31 bytes at full size)
        need = 0 if H == 1 else 4 * HP * cols + (4 * HP * e if name == BWD else 0)
        assert n >= need and n >= single
        # one byte short: rejected on the host, before anything could be launched (the device
        # pointers are fake: a launch would not return -1 with this message)
        assert call(L, name, H, shape, ws_bytes=n - 1) == -1
        assert b"workspace too small" in L.maxk_last_error()
    n = sizes[4]
    assert call(L, name, 5, shape, ws=None, ws_bytes=n) == -1
    assert b"workspace too small" in L.maxk_last_error()
    assert call(L, name, 5, shape, ws=ctypes.c_void_p(4096 + 16), ws_bytes=n) == -1
    assert b"256-B aligned" in L.maxk_last_error()


@pytest.mark.parametrize("name", [FWD, BWD])
@pytest.mark.parametrize("chunk", [0, 64])
def test_workspace_query_monotone_in_edges(name, chunk):
    """More edges never need less workspace, at 3 and at 8 heads."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    size = getattr(L, name + "_workspace_size")
    es = sorted(set([0, 1, 63, 64, 65, 255, 256, 257, 5000]
                    + list(range(65536 * 256 - 1000, 65536 * 256 + 1000, 97))
                    + [int(x) for x in np.geomspace(1e4, 2 ** 31 - 1, 200)]))
    for H in (3, 8):
        sizes = [size(H, 1000, 1000, e, chunk) for e in es]
        assert all(s > 0 for s in sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:]))


# ------------------------------------------------------------------------------- the route
def test_route_rule_and_switch(monkeypatch):
    import maxk_cuda_kernels as mk
    monkeypatch.delenv("MAXK_HEADS_SOFTMAX", raising=False)
    assert mk.heads_softmax_route(1, 1000, 50000) == "calls"  # one head: nothing to share
    for H in range(2, 9):
        for rows, e in ((232965, 114615892), (2449029, 123718280), (600, 7000)):
            assert mk.heads_softmax_route(H, rows, e) == "heads"  # no threshold: DESIGN.md 5.9
    for forced in ("heads", "calls"):
        monkeypatch.setenv("MAXK_HEADS_SOFTMAX", forced)
        for H in (1, 2, 8):
            assert mk.heads_softmax_route(H, 1000, 50000) == forced
    monkeypatch.setenv("MAXK_HEADS_SOFTMAX", "something else")
    assert mk.heads_softmax_route(1, 1000, 50000) == "calls"
