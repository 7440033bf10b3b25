"""CPU: the fused multi-head GAT attention's reference helper, its C ABI surface, host validation,
the routing rule and the layer's switch.

tests/gat_attention_ref.py is the yardstick of test_gat_attention_gpu.py, so it is pinned here
against float64 torch autograd of a dense composition (leaky_relu of the score sums, a softmax
over each row's neighbours, a matmul with the scattered CBSR) on a small graph with an empty row,
a hub and an unread column, at slopes 0.2, 0 and 1.  No kernel is launched."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import gat_attention_ref as AR
import numerics as N
from conftest import PKG
from test_boundary_cpu import declared_symbols

FWD = "maxk_gat_attention_heads"
ALPHA = "maxk_gat_edge_alpha_heads"
SYMBOLS = (FWD, ALPHA, FWD + "_workspace_size", ALPHA + "_workspace_size")


# ------------------------------------------------------------------------------- the yardstick
def small_problem():
    from test_parity_gpu import rand_graph
    rng = np.random.default_rng(2301)
    rp, col = rand_graph(rng, 40, 5, hubs=((3, 35),), empty=2)
    g = N.make_graph(rng, rp, col, 40, unread=11)
    assert (np.diff(g.rp) == 0).any() and not (g.col == 11).any()
    D, k, H = 24, 5, 5
    ci = N.selectors(rng, g.C, D, k)
    ci[7, 2] = ci[7, 0]   # a repeated selector: both values are added
    ci[9, 1] = D + 3      # a selector past D: adds nothing
    cv = rng.standard_normal((g.C, k)).astype(np.float32)
    s_dst = rng.standard_normal((H, g.R)).astype(np.float32)
    s_src = rng.standard_normal((H, g.C)).astype(np.float32)
    return g, ci, cv, s_dst, s_src, D


def dense_composition(g, ci, cv, s_dst, s_src, D, slope):
    """(out [H, R, D], alpha [H, R, C]) in float64 torch, dense over the adjacency."""
    R, C = g.R, g.C
    A = torch.zeros(R, C, dtype=torch.float64)
    rows = np.repeat(np.arange(R), np.diff(g.rp))
    A[torch.from_numpy(rows), torch.from_numpy(g.col.astype(np.int64))] = 1.0
    X = torch.zeros(C, 256, dtype=torch.float64)
    X.index_put_((torch.arange(C)[:, None].expand(-1, ci.shape[1]),
                  torch.from_numpy(ci.astype(np.int64))),
                 torch.from_numpy(cv.astype(np.float64)), accumulate=True)
    X = X[:, :D]
    sd = torch.from_numpy(s_dst.astype(np.float64))
    ss = torch.from_numpy(s_src.astype(np.float64))
    e = torch.nn.functional.leaky_relu(sd[:, :, None] + ss[:, None, :], slope)
    masked = (A == 0) & (A.sum(1, keepdim=True) > 0)
    alpha = torch.softmax(e.masked_fill(masked, float("-inf")), 2) * A
    return (alpha @ X).numpy(), alpha.numpy()


@pytest.mark.parametrize("slope", [0.2, 0.0, 1.0])
def test_reference_agrees_with_dense_torch(slope):
    g, ci, cv, s_dst, s_src, D = small_problem()
    H = s_dst.shape[0]
    n = N.count_fwd(g, ci, D)
    a = AR.attention(g.rp, g.col, s_dst, s_src, slope, cv, ci, D, n)
    out, alpha = dense_composition(g, ci, cv, s_dst, s_src, D, slope)
    assert a.out.shape == a.out_bound.shape == (H, g.R, D)
    assert a.m.shape == a.m_bound.shape == a.z.shape == a.z_bound.shape == (H, g.R)
    err = np.abs(a.out - out).max()
    print(f"\ngat_attention_ref vs dense torch, slope {slope}: out {err:.3g}")
    assert err <= 1e-12 * max(1.0, np.abs(out).max())
    rows = np.repeat(np.arange(g.R), np.diff(g.rp))
    assert np.abs(a.w - alpha[:, rows, g.col]).max() <= 1e-12
    # the statistics rebuild alpha
    w2 = AR.alpha_from_stats(g.rp, g.col, s_dst, s_src, slope, a.m, a.z)
    assert np.abs(w2 - a.w).max() <= 1e-12
    # structure: exact zeros with bound 0 where nothing is added, positive bounds elsewhere
    deg = np.diff(g.rp)
    assert (a.out[:, deg == 0] == 0).all() and (a.out_bound[:, deg == 0] == 0).all()
    assert (a.m[:, deg == 0] == 0).all() and (a.z[:, deg == 0] == 0).all()
    assert ((a.out_bound > 0) == (n > 0)[None]).all()
    assert ((a.out != 0) <= (n > 0)[None]).all()
    assert (a.z[:, deg > 0] >= 1).all() and (a.z_bound[:, deg > 0] > 0).all()
    # the weight bound is the edge softmax's and 8 u of the weight
    f = a.heads[2]
    assert np.allclose(AR.weight_bound(f) - f.bound, 8 * AR.U * f.w, rtol=1e-12, atol=0)
    two = AR.heads_slice(a, 2)
    assert two.out.shape == (2, g.R, D) and len(two.heads) == 2


def test_reference_non_finite_rules():
    """A NaN score: NaN wherever the row has an addend, 0 elsewhere; a -Inf logit adds exactly
    0; a row of only -Inf is NaN where it has addends; the NaN-ignoring maximum."""
    g, ci, cv, s_dst, s_src, D = small_problem()
    n = N.count_fwd(g, ci, D)
    rows = np.repeat(np.arange(g.R), np.diff(g.rp))
    c_nan = int(g.col[g.rp[g.hub]])
    s_src = s_src.copy()
    s_src[1, c_nan] = np.nan
    a = AR.attention(g.rp, g.col, s_dst, s_src, 0.2, cv, ci, D, n)
    hit = np.unique(rows[g.col == c_nan])
    assert np.isnan(a.out[1, hit][:, :][(n[hit] > 0)]).all()
    assert (a.out[1, hit][(n[hit] == 0)] == 0).all()
    assert np.isfinite(a.out[[0, 2, 3, 4]]).all()
    assert np.isfinite(a.m[1, hit]).all() and np.isnan(a.z[1, hit]).all()
    r = int(np.flatnonzero(np.diff(g.rp) >= 2)[0])
    sd = s_dst.copy()
    sd[0, r] = -np.inf
    b = AR.attention(g.rp, g.col, sd, s_src, 0.2, cv, ci, D, n)
    assert np.isnan(b.out[0, r][n[r] > 0]).all() and (b.out[0, r][n[r] == 0] == 0).all()
    assert np.isneginf(b.m[0, r]) and b.z[0, r] == 0


# ------------------------------------------------------------------------------- the C ABI
def test_symbols_declared_exported_and_bound():
    from maxk_cuda_kernels import _capi
    syms = declared_symbols()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libmaxk_hip.so"))
    for s in SYMBOLS:
        assert s in syms and hasattr(lib, s) and s in _capi.SIGNATURES, s
    i32, i64, p, f32, sz = (ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float,
                            ctypes.c_size_t)
    assert _capi.SIGNATURES[FWD] == (ctypes.c_int, [p] * 4 + [f32] + [p] * 5 + [i64] * 3
                                     + [i32] * 4 + [p, sz, p])
    assert _capi.SIGNATURES[FWD + "_workspace_size"] == (sz, [i64] * 3 + [i32] * 4)
    assert _capi.SIGNATURES[ALPHA] == (ctypes.c_int, [p] * 4 + [f32] + [p] * 3 + [i32]
                                       + [i64] * 3 + [p, sz, p])
    assert _capi.SIGNATURES[ALPHA + "_workspace_size"] == (sz, [i32] + [i64] * 3)
    import maxk_cuda_kernels as mk
    for name in ("gat_attention_heads", "gat_edge_alpha_heads", "heads_attention_route"):
        assert callable(getattr(mk, name)) and name in mk.__all__
    assert mk.version() == 100  # an addition: the ABI version stays
    import maxk_layers as ML
    import maxk_spgemm_function as MF
    assert issubclass(MF.MaxKGATAttentionHeadsFunction, torch.autograd.Function)
    assert callable(MF.maxk_gat_attention_heads) and callable(ML.CSRGraph.attend_heads)


def test_binding_refuses_cpu_tensors(monkeypatch):
    """No fallback: a CPU tensor is an error in the binding, the autograd function, the graph's
    method and the layer under attention="fused"."""
    import maxk_cuda_kernels as mk
    import maxk_layers as ML
    import maxk_spgemm_function as MF
    monkeypatch.delenv("MAXK_HEADS_ATTN", raising=False)
    rp = torch.tensor([0, 2, 3], dtype=torch.int32)
    col = torch.tensor([0, 1, 1], dtype=torch.int32)
    v = torch.zeros(2, 2)
    cv = torch.zeros(2, 3)
    ci = torch.zeros(2, 3, dtype=torch.uint8)
    g = ML.CSRGraph(rp, col)
    conv = ML.MaxKMultiHeadGATConv(4, 3, 2, attention="fused")
    x = torch.zeros(2, 4)
    calls = [lambda: mk.gat_attention_heads(rp, col, v, v, cv, ci, 4),
             lambda: mk.gat_edge_alpha_heads(rp, col, v, v, v, v),
             lambda: MF.maxk_gat_attention_heads(rp, col, v, v, cv, ci, 4),
             lambda: g.attend_heads(cv, ci, 4, v, v),
             lambda: conv(g, x, cv, ci)]
    for call_ in calls:
        with pytest.raises(RuntimeError, match="must be CUDA tensor"):
            call_()


P = ctypes.c_void_p(4096)  # a fake non-null, 256-B aligned device pointer: never dereferenced


def call_fwd(L, H, shape, slope=0.2, p=P, ws=P, ws_bytes=1 << 42):
    """shape = (rows, cols, e, D, k, chunk)."""
    rows, cols, e, D, k, chunk = shape
    return L.maxk_gat_attention_heads(p, p, p, p, slope, p, p, p, p, p, rows, cols, e, D, k, H,
                                      chunk, ws, ws_bytes, None)


def call_alpha(L, H, shape, slope=0.2, p=P, ws=P, ws_bytes=1 << 42):
    """shape = (rows, cols, e)."""
    return L.maxk_gat_edge_alpha_heads(p, p, p, p, slope, p, p, p, H, *shape, ws, ws_bytes, None)


def test_host_side_validation_forward():
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    size = L.maxk_gat_attention_heads_workspace_size
    ok = (10, 10, 5, 64, 8, 0)
    for H in (0, 9, -1):  # num_heads outside [1, MAXK_MAX_HEADS]
        assert call_fwd(L, H, ok) == -1
        assert b"num_heads must be in [1,8]" in L.maxk_last_error()
        assert call_fwd(L, H, (10, 10, 0, 64, 8, 0)) == -1  # even without edges
        assert size(10, 10, 5, 64, 8, H, 0) == 0
    for shape, word in (((-1, 10, 5, 64, 8, 0), b"num_rows"), ((10, -1, 5, 64, 8, 0), b"num_cols"),
                        ((10, 10, -5, 64, 8, 0), b"num_e"),
                        ((10, 10, 5, 64, 8, -1), b"chunk_edges")):
        assert call_fwd(L, 3, shape) == -1, shape  # negative sizes
        assert word in L.maxk_last_error()
        rows, cols, e, D, k, chunk = shape
        assert size(rows, cols, e, D, k, 3, chunk) == 0
    for D, k, word in ((0, 1, b"dim_origin"), (257, 8, b"dim_origin"), (64, 0, b"dim_k"),
                       (64, 65, b"dim_k")):  # k / D range
        assert call_fwd(L, 3, (10, 10, 5, D, k, 0)) == -1, (D, k)
        assert word in L.maxk_last_error()
    assert call_fwd(L, 3, ok, p=None) == -1  # null pointers
    assert b"NULL" in L.maxk_last_error()
    for slope in (-0.1, 1.5, math.nan):
        assert call_fwd(L, 3, ok, slope=slope) == -1, slope
        assert b"negative_slope must be in [0, 1]" in L.maxk_last_error()
        assert call_fwd(L, 3, (10, 10, 0, 64, 8, 0), slope=slope) == -1  # even without edges
    assert call_fwd(L, 3, (10, 0, 5, 64, 8, 0)) == -1  # edges and no column to hold them
    assert b"edges present" in L.maxk_last_error()
    assert call_fwd(L, 3, (10, 1 << 24, 5, 64, 8, 0)) == -1  # a table past 2^24 columns
    assert b"2^24 columns" in L.maxk_last_error()
    for H in range(1, 9):  # every value in the range is accepted up to the workspace check
        for D, k in ((64, 3), (256, 96), (9, 7), (256, 256)):
            assert call_fwd(L, H, (10, 10, 5, D, k, 0), ws_bytes=0) == -1
            assert b"workspace too small" in L.maxk_last_error()


def test_host_side_validation_alpha():
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    size = L.maxk_gat_edge_alpha_heads_workspace_size
    for H in (0, 9, -1):
        assert call_alpha(L, H, (10, 10, 5)) == -1
        assert b"num_heads must be in [1,8]" in L.maxk_last_error()
        assert size(H, 10, 10, 5) == 0
    for shape, word in (((-1, 10, 5), b"num_rows"), ((10, -1, 5), b"num_cols"),
                        ((10, 10, -5), b"num_e")):
        assert call_alpha(L, 3, shape) == -1, shape
        assert word in L.maxk_last_error()
        assert size(3, *shape) == 0
    assert call_alpha(L, 3, (10, 10, 5), p=None) == -1
    assert b"NULL" in L.maxk_last_error()
    for slope in (-0.1, 1.5, math.nan):
        assert call_alpha(L, 3, (10, 10, 5), slope=slope) == -1, slope
        assert b"negative_slope must be in [0, 1]" in L.maxk_last_error()
    assert call_alpha(L, 3, (0, 0, 5)) == -1
    assert b"edges present" in L.maxk_last_error()
    for H in range(1, 9):
        n = size(H, 10, 700, 5)
        HP = 2 if H <= 2 else 4 if H <= 4 else 8
        assert n % 256 == 0 and n >= 4 * HP * 700
        assert call_alpha(L, H, (10, 700, 5), ws_bytes=n - 1) == -1
        assert b"workspace too small" in L.maxk_last_error()
    assert call_alpha(L, 3, (10, 10, 5), ws=ctypes.c_void_p(4096 + 16)) == -1
    assert b"256-B aligned" in L.maxk_last_error()


def test_no_edges_succeeds():
    """num_e == 0: the alpha entry launches nothing whatever the pointers; the forward has three
    outputs to zero, so null outputs are an error and an empty graph of no rows is not."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    assert call_alpha(L, 3, (10, 10, 0), p=None, ws=None, ws_bytes=0) == 0
    assert L.maxk_last_error() == b""
    assert call_fwd(L, 8, (0, 0, 0, 64, 8, 64), p=None, ws=None, ws_bytes=0) == 0
    assert L.maxk_last_error() == b""
    assert call_fwd(L, 3, (10, 10, 0, 64, 8, 0), p=None, ws=None, ws_bytes=0) == -1
    assert b"row_max" in L.maxk_last_error()


SHAPES = [(600, 600, 7000, 256, 16, 0), (600, 600, 7000, 64, 3, 64), (150, 700, 6000, 256, 96, 0),
          (1, 1, 1, 9, 7, 0), (232965, 232965, 114615892, 256, 16, 0),
          (2449029, 2449029, 123718280, 256, 32, 0)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_workspace_query_and_short_workspace(shape):
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    rows, cols, e, D, k, chunk = shape
    sizes = [L.maxk_gat_attention_heads_workspace_size(rows, cols, e, D, k, H, chunk)
             for H in range(1, 9)]
    assert all(n > 0 and n % 256 == 0 for n in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))  # non-decreasing in H
    for H, n in zip(range(1, 9), sizes):
        HP = 2 if H <= 2 else 4 if H <= 4 else 8
        assert n >= 6 * k * cols + 4 * HP * cols  # the records and ss_t
        if e > 10 ** 8:  # beside the records nothing of H * E floats: no alpha
            assert n - 16 * k * cols < 4 * H * e
        assert call_fwd(L, H, shape, ws_bytes=n - 1) == -1
        assert b"workspace too small" in L.maxk_last_error()
    n = sizes[4]
    assert call_fwd(L, 5, shape, ws=None, ws_bytes=n) == -1
    assert b"workspace too small" in L.maxk_last_error()
    assert call_fwd(L, 5, shape, ws=ctypes.c_void_p(4096 + 16), ws_bytes=n) == -1
    assert b"256-B aligned" in L.maxk_last_error()


@pytest.mark.parametrize("chunk", [0, 64])
def test_workspace_query_monotone_in_edges(chunk):
    """More edges never need less workspace, at 3 and at 8 heads."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    size = L.maxk_gat_attention_heads_workspace_size
    es = sorted(set([0, 1, 63, 64, 65, 255, 256, 257, 5000]
                    + list(range(65536 * 256 - 1000, 65536 * 256 + 1000, 97))
                    + list(range(65536 * 64 - 3000, 65536 * 64 + 1000, 97))
                    + [int(x) for x in np.geomspace(1e4, 2 ** 31 - 1, 300)]))
    for H in (3, 8):
        sizes = [size(1000, 1000, e, 256, 16, H, chunk) for e in es]
        assert all(s > 0 for s in sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:]))


# ------------------------------------------------------------------------------- the route
def test_route_rule_and_switch(monkeypatch):
    import maxk_cuda_kernels as mk
    monkeypatch.delenv("MAXK_HEADS_ATTN", raising=False)
    for H in range(1, 9):  # the measured rule: DESIGN.md 5.10
        assert mk.heads_attention_route(H, 232965, 114615892) == (
            "fused" if H >= 2 else "stored", "stored")  # dense: the fused forward wins
        for rows, e in ((2449029, 123718280), (600, 7000)):
            assert mk.heads_attention_route(H, rows, e) == ("stored", "stored")
    for forced in ("fused", "stored"):
        monkeypatch.setenv("MAXK_HEADS_ATTN", forced)
        for H in (1, 2, 8):
            assert mk.heads_attention_route(H, 1000, 50000) == (forced, forced)
    monkeypatch.delenv("MAXK_HEADS_ATTN")
    free = mk.heads_attention_route(4, 1000, 50000)
    monkeypatch.setenv("MAXK_HEADS_ATTN", "something else")
    assert mk.heads_attention_route(4, 1000, 50000) == free


def test_layer_argument_and_switch(monkeypatch):
    import maxk_layers as ML
    monkeypatch.delenv("MAXK_HEADS_ATTN", raising=False)
    assert ML.MaxKMultiHeadGATConv(12, 5, 3).attention_mode() == "stored"  # the default stays
    assert ML.MaxKMultiHeadGATConv(12, 5, 3, attention="fused").attention_mode() == "fused"
    with pytest.raises(ValueError, match="attention"):
        ML.MaxKMultiHeadGATConv(12, 5, 3, attention="both")
    for forced in ("fused", "stored"):
        monkeypatch.setenv("MAXK_HEADS_ATTN", forced)
        for arg in ("fused", "stored"):
            assert ML.MaxKMultiHeadGATConv(12, 5, 3, attention=arg).attention_mode() == forced
    monkeypatch.setenv("MAXK_HEADS_ATTN", "neither")
    assert ML.MaxKMultiHeadGATConv(12, 5, 3, attention="fused").attention_mode() == "fused"
