"""CPU: the fused attention backward's reference helper, its C ABI surface, host validation, the
routing rule and the switches of the autograd function, the graph's method and the layer.

tests/gat_attention_bwd_ref.py is the yardstick of test_gat_attention_bwd_gpu.py, so it is pinned
here against float64 torch autograd of the dense composition of test_gat_attention_cpu.py (a
small graph with an empty row, a hub, an unread column, a repeated selector and one past D), at
slopes 0.2, 0 and 1.  No kernel is launched."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import gat_attention_bwd_ref as BR
import gat_attention_ref as AR
import numerics as N
from conftest import PKG
from test_boundary_cpu import declared_symbols
from test_gat_attention_cpu import small_problem
from test_gat_attention_gpu import feat_grad_ref, make_case, the_graph

BWD = "maxk_gat_attention_heads_backward"
SYMBOLS = (BWD, BWD + "_workspace_size")


# ------------------------------------------------------------------------------- the yardstick
def dense_grads(g, ci, cv, s_dst, s_src, D, slope, G):
    """(grad s_dst, grad s_src, grad cv) of sum(out * G) in float64 torch, dense over the
    adjacency (the composition of test_gat_attention_cpu.dense_composition, differentiable)."""
    R, C = g.R, g.C
    A = torch.zeros(R, C, dtype=torch.float64)
    rows = np.repeat(np.arange(R), np.diff(g.rp))
    A[torch.from_numpy(rows), torch.from_numpy(g.col.astype(np.int64))] = 1.0
    v = torch.from_numpy(cv.astype(np.float64)).requires_grad_(True)
    X = torch.zeros(C, 256, dtype=torch.float64).index_put(
        (torch.arange(C)[:, None].expand(-1, ci.shape[1]), torch.from_numpy(ci.astype(np.int64))),
        v, accumulate=True)[:, :D]
    sd = torch.from_numpy(s_dst.astype(np.float64)).requires_grad_(True)
    ss = torch.from_numpy(s_src.astype(np.float64)).requires_grad_(True)
    e = torch.nn.functional.leaky_relu(sd[:, :, None] + ss[:, None, :], slope)
    masked = (A == 0) & (A.sum(1, keepdim=True) > 0)
    alpha = torch.softmax(e.masked_fill(masked, float("-inf")), 2) * A
    out = alpha @ X
    return [t.numpy() for t in torch.autograd.grad(
        out, [sd, ss, v], torch.from_numpy(G.astype(np.float64)))]


@pytest.mark.parametrize("slope", [0.2, 0.0, 1.0])
def test_reference_agrees_with_dense_torch_autograd(slope):
    g, ci, cv, s_dst, s_src, D = small_problem()
    H = s_dst.shape[0]
    rng = np.random.default_rng(2801)
    G = rng.standard_normal((H, g.R, D)).astype(np.float32)
    n = N.count_fwd(g, ci, D)
    a = AR.attention(g.rp, g.col, s_dst, s_src, slope, cv, ci, D, n)
    b = BR.backward(g, a, cv, ci, G, slope, D, BR.rounded_out_err(a), feat_grad_ref)
    want = dense_grads(g, ci, cv, s_dst, s_src, D, slope, G)
    for name, got, ref in (("s_dst", b.g_dst, want[0]), ("s_src", b.g_src, want[1]),
                           ("cbsr", b.g_cbsr, want[2])):
        err = np.abs(got - ref).max()
        print(f"\ngat_attention_bwd_ref vs torch autograd, slope {slope}: {name} {err:.3g}")
        assert got.shape == ref.shape and err <= 1e-12 * max(1.0, np.abs(ref).max()), name
    # t = sum_j out_j G_j is the softmax backward's sum_e alpha_e ga_e, in float64
    te = np.stack([np.bincount(a.heads[h].rows, a.w[h] * b.ga[h], minlength=g.R)
                   for h in range(H)])
    assert np.abs(te - b.t).max() <= 1e-12 * max(1.0, np.abs(b.t).max())
    # structure: an element without addends is an exact 0 with bound 0
    deg = np.diff(g.rp)
    assert (b.g_dst[:, deg == 0] == 0).all() and (b.g_dst_bound[:, deg == 0] == 0).all()
    assert (b.g_src[:, g.unread] == 0).all() and (b.g_src_bound[:, g.unread] == 0).all()
    assert (b.g_cbsr[g.unread] == 0).all() and (b.g_cbsr_bound[g.unread] == 0).all()
    assert b.g_cbsr[9, 1] == 0 and b.g_cbsr_bound[9, 1] == 0     # the selector past D
    assert b.g_cbsr[7, 2] == b.g_cbsr[7, 0] != 0                 # the repeated selector: both
    if slope > 0:  # slope 0: gz of an edge with z <= 0 is the exact 0 of a product with 0
        assert (b.g_dst_bound[:, deg > 0] > 0).all() and (b.gz_bound > 0).all()


def test_reference_skips_columns_without_addends():
    """A NaN of G in a column no edge of the row selects reaches nothing."""
    g, ci, cv, s_dst, s_src, D = small_problem()
    H = s_dst.shape[0]
    rng = np.random.default_rng(2802)
    G = rng.standard_normal((H, g.R, D)).astype(np.float32)
    n = N.count_fwd(g, ci, D)
    a = AR.attention(g.rp, g.col, s_dst, s_src, 0.2, cv, ci, D, n)
    clean = BR.backward(g, a, cv, ci, G, 0.2, D, BR.rounded_out_err(a), feat_grad_ref)
    G2 = G.copy()
    assert (n == 0).any()
    G2[:, n == 0] = np.nan
    b = BR.backward(g, a, cv, ci, G2, 0.2, D, BR.rounded_out_err(a), feat_grad_ref)
    for x, y in zip(clean, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", ["S", "Dn", "R", "corner", "transpose"])
def test_rounded_reference_is_inside_its_bounds(name):
    """The reference rounded to fp32 -- the best any fp32 kernel can return -- is inside the
    bounds, with the `out` of both regimes (rounded reference, the forward's own bound); an
    element whose bound is 0 is an exact 0."""
    H = 2
    k, D = (7, 9) if name == "R" else (16, 256)
    c = make_case(name, k, D)
    g, a = c["g"], AR.heads_slice(c["a"], H)
    rng = np.random.default_rng(2803)
    G = np.stack([N.values(rng, (g.R, D), "unit") for _ in range(H)])
    for out_err in (BR.rounded_out_err(a), a.out_bound):
        b = BR.backward(g, a, c["cv"], c["ci"], G, 0.2, D, out_err, feat_grad_ref)
        for what in ("gz", "g_dst", "g_src", "g_cbsr"):
            ref, bound = getattr(b, what), getattr(b, what + "_bound")
            assert np.isfinite(ref).all() and np.isfinite(bound).all() and (bound >= 0).all()
            r = N.within(ref.astype(np.float32), ref, bound, f"{name} {what}")
            assert r <= 0.5, (what, r)  # half an ulp of the result against (n + 8) ulp of sums
            assert (ref[bound == 0] == 0).all()
    assert (b.g_dst_bound[:, np.diff(g.rp) > 0] > 0).all()


# ------------------------------------------------------------------------------- the C ABI
def test_symbols_declared_exported_and_bound():
    from maxk_cuda_kernels import _capi
    syms = declared_symbols()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libmaxk_hip.so"))
    for s in SYMBOLS:
        assert s in syms and hasattr(lib, s) and s in _capi.SIGNATURES, s
    i32, i64, p, f32, sz = (ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float,
                            ctypes.c_size_t)
    assert _capi.SIGNATURES[BWD] == (ctypes.c_int, [p] * 6 + [f32] + [p] * 9 + [i64] * 3
                                     + [i32] * 4 + [p, sz, p])
    assert _capi.SIGNATURES[BWD + "_workspace_size"] == (sz, [i64] * 3 + [i32] * 4)
    import maxk_cuda_kernels as mk
    for name in ("gat_attention_heads_backward", "heads_attention_backward_route"):
        assert callable(getattr(mk, name)) and name in mk.__all__
    assert mk.version() == 100  # an addition: the ABI version stays


def test_binding_refuses_cpu_tensors(monkeypatch):
    """No fallback: a CPU tensor is an error in the binding and under backward="fused"."""
    import maxk_cuda_kernels as mk
    import maxk_layers as ML
    import maxk_spgemm_function as MF
    monkeypatch.delenv("MAXK_HEADS_ATTN", raising=False)
    monkeypatch.delenv("MAXK_HEADS_ATTN_BWD", raising=False)
    rp = torch.tensor([0, 2, 3], dtype=torch.int32)
    col = torch.tensor([0, 1, 1], dtype=torch.int32)
    v = torch.zeros(2, 2)
    o = torch.zeros(2, 2, 4)
    cv = torch.zeros(2, 3)
    ci = torch.zeros(2, 3, dtype=torch.uint8)
    g = ML.CSRGraph(rp, col)
    conv = ML.MaxKMultiHeadGATConv(4, 3, 2, attention="fused", attention_backward="fused")
    calls = [lambda: mk.gat_attention_heads_backward(rp, col, v, v, cv, ci, o, v, v, o),
             lambda: MF.maxk_gat_attention_heads(rp, col, v, v, cv, ci, 4, backward="fused"),
             lambda: g.attend_heads(cv, ci, 4, v, v, backward="fused"),
             lambda: conv(g, torch.zeros(2, 4), cv, ci)]
    for call_ in calls:
        with pytest.raises(RuntimeError, match="must be CUDA tensor"):
            call_()


P = ctypes.c_void_p(4096)  # a fake non-null, 256-B aligned device pointer: never dereferenced


def call_bwd(L, H, shape, slope=0.2, p=P, ws=P, ws_bytes=1 << 42, **named):
    """shape = (rows, cols, e, D, k, chunk); named: one pointer argument by name."""
    rows, cols, e, D, k, chunk = shape
    names = ("row_ptr col_idx col_ptr csc_eid s_dst s_src cbsr_val cbsr_idx out row_max row_sum "
             "grad_out grad_s_dst grad_s_src grad_cbsr").split()
    a = {n: named.get(n, p) for n in names}
    return L.maxk_gat_attention_heads_backward(
        a["row_ptr"], a["col_idx"], a["col_ptr"], a["csc_eid"], a["s_dst"], a["s_src"], slope,
        a["cbsr_val"], a["cbsr_idx"], a["out"], a["row_max"], a["row_sum"], a["grad_out"],
        a["grad_s_dst"], a["grad_s_src"], a["grad_cbsr"], rows, cols, e, D, k, H, chunk, ws,
        ws_bytes, None)


def test_host_side_validation():
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    size = L.maxk_gat_attention_heads_backward_workspace_size
    ok = (10, 10, 5, 64, 8, 0)
    for H in (0, 9, -1):  # num_heads outside [1, MAXK_MAX_HEADS]
        assert call_bwd(L, H, ok) == -1
        assert b"num_heads must be in [1,8]" in L.maxk_last_error()
        assert call_bwd(L, H, (10, 10, 0, 64, 8, 0)) == -1  # even without edges
        assert size(10, 10, 5, 64, 8, H, 0) == 0
    for shape, word in (((-1, 10, 5, 64, 8, 0), b"num_rows"), ((10, -1, 5, 64, 8, 0), b"num_cols"),
                        ((10, 10, -5, 64, 8, 0), b"num_e"),
                        ((10, 10, 5, 64, 8, -1), b"chunk_edges")):
        assert call_bwd(L, 3, shape) == -1, shape
        assert word in L.maxk_last_error()
        rows, cols, e, D, k, chunk = shape
        assert size(rows, cols, e, D, k, 3, chunk) == 0
    for D, k, word in ((0, 1, b"dim_origin"), (257, 8, b"dim_origin"), (64, 0, b"dim_k"),
                       (64, 65, b"dim_k")):
        assert call_bwd(L, 3, (10, 10, 5, D, k, 0)) == -1, (D, k)
        assert word in L.maxk_last_error()
    for slope in (-0.1, 1.5, math.nan):
        assert call_bwd(L, 3, ok, slope=slope) == -1, slope
        assert b"negative_slope must be in [0, 1]" in L.maxk_last_error()
        assert call_bwd(L, 3, (10, 10, 0, 64, 8, 0), slope=slope) == -1  # even without edges
    # every pointer, by name
    for n in ("row_ptr col_idx col_ptr csc_eid s_dst s_src cbsr_val cbsr_idx out row_max row_sum "
              "grad_out grad_s_dst grad_s_src grad_cbsr").split():
        assert call_bwd(L, 3, ok, **{n: None}) == -1, n
        msg = L.maxk_last_error()
        assert n.encode() in msg and b"NULL" in msg, (n, msg)
    assert call_bwd(L, 3, (10, 0, 5, 64, 8, 0)) == -1  # edges and no column to hold them
    assert b"edges present" in L.maxk_last_error()
    assert call_bwd(L, 3, (10, 1 << 24, 5, 64, 8, 0)) == -1  # a table past 2^24 columns
    assert b"2^24 columns" in L.maxk_last_error()
    assert call_bwd(L, 3, ok, cbsr_val=ctypes.c_void_p(4098)) == -1
    assert b"4-B aligned" in L.maxk_last_error()
    for H in range(1, 9):  # every value in the range is accepted up to the workspace check
        for D, k in ((64, 3), (256, 96), (9, 7), (256, 256)):
            assert call_bwd(L, H, (10, 10, 5, D, k, 0), ws_bytes=0) == -1
            assert b"workspace too small" in L.maxk_last_error()


def test_no_edges():
    """num_e == 0: three outputs to zero, so null outputs are an error; an empty graph of no
    rows and no columns has nothing to write."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    assert call_bwd(L, 8, (0, 0, 0, 64, 8, 64), p=None, ws=None, ws_bytes=0) == 0
    assert L.maxk_last_error() == b""
    assert call_bwd(L, 3, (10, 10, 0, 64, 8, 0), p=None, ws=None, ws_bytes=0) == -1
    assert b"grad_s_dst" in L.maxk_last_error()


SHAPES = [(600, 600, 7000, 256, 16, 0), (600, 600, 7000, 64, 3, 64), (150, 700, 6000, 256, 96, 0),
          (1, 1, 1, 9, 7, 0), (232965, 232965, 114615892, 256, 16, 0),
          (2449029, 2449029, 123718280, 256, 32, 0)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_workspace_query_and_short_workspace(shape):
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    rows, cols, e, D, k, chunk = shape
    sizes = [L.maxk_gat_attention_heads_backward_workspace_size(rows, cols, e, D, k, H, chunk)
             for H in range(1, 9)]
    assert all(n > 0 and n % 256 == 0 for n in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))  # non-decreasing in H
    for H, n in zip(range(1, 9), sizes):
        HP = 2 if H <= 2 else 4 if H <= 4 else 8
        # T with its dummy row, the records, ss_t and gzT
        assert n >= 4 * k * (e + 1) + 6 * k * cols + 4 * HP * cols + 4 * HP * e
        if e > 10 ** 8:  # beside T, gzT and the records nothing that grows with H * E
            assert n - 4 * k * (e + 1) - 4 * HP * e - 16 * k * cols < 4 * e
        assert call_bwd(L, H, shape, ws_bytes=n - 1) == -1
        assert b"workspace too small" in L.maxk_last_error()
    n = sizes[4]
    assert call_bwd(L, 5, shape, ws=None, ws_bytes=n) == -1
    assert b"workspace too small" in L.maxk_last_error()
    assert call_bwd(L, 5, shape, ws=ctypes.c_void_p(4096 + 16), ws_bytes=n) == -1
    assert b"256-B aligned" in L.maxk_last_error()


@pytest.mark.parametrize("chunk", [0, 64])
def test_workspace_query_monotone_in_edges(chunk):
    """More edges never need less workspace, at 3 and at 8 heads."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    size = L.maxk_gat_attention_heads_backward_workspace_size
    es = sorted(set([0, 1, 63, 64, 65, 255, 256, 257, 5000]
                    + list(range(65536 * 256 - 1000, 65536 * 256 + 1000, 97))
                    + list(range(131072 * 256 - 1000, 131072 * 256 + 1000, 97))
                    + list(range(65536 * 64 - 3000, 65536 * 64 + 1000, 97))
                    + [int(x) for x in np.geomspace(1e4, 2 ** 31 - 1, 300)]))
    for H in (3, 8):
        sizes = [size(1000, 1000, e, 256, 16, H, chunk) for e in es]
        assert all(s > 0 for s in sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:]))


# ------------------------------------------------------------------------------- the switches
def test_route_rule(monkeypatch):
    import maxk_cuda_kernels as mk
    monkeypatch.delenv("MAXK_HEADS_ATTN_BWD", raising=False)
    for H in range(1, 9):  # the measured rule: the fused backward everywhere
        for rows, e in ((232965, 114615892), (2449029, 123718280), (600, 7000)):
            assert mk.heads_attention_backward_route(H, rows, e) == "fused"
    for forced in ("fused", "rebuilt"):
        monkeypatch.setenv("MAXK_HEADS_ATTN_BWD", forced)
        for H in (1, 2, 8):
            assert mk.heads_attention_backward_route(H, 1000, 50000) == forced
    monkeypatch.setenv("MAXK_HEADS_ATTN_BWD", "something else")
    assert mk.heads_attention_backward_route(4, 1000, 50000) == "fused"


def test_defaults_and_environment_override(monkeypatch):
    """backward defaults to "rebuilt" in the function, the graph's method and the layer;
    MAXK_HEADS_ATTN_BWD overrides the method's and the layer's argument; other words are
    refused."""
    import inspect

    import maxk_layers as ML
    import maxk_spgemm_function as MF
    monkeypatch.delenv("MAXK_HEADS_ATTN_BWD", raising=False)
    assert inspect.signature(MF.maxk_gat_attention_heads).parameters["backward"].default == \
        "rebuilt"
    assert inspect.signature(
        MF.MaxKGATAttentionHeadsFunction.forward).parameters["backward"].default == "rebuilt"
    assert inspect.signature(ML.CSRGraph.attend_heads).parameters["backward"].default == "rebuilt"
    assert ML.MaxKMultiHeadGATConv(12, 5, 3).attention_backward_mode() == "rebuilt"
    conv = ML.MaxKMultiHeadGATConv(12, 5, 3, attention="fused", attention_backward="fused")
    assert conv.attention_backward_mode() == "fused" and conv.attention_mode() == "fused"
    with pytest.raises(ValueError, match="attention_backward"):
        ML.MaxKMultiHeadGATConv(12, 5, 3, attention_backward="both")
    rp = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(ValueError, match="backward"):
        ML.CSRGraph(rp, rp[:1]).attend_heads(None, None, 4, None, None, backward="both")
    for forced in ("fused", "rebuilt"):
        monkeypatch.setenv("MAXK_HEADS_ATTN_BWD", forced)
        for arg in ("fused", "rebuilt"):
            assert ML.MaxKMultiHeadGATConv(
                12, 5, 3, attention_backward=arg).attention_backward_mode() == forced
    monkeypatch.setenv("MAXK_HEADS_ATTN_BWD", "neither")
    assert ML.MaxKMultiHeadGATConv(
        12, 5, 3, attention_backward="fused").attention_backward_mode() == "fused"
