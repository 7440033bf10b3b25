"""CPU: the fused multi-head dot-product attention's reference helper, its C ABI surface, host
validation, workspace sizes and the layer's arguments and switch.

tests/dot_attention_ref.py is the yardstick of test_dot_attention_gpu.py, so it is pinned here
against float64 torch autograd of a dense composition (the scores q . x over the adjacency, a
softmax over each row's neighbours, a matmul with the scattered CBSR) on a small graph with an
empty row, a hub and an unread column, at scales 1 and 0.125.  No kernel is launched."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import dot_attention_ref as DR
import numerics as N
from conftest import PKG
from test_boundary_cpu import declared_symbols

FWD = "maxk_dot_attention_heads"
ALPHA = "maxk_dot_edge_alpha_heads"
SYMBOLS = (FWD, ALPHA, FWD + "_workspace_size", ALPHA + "_workspace_size")


# ------------------------------------------------------------------------------- the yardstick
def small_problem():
    from test_parity_gpu import rand_graph
    rng = np.random.default_rng(1801)
    rp, col = rand_graph(rng, 40, 5, hubs=((3, 35),), empty=2)
    g = N.make_graph(rng, rp, col, 40, unread=11)
    assert (np.diff(g.rp) == 0).any() and not (g.col == 11).any()
    D, k, H = 24, 5, 5
    ci = N.selectors(rng, g.C, D, k)
    ci[7, 2] = ci[7, 0]   # a repeated selector: both values are added
    ci[9, 1] = D + 3      # a selector past D: adds nothing
    cv = rng.standard_normal((g.C, k)).astype(np.float32)
    q = rng.standard_normal((H, g.R, D)).astype(np.float32)
    return g, ci, cv, q, D


def dense_features(ci, cv, D):
    """X [C, D] float64: the CBSR scattered, repeated selectors added, selectors >= D dropped."""
    C = ci.shape[0]
    X = torch.zeros(C, 256, dtype=torch.float64)
    X.index_put_((torch.arange(C)[:, None].expand(-1, ci.shape[1]),
                  torch.from_numpy(ci.astype(np.int64))),
                 torch.from_numpy(cv.astype(np.float64)), accumulate=True)
    return X[:, :D]


def dense_composition(g, X, q, scale):
    """(out [H, R, D], alpha [H, R, C], logits [H, R, C]) in float64 torch, dense over the
    adjacency; X and q may require grad."""
    R, C = g.R, g.C
    A = torch.zeros(R, C, dtype=torch.float64)
    rows = np.repeat(np.arange(R), np.diff(g.rp))
    A[torch.from_numpy(rows), torch.from_numpy(g.col.astype(np.int64))] = 1.0
    e = scale * torch.einsum("hrd,cd->hrc", q, X)
    masked = (A == 0) & (A.sum(1, keepdim=True) > 0)
    alpha = torch.softmax(e.masked_fill(masked, float("-inf")), 2) * A
    return alpha @ X, alpha, e


@pytest.mark.parametrize("scale", [1.0, 0.125])
def test_reference_agrees_with_dense_torch(scale):
    g, ci, cv, q, D = small_problem()
    H = q.shape[0]
    n = N.count_fwd(g, ci, D)
    a = DR.attention(g.rp, g.col, q, scale, cv, ci, D, n)
    X = dense_features(ci, cv, D)
    out, alpha, e = dense_composition(g, X, torch.from_numpy(q.astype(np.float64)), scale)
    out, alpha, e = out.numpy(), alpha.numpy(), e.numpy()
    assert a.out.shape == a.out_bound.shape == (H, g.R, D)
    assert a.m.shape == a.m_bound.shape == a.z.shape == a.z_bound.shape == (H, g.R)
    assert a.l.shape == a.l_bound.shape == a.w.shape == a.w_bound.shape == (H, g.col.size)
    err = np.abs(a.out - out).max()
    print(f"\ndot_attention_ref vs dense torch, scale {scale}: out {err:.3g}")
    assert err <= 1e-12 * max(1.0, np.abs(out).max())
    rows = np.repeat(np.arange(g.R), np.diff(g.rp))
    assert np.abs(a.l - e[:, rows, g.col]).max() <= 1e-12 * max(1.0, np.abs(e).max())
    assert np.abs(a.w - alpha[:, rows, g.col]).max() <= 1e-12
    # the statistics rebuild alpha
    w2 = DR.alpha_from_stats(g.rp, a.l, a.m, a.z)
    assert np.abs(w2 - a.w).max() <= 1e-12
    # structure: exact zeros with bound 0 where nothing is added, positive bounds elsewhere
    deg = np.diff(g.rp)
    assert (a.out[:, deg == 0] == 0).all() and (a.out_bound[:, deg == 0] == 0).all()
    assert (a.m[:, deg == 0] == 0).all() and (a.z[:, deg == 0] == 0).all()
    assert ((a.out_bound > 0) == (n > 0)[None]).all()
    assert ((a.out != 0) <= (n > 0)[None]).all()
    assert (a.z[:, deg > 0] >= 1).all() and (a.z_bound[:, deg > 0] > 0).all()
    assert (a.l_bound > 0).all() and (a.m_bound[:, deg > 0] > 0).all()
    # the weight bound: the edge softmax's, 8 u of the weight and the logit error carried
    f = a.heads[2]
    d_row = DR._row_max_of(a.l_bound[2], g.rp)
    extra = DR.weight_bound(f, d_row) - f.bound
    assert np.allclose(extra, (8 * DR.U + np.expm1(2 * d_row[rows])) * f.w, rtol=1e-12, atol=0)
    assert (d_row[rows] >= a.l_bound[2]).all()
    two = DR.heads_slice(a, 2)
    assert two.out.shape == (2, g.R, D) and len(two.heads) == 2


def test_reference_gradients_agree_with_dense_torch():
    """The adjoints the autograd functions compose -- grad_q = scale * (gl scattered on X) and
    grad_X = alpha^T g + scale * gl^T q with gl the softmax backward of g X^T -- against torch
    autograd of the dense composition."""
    g, ci, cv, q, D = small_problem()
    scale = 0.25
    n = N.count_fwd(g, ci, D)
    a = DR.attention(g.rp, g.col, q, scale, cv, ci, D, n)
    X = dense_features(ci, cv, D).requires_grad_(True)
    qt = torch.from_numpy(q.astype(np.float64)).requires_grad_(True)
    out, _, _ = dense_composition(g, X, qt, scale)
    rng = np.random.default_rng(5)
    go = rng.standard_normal(out.shape)
    out.backward(torch.from_numpy(go))
    rows = np.repeat(np.arange(g.R), np.diff(g.rp))
    Xn = X.detach().numpy()
    ga = np.einsum("hed,ed->he", go[:, rows], Xn[g.col])                 # d out / d alpha
    gl = np.stack([DR.ER.backward(g.rp, g.col, a.heads[h], ga[h]).gl for h in range(q.shape[0])])
    gq = np.zeros_like(go)
    gX = np.zeros_like(Xn)
    for h in range(q.shape[0]):
        np.add.at(gq[h], rows, scale * gl[h][:, None] * Xn[g.col])
        np.add.at(gX, g.col, a.w[h][:, None] * go[h, rows]
                  + scale * gl[h][:, None] * q[h].astype(np.float64)[rows])
    assert np.abs(gq - qt.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(gq).max())
    assert np.abs(gX - X.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(gX).max())


def test_reference_non_finite_rules():
    """A NaN logit: NaN wherever the row has an addend, 0 elsewhere; a NaN of q at a column no
    neighbour selects reaches nothing; a -Inf logit adds exactly 0; a row of only -Inf is NaN
    where it has addends; the NaN-ignoring maximum."""
    g, ci, cv, q, D = small_problem()
    n = N.count_fwd(g, ci, D)
    rows = np.repeat(np.arange(g.R), np.diff(g.rp))
    base = DR.attention(g.rp, g.col, q, 1.0, cv, ci, D, n)
    r = g.hub
    sel_r = ci[g.col[g.rp[r]:g.rp[r + 1]]]
    used = np.unique(sel_r[sel_r < D])
    unused = np.setdiff1d(np.arange(D), used)
    q1 = q.copy()
    q1[1, r, used[0]] = np.nan
    a = DR.attention(g.rp, g.col, q1, 1.0, cv, ci, D, n)
    assert np.isnan(a.out[1, r][n[r] > 0]).all() and (a.out[1, r][n[r] == 0] == 0).all()
    assert np.isnan(a.z[1, r]) and not np.isnan(a.m[1, r])
    others = np.ones(a.out.shape, bool)
    others[1, r] = False
    assert np.array_equal(a.out[others], base.out[others])
    # an Inf logit behaves like the NaN
    q2 = q.copy()
    q2[0, r, used[0]] = np.inf
    b = DR.attention(g.rp, g.col, q2, 1.0, cv, ci, D, n)
    assert np.isnan(b.out[0, r][n[r] > 0]).all() and (b.out[0, r][n[r] == 0] == 0).all()
    if unused.size:  # a column of q no neighbour selects is never read
        q3 = q.copy()
        q3[:, r, unused[0]] = np.nan
        c = DR.attention(g.rp, g.col, q3, 1.0, cv, ci, D, n)
        assert np.array_equal(c.out, base.out) and np.array_equal(c.z, base.z)
    # a row of two edges: one logit -Inf adds exactly 0, both -Inf is NaN where it has addends
    r2 = int(np.flatnonzero(np.diff(g.rp) == 2)[0])
    e0 = int(g.rp[r2])
    l = base.l.copy()
    f1 = DR.ER.forward(g.rp, np.where(np.arange(l.shape[1]) == e0, -np.inf, l[0]))
    assert f1.w[e0] == 0 and f1.w[e0 + 1] == 1
    f2 = DR.ER.forward(g.rp, np.where(rows == r2, -np.inf, l[0]))
    m, z = DR.AR._stats(g.rp, f2)
    assert np.isnan(f2.w[rows == r2]).all() and np.isneginf(m[r2]) and z[r2] == 0


# ------------------------------------------------------------------------------- the C ABI
def test_symbols_declared_exported_and_bound():
    from maxk_cuda_kernels import _capi
    syms = declared_symbols()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libmaxk_hip.so"))
    for s in SYMBOLS:
        assert s in syms and hasattr(lib, s) and s in _capi.SIGNATURES, s
    i32, i64, p, f32, sz = (ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float,
                            ctypes.c_size_t)
    call = (ctypes.c_int, [p] * 3 + [f32] + [p] * 5 + [i64] * 3 + [i32] * 4 + [p, sz, p])
    size = (sz, [i64] * 3 + [i32] * 4)
    assert _capi.SIGNATURES[FWD] == call and _capi.SIGNATURES[ALPHA] == call
    assert _capi.SIGNATURES[FWD + "_workspace_size"] == size
    assert _capi.SIGNATURES[ALPHA + "_workspace_size"] == size
    import maxk_cuda_kernels as mk
    for name in ("dot_attention_heads", "dot_edge_alpha_heads"):
        assert callable(getattr(mk, name)) and name in mk.__all__
    assert mk.version() == 100  # an addition: the ABI version stays
    import maxk_layers as ML
    import maxk_spgemm_function as MF
    for cls in (MF.MaxKDotScoresHeadsFunction, MF.MaxKDotAttentionHeadsFunction):
        assert issubclass(cls, torch.autograd.Function)
    assert callable(MF.maxk_dot_scores_heads) and callable(MF.maxk_dot_attention_heads)
    assert callable(ML.CSRGraph.dot_attend_heads)
    assert issubclass(ML.MaxKTransformerConv, torch.nn.Module)


def test_binding_refuses_cpu_tensors(monkeypatch):
    """No fallback: a CPU tensor is an error in the binding, the autograd functions, the graph's
    method and the layer on both paths."""
    import maxk_cuda_kernels as mk
    import maxk_layers as ML
    import maxk_spgemm_function as MF
    monkeypatch.delenv("MAXK_DOT_ATTN", raising=False)
    rp = torch.tensor([0, 2, 3], dtype=torch.int32)
    col = torch.tensor([0, 1, 1], dtype=torch.int32)
    q = torch.zeros(2, 2, 4)
    st = torch.zeros(2, 2)
    cv = torch.zeros(2, 3)
    ci = torch.zeros(2, 3, dtype=torch.uint8)
    g = ML.CSRGraph(rp, col)
    x = torch.zeros(2, 4)
    calls = [lambda: mk.dot_attention_heads(rp, col, q, cv, ci, 4, 0.5),
             lambda: mk.dot_edge_alpha_heads(rp, col, q, cv, ci, 4, 0.5, st, st),
             lambda: MF.maxk_dot_scores_heads(rp, col, q, cv, ci, 0.5),
             lambda: MF.maxk_dot_attention_heads(rp, col, q, cv, ci, 4, 0.5),
             lambda: g.dot_attend_heads(cv, ci, 4, q, 0.5),
             lambda: ML.MaxKTransformerConv(4, 3, 2, attention="fused")(g, x, cv, ci),
             lambda: ML.MaxKTransformerConv(4, 3, 2, attention="stored")(g, x, cv, ci)]
    for call_ in calls:
        with pytest.raises(RuntimeError, match="must be CUDA tensor"):
            call_()


P = ctypes.c_void_p(4096)  # a fake non-null, 256-B aligned device pointer: never dereferenced


def call_entry(L, name, H, shape, scale=0.5, p=P, ws=P, ws_bytes=1 << 42):
    """shape = (rows, cols, e, D, k, chunk); both entries take nine pointers around the scale."""
    rows, cols, e, D, k, chunk = shape
    return getattr(L, name)(p, p, p, scale, p, p, p, p, p, rows, cols, e, D, k, H, chunk, ws,
                            ws_bytes, None)


@pytest.mark.parametrize("name", [FWD, ALPHA])
def test_host_side_validation(name):
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    size = getattr(L, name + "_workspace_size")
    ok = (10, 10, 5, 64, 8, 0)
    for H in (0, 9, -1):  # num_heads outside [1, MAXK_MAX_HEADS]
        assert call_entry(L, name, H, ok) == -1
        assert b"num_heads must be in [1,8]" in L.maxk_last_error()
        assert call_entry(L, name, H, (10, 10, 0, 64, 8, 0)) == -1  # even without edges
        assert size(10, 10, 5, 64, 8, H, 0) == 0
    for shape, word in (((-1, 10, 5, 64, 8, 0), b"num_rows"), ((10, -1, 5, 64, 8, 0), b"num_cols"),
                        ((10, 10, -5, 64, 8, 0), b"num_e"),
                        ((10, 10, 5, 64, 8, -1), b"chunk_edges")):
        assert call_entry(L, name, 3, shape) == -1, shape  # negative sizes
        assert word in L.maxk_last_error()
        rows, cols, e, D, k, chunk = shape
        assert size(rows, cols, e, D, k, 3, chunk) == 0
    for D, k, word in ((0, 1, b"dim_origin"), (257, 8, b"dim_origin"), (64, 0, b"dim_k"),
                       (64, 65, b"dim_k")):  # k / D range
        assert call_entry(L, name, 3, (10, 10, 5, D, k, 0)) == -1, (D, k)
        assert word in L.maxk_last_error()
        assert size(10, 10, 5, D, k, 3, 0) == 0
    assert call_entry(L, name, 3, ok, p=None) == -1  # null pointers
    assert b"NULL" in L.maxk_last_error()
    for scale in (0.0, -1.0, math.inf, -math.inf, math.nan):
        assert call_entry(L, name, 3, ok, scale=scale) == -1, scale
        assert b"scale must be finite and > 0" in L.maxk_last_error()
        assert call_entry(L, name, 3, (10, 10, 0, 64, 8, 0), scale=scale) == -1  # without edges too
    assert call_entry(L, name, 3, (10, 0, 5, 64, 8, 0)) == -1  # edges and no column to hold them
    assert b"edges present" in L.maxk_last_error()
    assert call_entry(L, name, 3, (10, 1 << 24, 5, 64, 8, 0)) == -1  # a table past 2^24 columns
    assert b"2^24 columns" in L.maxk_last_error()
    assert call_entry(L, name, 3, (10, 1 << 23, 5, 256, 128, 0)) == -1  # ... or 4 GiB of records
    assert b"4 GiB of records" in L.maxk_last_error()
    for H in range(1, 9):  # every value in the range is accepted up to the workspace check
        for D, k in ((64, 3), (256, 96), (9, 7), (256, 256)):
            assert call_entry(L, name, H, (10, 10, 5, D, k, 0), ws_bytes=0) == -1
            assert b"workspace too small" in L.maxk_last_error()
    assert call_entry(L, name, 3, ok, ws=ctypes.c_void_p(4096 + 16)) == -1
    assert b"256-B aligned" in L.maxk_last_error()


def test_no_edges_succeeds():
    """num_e == 0: the alpha entry launches nothing whatever the pointers; the forward has three
    outputs to zero, so null outputs are an error and an empty graph of no rows is not."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    assert call_entry(L, ALPHA, 3, (10, 10, 0, 64, 8, 0), p=None, ws=None, ws_bytes=0) == 0
    assert L.maxk_last_error() == b""
    assert call_entry(L, FWD, 8, (0, 0, 0, 64, 8, 64), p=None, ws=None, ws_bytes=0) == 0
    assert L.maxk_last_error() == b""
    assert call_entry(L, FWD, 3, (10, 10, 0, 64, 8, 0), p=None, ws=None, ws_bytes=0) == -1
    assert b"row_max" in L.maxk_last_error()


SHAPES = [(600, 600, 7000, 256, 16, 0), (600, 600, 7000, 64, 3, 64), (150, 700, 6000, 256, 96, 0),
          (1, 1, 1, 9, 7, 0), (232965, 232965, 114615891, 256, 16, 0),
          (2449029, 2449029, 123718280, 256, 32, 0)]


def records_bytes(cols, k):
    """The packed records' size: 6 k bytes per column padded to a power of two up to a line,
    to whole 64-B sectors or lines past it (cbsr_pack.h)."""
    b = 6 * k
    if b <= 128:
        s = 16
        while s < b:
            s *= 2
    else:
        s64 = (b + 63) // 64 * 64
        s = s64 if s64 * cols <= 128 << 20 else (b + 127) // 128 * 128
    return (s * cols + 255) // 256 * 256


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_workspace_query_and_short_workspace(shape):
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    rows, cols, e, D, k, chunk = shape
    rec = records_bytes(cols, k)
    sizes = [L.maxk_dot_attention_heads_workspace_size(rows, cols, e, D, k, H, chunk)
             for H in range(1, 9)]
    assert all(n > 0 and n % 256 == 0 for n in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))  # non-decreasing in H
    for H, n in zip(range(1, 9), sizes):
        assert n >= rec
        if e > 10 ** 8:  # beside the records nothing of H * E floats: no logits, no alpha
            assert n < rec + H * e  # a quarter of one alpha [H, E]
        assert call_entry(L, FWD, H, shape, ws_bytes=n - 1) == -1
        assert b"workspace too small" in L.maxk_last_error()
        # the alpha entry: the records alone, whatever H and num_e
        na = L.maxk_dot_edge_alpha_heads_workspace_size(rows, cols, e, D, k, H, chunk)
        assert na == rec
        assert call_entry(L, ALPHA, H, shape, ws_bytes=na - 1) == -1
        assert b"workspace too small" in L.maxk_last_error()
    n = sizes[4]
    assert call_entry(L, FWD, 5, shape, ws=None, ws_bytes=n) == -1
    assert b"workspace too small" in L.maxk_last_error()


def test_workspace_slabs_at_the_auto_chunk():
    """Reddit-sized at 8 heads, chunk_edges = 0: below the records plus H * E bytes; at the auto
    rule's largest item, 2048 tokens, a cut row's slabs cost H * D * 4 / 2048 = H / 2 bytes per
    token (and 2 * 4 * H + 4 of statistics and the row per item)."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    size = L.maxk_dot_attention_heads_workspace_size
    R = C = 232965
    E, D, k, H = 114615891, 256, 16, 8
    rec = records_bytes(C, k)
    assert size(R, C, E, D, k, H, 0) < rec + H * E
    tokens = R + E
    items = -(-tokens // 2048)
    n = size(R, C, E, D, k, H, 2048)
    per_item = H * D * 4 + 2 * 4 * H + 4
    assert rec + items * (H * D * 4) <= n <= rec + items * per_item + 4 * 256
    assert abs((n - rec) / tokens - H / 2) < 0.05


@pytest.mark.parametrize("chunk", [0, 64])
def test_workspace_query_monotone_in_edges(chunk):
    """More edges never need less workspace, at 3 and at 8 heads."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    es = sorted(set([0, 1, 63, 64, 65, 255, 256, 257, 5000]
                    + list(range(65536 * 256 - 1000, 65536 * 256 + 1000, 97))
                    + list(range(65536 * 64 - 3000, 65536 * 64 + 1000, 97))
                    + [int(x) for x in np.geomspace(1e4, 2 ** 31 - 1, 300)]))
    for name in (FWD, ALPHA):
        size = getattr(L, name + "_workspace_size")
        for H in (3, 8):
            sizes = [size(1000, 1000, e, 256, 16, H, chunk) for e in es]
            assert all(s > 0 for s in sizes)
            assert all(a <= b for a, b in zip(sizes, sizes[1:]))


# ------------------------------------------------------------------------------- the layer
def test_layer_arguments_and_switch(monkeypatch):
    import maxk_cuda_kernels as mk
    import maxk_layers as ML
    monkeypatch.delenv("MAXK_DOT_ATTN", raising=False)
    conv = ML.MaxKTransformerConv(12, 5, 3)
    assert conv.attention_mode() == "stored"  # the default stays
    assert conv.scale == 5 ** -0.5
    for fc in (conv.fc_q, conv.fc_k, conv.fc_v):
        assert tuple(fc.weight.shape) == (15, 12) and fc.bias is None
    assert tuple(conv.bias.shape) == (3, 5)
    assert ML.MaxKTransformerConv(12, 5, 3, bias=False).bias is None
    assert ML.MaxKTransformerConv(12, 5, 3, attention="fused").attention_mode() == "fused"
    with pytest.raises(ValueError, match="attention"):
        ML.MaxKTransformerConv(12, 5, 3, attention="both")
    for heads in (0, mk.MAX_HEADS + 1):
        with pytest.raises(ValueError, match="num_heads"):
            ML.MaxKTransformerConv(12, 5, heads)
    for p in (-0.1, 1.0, math.nan):
        with pytest.raises(ValueError, match="attn_drop"):
            ML.MaxKTransformerConv(12, 5, 3, attn_drop=p)
    for forced in ("fused", "stored"):
        monkeypatch.setenv("MAXK_DOT_ATTN", forced)
        for arg in ("fused", "stored"):
            assert ML.MaxKTransformerConv(12, 5, 3, attention=arg).attention_mode() == forced
    monkeypatch.setenv("MAXK_DOT_ATTN", "neither")
    assert ML.MaxKTransformerConv(12, 5, 3, attention="fused").attention_mode() == "fused"


def test_fused_layer_refuses_dropout_in_training(monkeypatch):
    """attn_drop > 0 with the fused walk raises before any kernel is reached (CPU tensors here);
    in eval() the same call goes on to the binding, which refuses the CPU tensors."""
    import maxk_layers as ML
    monkeypatch.delenv("MAXK_DOT_ATTN", raising=False)
    rp = torch.tensor([0, 2, 3], dtype=torch.int32)
    col = torch.tensor([0, 1, 1], dtype=torch.int32)
    g = ML.CSRGraph(rp, col)
    x, cv, ci = torch.zeros(2, 4), torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.uint8)
    conv = ML.MaxKTransformerConv(4, 3, 2, attention="fused", attn_drop=0.5)
    with pytest.raises(ValueError, match="no dropout yet"):
        conv(g, x, cv, ci)
    conv.eval()
    with pytest.raises(RuntimeError, match="must be CUDA tensor"):
        conv(g, x, cv, ci)
    monkeypatch.setenv("MAXK_DOT_ATTN", "fused")  # the switch reaches the check too
    stored = ML.MaxKTransformerConv(4, 3, 2, attention="stored", attn_drop=0.5)
    with pytest.raises(ValueError, match="no dropout yet"):
        stored(g, x, cv, ci)
