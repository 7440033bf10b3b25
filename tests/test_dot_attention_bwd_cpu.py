"""CPU: the fused dot-product attention backward's reference helper, its C ABI surface, host
validation, the workspace query, the routing rule and the switches of the autograd function, the
graph's method and the layer.

tests/dot_attention_bwd_ref.py is the yardstick of test_dot_attention_bwd_gpu.py, so it is pinned
here against float64 torch autograd of the dense composition of test_dot_attention_cpu.py (a
small graph with an empty row, a hub, an unread column, a repeated selector and one past D).  No
kernel is launched."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import dot_attention_bwd_ref as BR
import dot_attention_ref as DR
import numerics as N
from conftest import PKG
from test_boundary_cpu import declared_symbols
from test_dot_attention_cpu import dense_composition, dense_features, small_problem
from test_dot_attention_gpu import make_case

BWD = "maxk_dot_attention_heads_backward"
SYMBOLS = (BWD, BWD + "_workspace_size")
ENV = "MAXK_DOT_ATTN_BWD"


# ------------------------------------------------------------------------------- the yardstick
def reference(scale, G=None, q=None, seed=2901):
    g, ci, cv, q0, D = small_problem()
    q = q0 if q is None else q
    H = q.shape[0]
    if G is None:
        G = np.random.default_rng(seed).standard_normal((H, g.R, D)).astype(np.float32)
    n = N.count_fwd(g, ci, D)
    a = DR.attention(g.rp, g.col, q, scale, cv, ci, D, n)
    b = BR.backward(g, a, q, scale, cv, ci, G, D, BR.rounded_out_err(a), n)
    return g, ci, cv, q, D, G, n, a, b


@pytest.mark.parametrize("scale", [1.0, 0.25])
def test_reference_agrees_with_dense_torch_autograd(scale):
    g, ci, cv, q, D, G, n, a, b = reference(scale)
    H = q.shape[0]
    v = torch.from_numpy(cv.astype(np.float64)).requires_grad_(True)
    X = torch.zeros(g.C, 256, dtype=torch.float64).index_put(
        (torch.arange(g.C)[:, None].expand(-1, ci.shape[1]), torch.from_numpy(ci.astype(np.int64))),
        v, accumulate=True)[:, :D]
    assert torch.equal(X.detach(), dense_features(ci, cv, D))
    qt = torch.from_numpy(q.astype(np.float64)).requires_grad_(True)
    out, _, _ = dense_composition(g, X, qt, scale)
    want_q, want_v = (t.numpy() for t in torch.autograd.grad(
        out, [qt, v], torch.from_numpy(G.astype(np.float64))))
    got_v, v_bound = BR.cbsr(b, H)
    for name, got, ref in (("q", b.g_q, want_q), ("cbsr", got_v, want_v)):
        err = np.abs(got - ref).max()
        print(f"\ndot_attention_bwd_ref vs torch autograd, scale {scale}: {name} {err:.3g}")
        assert got.shape == ref.shape and err <= 1e-12 * max(1.0, np.abs(ref).max()), name
    # t = sum_j out_j G_j is the softmax backward's sum_e alpha_e ga_e, in float64
    te = np.stack([np.bincount(a.heads[h].rows, a.w[h] * b.ga[h], minlength=g.R)
                   for h in range(H)])
    assert np.abs(te - b.t).max() <= 1e-12 * max(1.0, np.abs(b.t).max())
    # structure: an element without addends is an exact 0 with bound 0
    deg = np.diff(g.rp)
    assert (b.g_q[:, deg == 0] == 0).all() and (b.g_q_bound[:, deg == 0] == 0).all()
    assert ((b.g_q_bound > 0) == (n > 0)[None]).all() and ((b.g_q != 0) <= (n > 0)[None]).all()
    assert (got_v[g.unread] == 0).all() and (v_bound[g.unread] == 0).all()
    assert got_v[9, 1] == 0 and v_bound[9, 1] == 0           # the selector past D
    assert got_v[7, 2] == got_v[7, 0] != 0                   # the repeated selector: both
    assert (b.gl_bound > 0).all()
    # g_cbsr sums the heads
    one, _ = BR.cbsr(b, 1)
    assert not np.array_equal(one, got_v) and one.shape == got_v.shape


def test_reference_skips_columns_without_addends():
    """A NaN of G, and one of q, in a column no edge of the row selects reaches nothing."""
    g, ci, cv, q, D, G, n, a, clean = reference(0.5)
    assert (n == 0).any()
    G2 = G.copy()
    G2[:, n == 0] = np.nan
    b = reference(0.5, G=G2)[-1]
    q2 = q.copy()
    q2[:, n == 0] = np.nan
    c = reference(0.5, q=q2)[-1]
    for other in (b, c):
        for x, y in zip(clean[:8], other[:8]):
            assert np.array_equal(x, y)
        for H in (1, 5):
            for x, y in zip(BR.cbsr(clean, H), BR.cbsr(other, H)):
                assert np.array_equal(x, y)


def test_reference_non_finite_rules():
    """A NaN in q[h, r, j] at a column a neighbour of r selects reaches head h's g_q row r
    wherever it has an addend and g_cbsr of the columns r reads, and nothing else; a -Inf logit
    gives alpha = 0 and gl = 0."""
    g, ci, cv, q, D, G, n, a, clean = reference(1.0)
    r = g.hub
    nb = g.col[g.rp[r]:g.rp[r + 1]]
    used = np.unique(ci[nb][ci[nb] < D])
    q1 = q.copy()
    q1[1, r, used[0]] = np.nan
    b = reference(1.0, q=q1)[-1]
    assert np.isnan(b.g_q[1, r][n[r] > 0]).all() and (b.g_q[1, r][n[r] == 0] == 0).all()
    others = np.ones(b.g_q.shape, bool)
    others[1, r] = False
    assert np.array_equal(b.g_q[others], clean.g_q[others])
    gc, gc0 = BR.cbsr(b, 5)[0], BR.cbsr(clean, 5)[0]
    live = (ci < D)
    assert np.isnan(gc[nb][live[nb]]).all()
    rest = np.setdiff1d(np.arange(g.C), nb)
    assert np.array_equal(gc[rest], gc0[rest])
    assert np.array_equal(BR.cbsr(b, 1)[0], BR.cbsr(clean, 1)[0])  # head 0 alone: untouched
    # a -Inf logit: the weight is 0 and so is gl (ga and t are finite)
    r2 = int(np.flatnonzero(np.diff(g.rp) == 2)[0])
    e0 = int(g.rp[r2])
    c0 = g.col[e0]
    own = [l for l in range(ci.shape[1]) if ci[c0, l] < D
           and ci[c0, l] not in ci[g.col[e0 + 1]] and (ci[c0] == ci[c0, l]).sum() == 1]
    if own:
        q3 = q.copy()
        q3[0, r2, ci[c0, own[0]]] = -np.copysign(np.inf, cv[c0, own[0]])
        d = reference(1.0, q=q3)[-1]
        a3 = reference(1.0, q=q3)[-2]
        assert a3.w[0, e0] == 0 and d.gl[0, e0] == 0


@pytest.mark.parametrize("name", ["S", "Dn", "R", "corner", "transpose"])
def test_rounded_reference_is_inside_its_bounds(name):
    """The reference rounded to fp32 -- the best any fp32 kernel can return -- is inside the
    bounds, with the `out` of both regimes (rounded reference, the forward's own bound); an
    element whose bound is 0 is an exact 0."""
    H = 2
    k, D = (7, 9) if name == "R" else (16, 256)
    c = make_case(name, k, D, 0.125)
    g, a = c["g"], DR.heads_slice(c["a"], H)
    rng = np.random.default_rng(2903)
    G = np.stack([N.values(rng, (g.R, D), "unit") for _ in range(H)])
    for out_err in (BR.rounded_out_err(a), a.out_bound):
        b = BR.backward(g, a, c["q"][:H], c["scale"], c["cv"], c["ci"], G, D, out_err, c["n"])
        gc, gcb = BR.cbsr(b, H)
        for what, ref, bound in (("gl", b.gl, b.gl_bound), ("g_q", b.g_q, b.g_q_bound),
                                 ("g_cbsr", gc, gcb)):
            assert np.isfinite(ref).all() and np.isfinite(bound).all() and (bound >= 0).all()
            r = N.within(ref.astype(np.float32), ref, bound, f"{name} {what}")
            assert r <= 0.5, (what, r)  # half an ulp of the result against (n + 8) ulp of sums
            assert (ref[bound == 0] == 0).all()
    assert ((b.g_q_bound > 0) == (c["n"] > 0)[None]).all()


# ------------------------------------------------------------------------------- the C ABI
def test_symbols_declared_exported_and_bound():
    from maxk_cuda_kernels import _capi
    syms = declared_symbols()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libmaxk_hip.so"))
    for s in SYMBOLS:
        assert s in syms and hasattr(lib, s) and s in _capi.SIGNATURES, s
    i32, i64, p, f32, sz = (ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float,
                            ctypes.c_size_t)
    assert _capi.SIGNATURES[BWD] == (ctypes.c_int, [p] * 5 + [f32] + [p] * 8 + [i64] * 3
                                     + [i32] * 4 + [p, sz, p])
    assert _capi.SIGNATURES[BWD + "_workspace_size"] == (sz, [i64] * 3 + [i32] * 4)
    import maxk_cuda_kernels as mk
    for name in ("dot_attention_heads_backward", "dot_attention_backward_route"):
        assert callable(getattr(mk, name)) and name in mk.__all__
    assert mk.version() == 100  # an addition: the ABI version stays


def test_binding_refuses_cpu_tensors(monkeypatch):
    """No fallback: a CPU tensor is an error in the binding and under backward="fused"."""
    import maxk_cuda_kernels as mk
    import maxk_layers as ML
    import maxk_spgemm_function as MF
    monkeypatch.delenv("MAXK_DOT_ATTN", raising=False)
    monkeypatch.delenv(ENV, raising=False)
    rp = torch.tensor([0, 2, 3], dtype=torch.int32)
    col = torch.tensor([0, 1, 1], dtype=torch.int32)
    q = torch.zeros(2, 2, 4)
    st = torch.zeros(2, 2)
    cv = torch.zeros(2, 3)
    ci = torch.zeros(2, 3, dtype=torch.uint8)
    g = ML.CSRGraph(rp, col)
    conv = ML.MaxKTransformerConv(4, 3, 2, attention="fused", attention_backward="fused")
    calls = [lambda: mk.dot_attention_heads_backward(rp, col, q, cv, ci, q, st, st, q, 0.5),
             lambda: MF.maxk_dot_attention_heads(rp, col, q, cv, ci, 4, 0.5, backward="fused"),
             lambda: g.dot_attend_heads(cv, ci, 4, q, 0.5, backward="fused"),
             lambda: conv(g, torch.zeros(2, 4), cv, ci)]
    for call_ in calls:
        with pytest.raises(RuntimeError, match="must be CUDA tensor"):
            call_()


P = ctypes.c_void_p(4096)  # a fake non-null, 256-B aligned device pointer: never dereferenced
POINTERS = ("row_ptr col_idx col_ptr csc_eid q cbsr_val cbsr_idx out row_max row_sum grad_out "
            "grad_q grad_cbsr").split()


def call_bwd(L, H, shape, scale=0.5, p=P, ws=P, ws_bytes=1 << 42, **named):
    """shape = (rows, cols, e, D, k, chunk); named: one pointer argument by name."""
    rows, cols, e, D, k, chunk = shape
    a = {n: named.get(n, p) for n in POINTERS}
    return L.maxk_dot_attention_heads_backward(
        a["row_ptr"], a["col_idx"], a["col_ptr"], a["csc_eid"], a["q"], scale, a["cbsr_val"],
        a["cbsr_idx"], a["out"], a["row_max"], a["row_sum"], a["grad_out"], a["grad_q"],
        a["grad_cbsr"], rows, cols, e, D, k, H, chunk, ws, ws_bytes, None)


def test_host_side_validation():
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    size = L.maxk_dot_attention_heads_backward_workspace_size
    ok = (10, 10, 5, 64, 8, 0)
    for H in (0, 9, -1):  # num_heads outside [1, MAXK_MAX_HEADS]
        assert call_bwd(L, H, ok) == -1
        assert b"num_heads must be in [1,8]" in L.maxk_last_error()
        assert call_bwd(L, H, (10, 10, 0, 64, 8, 0)) == -1  # even without edges
        assert size(10, 10, 5, 64, 8, H, 0) == 0
    for shape, word in (((-1, 10, 5, 64, 8, 0), b"num_rows"), ((10, -1, 5, 64, 8, 0), b"num_cols"),
                        ((10, 10, -5, 64, 8, 0), b"num_e"),
                        ((10, 10, 5, 64, 8, -1), b"chunk_edges")):
        assert call_bwd(L, 3, shape) == -1, shape  # negative sizes
        assert word in L.maxk_last_error()
        rows, cols, e, D, k, chunk = shape
        assert size(rows, cols, e, D, k, 3, chunk) == 0
    for D, k, word in ((0, 1, b"dim_origin"), (257, 8, b"dim_origin"), (64, 0, b"dim_k"),
                       (64, 65, b"dim_k")):  # k / D range
        assert call_bwd(L, 3, (10, 10, 5, D, k, 0)) == -1, (D, k)
        assert word in L.maxk_last_error()
        assert size(10, 10, 5, D, k, 3, 0) == 0
    for scale in (0.0, -1.0, math.inf, -math.inf, math.nan):
        assert call_bwd(L, 3, ok, scale=scale) == -1, scale
        assert b"scale must be finite and > 0" in L.maxk_last_error()
        assert call_bwd(L, 3, (10, 10, 0, 64, 8, 0), scale=scale) == -1  # without edges too
    for n in POINTERS:  # every pointer, by name
        assert call_bwd(L, 3, ok, **{n: None}) == -1, n
        msg = L.maxk_last_error()
        assert n.encode() in msg and b"NULL" in msg, (n, msg)
    assert call_bwd(L, 3, (10, 0, 5, 64, 8, 0)) == -1  # edges and no column to hold them
    assert b"edges present" in L.maxk_last_error()
    assert call_bwd(L, 3, (10, 1 << 24, 5, 64, 8, 0)) == -1  # a table past 2^24 columns
    assert b"2^24 columns" in L.maxk_last_error()
    assert call_bwd(L, 3, (10, 1 << 23, 5, 256, 128, 0)) == -1  # ... or 4 GiB of records
    assert b"4 GiB of records" in L.maxk_last_error()
    assert call_bwd(L, 3, ok, cbsr_val=ctypes.c_void_p(4098)) == -1
    assert b"4-B aligned" in L.maxk_last_error()
    for H in range(1, 9):  # every value in the range is accepted up to the workspace check
        for D, k in ((64, 3), (256, 96), (9, 7), (256, 256)):
            assert call_bwd(L, H, (10, 10, 5, D, k, 0), ws_bytes=0) == -1
            assert b"workspace too small" in L.maxk_last_error()


def test_no_edges():
    """num_e == 0: two outputs to zero, so null outputs are an error; an empty graph of no rows
    and no columns has nothing to write."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    assert call_bwd(L, 8, (0, 0, 0, 64, 8, 64), p=None, ws=None, ws_bytes=0) == 0
    assert L.maxk_last_error() == b""
    assert call_bwd(L, 3, (10, 10, 0, 64, 8, 0), p=None, ws=None, ws_bytes=0) == -1
    assert b"grad_q" in L.maxk_last_error()


SHAPES = [(600, 600, 7000, 256, 16, 0), (600, 600, 7000, 64, 3, 64), (150, 700, 6000, 256, 96, 0),
          (1, 1, 1, 9, 7, 0), (232965, 232965, 114615891, 256, 16, 0),
          (2449029, 2449029, 123718280, 256, 32, 0)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_workspace_query_and_short_workspace(shape):
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    rows, cols, e, D, k, chunk = shape
    sizes = [L.maxk_dot_attention_heads_backward_workspace_size(rows, cols, e, D, k, H, chunk)
             for H in range(1, 9)]
    assert all(n > 0 and n % 256 == 0 for n in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))  # non-decreasing in H
    for H, n in zip(range(1, 9), sizes):
        HP = 2 if H <= 2 else 4 if H <= 4 else 8
        # T with its dummy row, the records and glT
        assert n >= 4 * k * (e + 1) + 6 * k * cols + 4 * HP * e
        if e > 10 ** 8:  # beside T, glT and the records: B's slabs, far from a second [H, E]
            assert n - 4 * k * (e + 1) - 4 * HP * e - 16 * k * cols < 2 * H * e
        assert call_bwd(L, H, shape, ws_bytes=n - 1) == -1
        assert b"workspace too small" in L.maxk_last_error()
    n = sizes[4]
    assert call_bwd(L, 5, shape, ws=None, ws_bytes=n) == -1
    assert b"workspace too small" in L.maxk_last_error()
    assert call_bwd(L, 5, shape, ws=ctypes.c_void_p(4096 + 16), ws_bytes=n) == -1
    assert b"256-B aligned" in L.maxk_last_error()


def test_workspace_upper_bound():
    """Reddit-sized (the shape of test_dot_attention_cpu.py's
    test_workspace_slabs_at_the_auto_chunk) at 8 heads, chunk_edges = 0: below the GAT backward's
    workspace at the same shape plus 2 H E bytes.  The GAT entry already holds T, the phase-2
    slabs, the records and one [E, HP] array; what this entry adds are the hub-row slabs of the
    grad_q walk, H / 2 bytes per edge at the forward's largest auto item of 2048 tokens and at
    most H * D * 4 bytes for each of the auto rule's items.  One array of HP * E floats, never
    room for a second."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    R = C = 232965
    E, D, k, H = 114615891, 256, 16, 8
    n = L.maxk_dot_attention_heads_backward_workspace_size(R, C, E, D, k, H, 0)
    gat = L.maxk_gat_attention_heads_backward_workspace_size(R, C, E, D, k, H, 0)
    assert 0 < n < gat + 2 * H * E
    assert n - 4 * k * (E + 1) - 4 * 8 * E < 4 * 8 * E  # no second [E, HP] array
    # the slabs are the only part that depends on D: [H, items, D] floats, so halving D at 2048
    # tokens per item frees H / 4 bytes per token
    size = L.maxk_dot_attention_heads_backward_workspace_size
    items = -(-(R + E) // 2048)
    half = size(R, C, E, D, k, H, 2048) - size(R, C, E, D // 2, k, H, 2048)
    assert abs(half - items * H * (D // 2) * 4) <= 256
    assert abs(2 * half / (R + E) - H / 2) < 0.01


@pytest.mark.parametrize("chunk", [0, 64])
def test_workspace_query_monotone_in_edges(chunk):
    """More edges never need less workspace, at 3 and at 8 heads."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    size = L.maxk_dot_attention_heads_backward_workspace_size
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
    monkeypatch.delenv(ENV, raising=False)
    for H in range(1, 9):  # the measured rule: the fused backward everywhere
        for rows, e in ((232965, 114615892), (2449029, 123718280), (600, 7000)):
            for k in (16, 32):
                assert mk.dot_attention_backward_route(H, rows, e, k) == "fused"
    for forced in ("fused", "rebuilt"):
        monkeypatch.setenv(ENV, forced)
        for H in (1, 2, 8):
            assert mk.dot_attention_backward_route(H, 1000, 50000, 16) == forced
    monkeypatch.setenv(ENV, "something else")
    assert mk.dot_attention_backward_route(4, 1000, 50000, 16) == "fused"


def test_defaults_and_environment_override(monkeypatch):
    """backward defaults to "rebuilt" in the function, the graph's method and the layer;
    MAXK_DOT_ATTN_BWD overrides the method's and the layer's argument; other words are refused
    as arguments and ignored in the environment."""
    import maxk_layers as ML
    import maxk_spgemm_function as MF
    monkeypatch.delenv(ENV, raising=False)
    monkeypatch.delenv("MAXK_DOT_ATTN", raising=False)
    assert inspect.signature(MF.maxk_dot_attention_heads).parameters["backward"].default == \
        "rebuilt"
    assert inspect.signature(
        MF.MaxKDotAttentionHeadsFunction.forward).parameters["backward"].default == "rebuilt"
    assert inspect.signature(ML.CSRGraph.dot_attend_heads).parameters["backward"].default == \
        "rebuilt"
    assert inspect.signature(
        ML.MaxKTransformerConv.__init__).parameters["attention_backward"].default == "rebuilt"
    assert ML.MaxKTransformerConv(12, 5, 3).attention_backward_mode() == "rebuilt"
    assert ML.MaxKTransformerConv(12, 5, 3).attention_mode() == "stored"
    conv = ML.MaxKTransformerConv(12, 5, 3, attention="fused", attention_backward="fused")
    assert conv.attention_backward_mode() == "fused" and conv.attention_mode() == "fused"
    with pytest.raises(ValueError, match="attention_backward"):
        ML.MaxKTransformerConv(12, 5, 3, attention_backward="both")
    rp = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(ValueError, match="backward"):
        ML.CSRGraph(rp, rp[:1]).dot_attend_heads(None, None, 4, None, 0.5, backward="both")
    q = torch.zeros(1, 1, 4)
    with pytest.raises(ValueError, match="backward"):
        MF.MaxKDotAttentionHeadsFunction.apply(rp, rp[:1], q, q[0], q[0], 4, 0.5, "both")
    for forced in ("fused", "rebuilt"):
        monkeypatch.setenv(ENV, forced)
        for arg in ("fused", "rebuilt"):
            assert ML.MaxKTransformerConv(
                12, 5, 3, attention_backward=arg).attention_backward_mode() == forced
    monkeypatch.setenv(ENV, "neither")
    assert ML.MaxKTransformerConv(
        12, 5, 3, attention_backward="fused").attention_backward_mode() == "fused"


def test_fused_backward_layer_still_refuses_dropout(monkeypatch):
    """attn_drop > 0 with the fused walk keeps raising, whatever the backward."""
    import maxk_layers as ML
    monkeypatch.delenv("MAXK_DOT_ATTN", raising=False)
    monkeypatch.delenv(ENV, raising=False)
    rp = torch.tensor([0, 2, 3], dtype=torch.int32)
    col = torch.tensor([0, 1, 1], dtype=torch.int32)
    g = ML.CSRGraph(rp, col)
    x, cv, ci = torch.zeros(2, 4), torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.uint8)
    conv = ML.MaxKTransformerConv(4, 3, 2, attention="fused", attn_drop=0.5,
                                  attention_backward="fused")
    with pytest.raises(ValueError, match="no dropout yet"):
        conv(g, x, cv, ci)
