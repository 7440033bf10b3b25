"""CPU: the reference of the attention dropout inside the fused dot-product attention, the C ABI
surface of the two dropout entries, their host validation and size queries, and the layer's
opt-in keyword.

tests/dot_attn_dropout_ref.py is the yardstick of test_dot_attn_dropout_gpu.py, so it is pinned
here against float64 torch autograd of the dense composition of test_dot_attention_cpu.py with the
same mask d multiplied into the masked softmax (V = 40, H = 3: a graph with an empty row, a hub,
an unread column, a repeated selector and one past D).  No kernel is launched."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import dot_attention_bwd_ref as DB
import dot_attn_dropout_ref as DD
import numerics as N
from conftest import PKG
from test_boundary_cpu import declared_symbols
from test_dot_attention_cpu import dense_features, small_problem

FWD = "maxk_dot_attention_heads_dropout"
BWD = "maxk_dot_attention_heads_dropout_backward"
SYMBOLS = (FWD, FWD + "_workspace_size", BWD, BWD + "_workspace_size")
H = 3


# ------------------------------------------------------------------------------- the yardstick
def reference(scale, p, seed, G=None, cv=None):
    g, ci, cv0, q, D = small_problem()
    cv = cv0 if cv is None else cv
    q = q[:H]
    if G is None:
        G = np.random.default_rng(2911).standard_normal((H, g.R, D)).astype(np.float32)
    n = N.count_fwd(g, ci, D)
    ad, a, d = DD.attention(g.rp, g.col, q, scale, cv, ci, D, n, p, seed)
    b = DD.backward(g, a, ad, d, q, scale, cv, ci, G, D, DD.rounded_out_err(ad), n)
    return g, ci, cv, q, D, G, n, a, ad, d, b


def dense_dropped(g, ci, cv, q, D, scale, G, d):
    """out and (grad q, grad cv) of sum(out * G) in float64 torch, dense over the adjacency, the
    same d multiplied into the masked softmax."""
    R_, C = g.R, g.C
    rows = torch.from_numpy(np.repeat(np.arange(R_), np.diff(g.rp)))
    cols = torch.from_numpy(g.col.astype(np.int64))
    A = torch.zeros(R_, C, dtype=torch.float64)
    A[rows, cols] = 1.0
    Dm = torch.zeros(d.shape[0], R_, C, dtype=torch.float64)
    Dm[:, rows, cols] = torch.from_numpy(d)
    v = torch.from_numpy(cv.astype(np.float64)).requires_grad_(True)
    X = torch.zeros(C, 256, dtype=torch.float64).index_put(
        (torch.arange(C)[:, None].expand(-1, ci.shape[1]), torch.from_numpy(ci.astype(np.int64))),
        v, accumulate=True)[:, :D]
    assert torch.equal(X.detach(), dense_features(ci, cv, D))
    qt = torch.from_numpy(q.astype(np.float64)).requires_grad_(True)
    e = scale * torch.einsum("hrd,cd->hrc", qt, X)
    masked = (A == 0) & (A.sum(1, keepdim=True) > 0)
    alpha = torch.softmax(e.masked_fill(masked, float("-inf")), 2) * A
    out = (alpha * Dm) @ X
    grads = torch.autograd.grad(out, [qt, v], torch.from_numpy(G.astype(np.float64)))
    return out.detach().numpy(), [t.numpy() for t in grads]


@pytest.mark.parametrize("p", [0.5, 0.9])
@pytest.mark.parametrize("scale", [1.0, 0.25])
def test_reference_agrees_with_dense_torch_autograd(scale, p):
    g, ci, cv, q, D, G, n, a, ad, d, b = reference(scale, p, 77)
    assert g.R == 40 and q.shape[0] == H
    assert (d == 0).any() and (d > 0).any()
    out, (want_q, want_v) = dense_dropped(g, ci, cv, q, D, scale, G, d)
    assert np.abs(ad.out - out).max() <= 1e-12 * max(1.0, np.abs(out).max())
    got_v, v_bound = DB.cbsr(b, H)
    for name, got, ref in (("q", b.g_q, want_q), ("cbsr", got_v, want_v)):
        err = np.abs(got - ref).max()
        print(f"\ndot_attn_dropout_ref vs torch autograd, scale {scale} p {p}: {name} {err:.3g}")
        assert got.shape == ref.shape and err <= 1e-12 * max(1.0, np.abs(ref).max()), name
    # the statistics and the logits are the undropped softmax's
    assert ad.m is a.m and ad.z is a.z and ad.l is a.l
    # the t identity: sum_e alpha d ga == out . grad_out, to float64 rounding (b.ga holds d ga)
    te = np.stack([np.bincount(a.heads[h].rows, a.w[h] * b.ga[h], minlength=g.R)
                   for h in range(H)])
    assert np.abs(te - b.t).max() <= 1e-12 * max(1.0, np.abs(b.t).max())
    # structure: bounds are finite and non-negative, 0 exactly where nothing is added
    for ref, bound in ((ad.out, ad.out_bound), (b.g_q, b.g_q_bound), (got_v, v_bound)):
        assert np.isfinite(bound).all() and (bound >= 0).all() and (ref[bound == 0] == 0).all()
    assert (ad.out_bound[:, n == 0] == 0).all() and ((ad.out_bound > 0) == (n > 0)[None]).all()
    assert (got_v[g.unread] == 0).all() and (v_bound[g.unread] == 0).all()
    assert got_v[9, 1] == 0 and v_bound[9, 1] == 0           # the selector past D


def test_rate_zero_is_the_reference_without_dropout():
    g, ci, cv, q, D, G, n, a, ad, d, b = reference(0.5, 0.0, 5)
    assert (d == 1).all()
    assert np.array_equal(ad.out, a.out) and np.array_equal(ad.w, a.w)
    plain = DB.backward(g, a, q, 0.5, cv, ci, G, D, DB.rounded_out_err(a), n)
    assert np.abs(plain.g_q - b.g_q).max() <= 1e-13 * max(1.0, np.abs(b.g_q).max())
    x, y = DB.cbsr(plain, H)[0], DB.cbsr(b, H)[0]
    assert np.abs(x - y).max() <= 1e-13 * max(1.0, np.abs(y).max())


def test_rounded_reference_is_inside_its_bounds():
    g, ci, cv, q, D, G, n, a, ad, d, _ = reference(0.25, 0.5, 5)
    for out_err in (DD.rounded_out_err(ad), ad.out_bound):
        b = DD.backward(g, a, ad, d, q, 0.25, cv, ci, G, D, out_err, n)
        gc, gcb = DB.cbsr(b, H)
        for ref, bound in ((ad.out, ad.out_bound), (b.gl, b.gl_bound), (b.g_q, b.g_q_bound),
                           (gc, gcb)):
            assert N.within(ref.astype(np.float32), ref, bound, "rounded") <= 0.5


def test_t_skips_the_columns_where_the_dropped_out_is_zero():
    """A NaN of G in a column of a row where the dropped out is exactly 0 -- no addend, or every
    addend dropped -- does not reach t; where every addend is dropped it still reaches ga of the
    dropped edges, and d ga = 0 * NaN: dropping does not shield.  In a column without an addend
    it reaches nothing."""
    g, ci, cv, q, D, G, n, a, ad, d, clean = reference(0.5, 0.9, 3)
    zero = ad.out == 0
    assert (zero & (n > 0)[None]).any()  # columns all of whose addends are dropped
    G2 = G.copy()
    G2[zero] = np.nan
    b = reference(0.5, 0.9, 3, G=G2)[-1]
    assert np.array_equal(clean.t, b.t) and np.isnan(b.ga).any()
    G3 = G.copy()
    G3[:, n == 0] = np.nan
    b = reference(0.5, 0.9, 3, G=G3)[-1]
    for x, y in zip(clean[:8], b[:8]):
        assert np.array_equal(x, y)


def test_dropping_does_not_shield():
    """0 * NaN and 0 * Inf are NaN: a dropped edge's Inf value reaches the output."""
    g, ci, cv, q, D, G, n, a, ad, d, _ = reference(0.5, 0.5, 77)
    e = int(np.flatnonzero((d[0] == 0) & (d[1] > 0))[0])
    c = g.col[e]
    l = int(np.flatnonzero(ci[c] < D)[0])
    cv2 = cv.copy()
    cv2[c, l] = np.inf
    ad2 = reference(0.5, 0.5, 77, cv=cv2)[8]
    r = np.repeat(np.arange(g.R), np.diff(g.rp))[e]
    assert np.isnan(ad2.out[0, r, ci[c, l]])


# ------------------------------------------------------------------------------- the C ABI
def test_symbols_declared_exported_and_bound():
    from maxk_cuda_kernels import _capi
    syms = declared_symbols()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libmaxk_hip.so"))
    for s in SYMBOLS:
        assert s in syms and hasattr(lib, s) and s in _capi.SIGNATURES, s
    i32, i64, p, f32, sz, u64 = (ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float,
                                 ctypes.c_size_t, ctypes.c_uint64)
    # the entries they extend with (float p, uint64_t seed) inserted before the workspace
    for drop, plain in ((FWD, "maxk_dot_attention_heads"),
                        (BWD, "maxk_dot_attention_heads_backward")):
        res, args = _capi.SIGNATURES[plain]
        assert _capi.SIGNATURES[drop] == (res, args[:-3] + [f32, u64] + args[-3:])
        assert _capi.SIGNATURES[drop + "_workspace_size"] == \
            _capi.SIGNATURES[plain + "_workspace_size"] == (sz, [i64] * 3 + [i32] * 4)
    assert _capi.SIGNATURES[FWD] == (ctypes.c_int, [p] * 3 + [f32] + [p] * 5 + [i64] * 3
                                     + [i32] * 4 + [f32, u64, p, sz, p])
    assert _capi.SIGNATURES[BWD] == (ctypes.c_int, [p] * 5 + [f32] + [p] * 8 + [i64] * 3
                                     + [i32] * 4 + [f32, u64, p, sz, p])
    import maxk_cuda_kernels as mk
    assert mk.version() == 100  # an addition: the ABI version stays
    for fn in (mk.dot_attention_heads, mk.dot_attention_heads_backward):
        ps = inspect.signature(fn).parameters
        assert list(ps)[-2:] == ["dropout", "seed"]
        assert ps["dropout"].default == 0.0 and ps["seed"].default == 0


P = ctypes.c_void_p(4096)  # a fake non-null, 256-B aligned device pointer: never dereferenced
OK = (10, 10, 5, 64, 8, 3, 0)  # rows, cols, e, D, k, H, chunk


def call_fwd(L, p, seed=1, shape=OK, ws_bytes=1 << 42, **named):
    names = "row_ptr col_idx q cbsr_val cbsr_idx out row_max row_sum".split()
    a = {n: named.get(n, P) for n in names}
    return L.maxk_dot_attention_heads_dropout(
        a["row_ptr"], a["col_idx"], a["q"], 0.5, a["cbsr_val"], a["cbsr_idx"], a["out"],
        a["row_max"], a["row_sum"], *shape, p, seed, P, ws_bytes, None)


def call_bwd(L, p, seed=1, shape=OK, ws_bytes=1 << 42, **named):
    names = ("row_ptr col_idx col_ptr csc_eid q cbsr_val cbsr_idx out row_max row_sum grad_out "
             "grad_q grad_cbsr").split()
    a = {n: named.get(n, P) for n in names}
    return L.maxk_dot_attention_heads_dropout_backward(
        a["row_ptr"], a["col_idx"], a["col_ptr"], a["csc_eid"], a["q"], 0.5, a["cbsr_val"],
        a["cbsr_idx"], a["out"], a["row_max"], a["row_sum"], a["grad_out"], a["grad_q"],
        a["grad_cbsr"], *shape, p, seed, P, ws_bytes, None)


def test_host_side_validation():
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    for p in (-0.1, 1.0, 1.5, math.nan, math.inf):  # before any launch: the pointers are fakes
        for rc in (call_fwd(L, p), call_bwd(L, p)):
            assert rc == -1, p
            assert b"p must be in [0, 1)" in L.maxk_last_error()
    for p in (0.0, 0.5):  # p == 0 takes the entry without dropout's checks, p > 0 the same ones
        for call in (call_fwd, call_bwd):
            for Hx in (0, 9):
                assert call(L, p, shape=OK[:5] + (Hx, 0)) == -1
                assert b"num_heads must be in [1,8]" in L.maxk_last_error()
            assert call(L, p, ws_bytes=0) == -1
            assert b"workspace too small" in L.maxk_last_error()
        for n in "row_ptr col_idx q cbsr_val cbsr_idx out row_max row_sum".split():
            assert call_fwd(L, p, **{n: None}) == -1, n
            msg = L.maxk_last_error()
            assert n.encode() in msg and b"NULL" in msg, (n, msg)
        for n in ("row_ptr col_idx col_ptr csc_eid q cbsr_val cbsr_idx out row_max row_sum "
                  "grad_out grad_q grad_cbsr").split():
            assert call_bwd(L, p, **{n: None}) == -1, n
            msg = L.maxk_last_error()
            assert n.encode() in msg and b"NULL" in msg, (n, msg)


@pytest.mark.parametrize("shape", [OK, (1000, 900, 5000, 256, 96, 8, 64), (600, 600, 7000, 64, 3, 1, 7),
                                   (1, 1, 1, 9, 7, 5, 0), (232965, 232965, 114615891, 256, 16, 8, 0)],
                         ids=lambda s: "x".join(map(str, s)))
def test_size_queries_are_those_of_the_entries_without_dropout(shape):
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    assert L.maxk_dot_attention_heads_dropout_workspace_size(*shape) == \
        L.maxk_dot_attention_heads_workspace_size(*shape) > 0
    assert L.maxk_dot_attention_heads_dropout_backward_workspace_size(*shape) == \
        L.maxk_dot_attention_heads_backward_workspace_size(*shape) > 0
    bad = shape[:5] + (9, shape[6])
    assert L.maxk_dot_attention_heads_dropout_workspace_size(*bad) == 0
    assert L.maxk_dot_attention_heads_dropout_backward_workspace_size(*bad) == 0


# ------------------------------------------------------------------------------- the layers
def tiny():
    import maxk_layers as ML
    rp = torch.tensor([0, 2, 3], dtype=torch.int32)
    col = torch.tensor([0, 1, 1], dtype=torch.int32)
    return (ML.CSRGraph(rp, col), rp, col, torch.zeros(2, 4), torch.zeros(2, 3),
            torch.zeros(2, 3, dtype=torch.uint8))


def test_keywords_and_defaults():
    import maxk_layers as ML
    import maxk_spgemm_function as MF
    for fn in (MF.maxk_dot_attention_heads, MF.MaxKDotAttentionHeadsFunction.forward,
               ML.CSRGraph.dot_attend_heads):
        ps = inspect.signature(fn).parameters
        assert list(ps)[-3:] == ["backward", "dropout", "seed"]
        assert ps["backward"].default == "rebuilt" and ps["dropout"].default == 0.0
        assert ps["seed"].default == 0
    ps = inspect.signature(ML.MaxKTransformerConv.__init__).parameters
    assert list(ps)[-1] == "fused_attn_drop" and ps["fused_attn_drop"].default is False


@pytest.mark.parametrize("bwd", ["rebuilt", "fused"])
def test_layer_opt_in_reaches_the_binding(monkeypatch, bwd):
    """fused_attn_drop=True in training mode with CPU tensors: the binding's "must be CUDA tensor"
    error, not the layer's ValueError -- no fallback either; the default keeps the ValueError."""
    import maxk_layers as ML
    monkeypatch.delenv("MAXK_DOT_ATTN", raising=False)
    monkeypatch.delenv("MAXK_DOT_ATTN_BWD", raising=False)
    g, rp, col, x, cv, ci = tiny()
    conv = ML.MaxKTransformerConv(4, 3, 2, attention="fused", attn_drop=0.5,
                                  attention_backward=bwd, fused_attn_drop=True)
    seen = []
    real = ML.maxk_dot_attention_heads
    monkeypatch.setattr(ML, "maxk_dot_attention_heads",
                        lambda *a: seen.append(a[-3:]) or real(*a))
    with pytest.raises(RuntimeError, match="must be CUDA tensor"):
        conv(g, x, cv, ci, attn_seed=11)
    assert seen == [(bwd, 0.5, 11)]
    conv.eval()  # no dropout in eval(): the call without the two numbers
    with pytest.raises(RuntimeError, match="must be CUDA tensor"):
        conv(g, x, cv, ci, attn_seed=11)
    assert seen[1] == (bwd, 0.0, 0)
    plain = ML.MaxKTransformerConv(4, 3, 2, attention="fused", attn_drop=0.5,
                                   attention_backward=bwd)
    with pytest.raises(ValueError, match="no dropout yet"):
        plain(g, x, cv, ci)
    # the stored path is untouched by the keyword
    stored = ML.MaxKTransformerConv(4, 3, 2, attn_drop=0.5, fused_attn_drop=True)
    assert stored.attention_mode() == "stored"


def test_binding_refuses_cpu_tensors():
    """No fallback: a CPU tensor is an error in the binding with dropout as without."""
    import maxk_cuda_kernels as mk
    _, rp, col, x, cv, ci = tiny()
    q = torch.zeros(2, 2, 4)
    st = torch.zeros(2, 2)
    with pytest.raises(RuntimeError, match="must be CUDA tensor"):
        mk.dot_attention_heads(rp, col, q, cv, ci, 4, 0.5, dropout=0.5, seed=1)
    with pytest.raises(RuntimeError, match="must be CUDA tensor"):
        mk.dot_attention_heads_backward(rp, col, q, cv, ci, q, st, st, q, 0.5, dropout=0.5,
                                        seed=1)
