"""CPU: the multi-head aggregation's reference helper, its C ABI surface, host validation and
the layer's host logic.

tests/heads_ref.py is the yardstick of test_heads_gpu.py (the reference project has no attention
and the CPU oracle no multi-head function), so it is pinned here against torch autograd on a
dense float64 restatement: A_h built from the CSR with w[h].requires_grad, X = scatter(cbsr) with
the values requiring grad, sum_h <(A_h @ X) / div, G[h]>.backward().  No kernel is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import edge_grad_ref as R
import heads_ref as HR
import numerics as N
from conftest import PKG
from test_boundary_cpu import declared_symbols

SYMBOLS = ("maxk_spgemm_forward_heads", "maxk_spgemm_forward_heads_workspace_size",
           "maxk_edge_weight_grad_heads", "maxk_edge_weight_grad_heads_workspace_size")


# ------------------------------------------------------------------------------- the yardstick
def small_problem():
    """V = 12, D = 9, k = 3, H = 3: an empty row, a repeated selector, a selector >= D."""
    from test_parity_gpu import rand_graph
    rng = np.random.default_rng(1293)
    V, D, k, H = 12, 9, 3, 3
    rp, col = rand_graph(rng, V, 4, empty=1)
    g = N.make_graph(rng, rp, col, V)
    assert (np.diff(g.rp) == 0).any()
    w = rng.uniform(0.5, 1.5, (H, g.col.size)).astype(np.float32)
    cv = rng.standard_normal((V, k)).astype(np.float32)
    ci = np.stack([rng.choice(D, k, replace=False) for _ in range(V)]).astype(np.uint8)
    read = np.unique(g.col)
    a, b = int(read[0]), int(read[1])
    ci[a, 2] = ci[a, 0]  # a repeated selector
    ci[b, 1] = 200       # a selector >= D
    G = rng.standard_normal((H, V, D)).astype(np.float32)
    return g, w, cv, ci, G, D


def autograd_heads(g, w, cv, ci, G, D, div):
    """(out [H, R, D], d/dw [H, E], d/dcv [C, k]) of the dense float64 restatement."""
    H = w.shape[0]
    rows = torch.from_numpy(R.edge_rows(g.rp))
    cols = torch.from_numpy(g.col.astype(np.int64))
    wt = torch.from_numpy(w.astype(np.float64)).requires_grad_(True)
    cvt = torch.from_numpy(cv.astype(np.float64)).requires_grad_(True)
    X = torch.zeros(g.C, D, dtype=torch.float64)
    for c in range(g.C):
        for l in range(ci.shape[1]):
            if ci[c, l] < D:
                X = X.index_put((torch.tensor(c), torch.tensor(int(ci[c, l]))), cvt[c, l],
                                accumulate=True)
    outs = []
    for h in range(H):
        A = torch.zeros(g.R, g.C, dtype=torch.float64).index_put((rows, cols), wt[h],
                                                                 accumulate=True)
        o = A @ X
        if div:
            o = o / torch.from_numpy(g.div.astype(np.float64))[:, None]
        outs.append(o)
    out = torch.stack(outs)
    out.backward(torch.from_numpy(G.astype(np.float64)))
    return out.detach().numpy(), wt.grad.numpy(), cvt.grad.numpy()


@pytest.mark.parametrize("div", [True, False], ids=["div", "nodiv"])
def test_reference_agrees_with_autograd(div):
    g, w, cv, ci, G, D = small_problem()
    out, gw, gcv = autograd_heads(g, w, cv, ci, G, D, div)
    H = w.shape[0]
    # the forward: the fp32 oracle per head, within its own bound of the exact result
    yo = HR.fwd_heads_ref(g, w, cv, ci, D, div)
    by = HR.bound_fwd_heads(g, w, cv, ci, D, div)
    assert yo.shape == by.shape == (H, g.R, D)
    assert (np.abs(yo - out) <= by).all()
    assert (by[:, np.diff(g.rp) == 0] == 0).all() and (yo[:, np.diff(g.rp) == 0] == 0).all()
    # the edge gradient: float64 against float64
    er = HR.edge_grad_heads_ref(g, cv, ci, G, div)
    assert er.ref.shape == er.n.shape == er.s_abs.shape == (H, g.col.size)
    rel = np.abs(er.ref - gw) / np.maximum(np.abs(gw), np.finfo(np.float64).tiny)
    rel = np.where(er.ref == gw, 0.0, rel)
    print(f"\nheads edge gradient vs autograd: max relative difference {rel.max():.3g}")
    assert rel.max() <= 1e-12
    assert (er.n == (ci[g.col] < D).sum(1)[None, :]).all()
    be = HR.bound_edge_heads(er)
    assert be.shape == er.ref.shape and (be[er.n > 0] > 0).all()
    assert all(a.shape == (2, g.col.size) for a in HR.heads_slice(er, 2))
    # the feature gradient: the fp32 oracle per head summed in double, n = sum_h n_h
    gf = HR.feat_grad_heads_ref(g, w, G, ci, div)
    bf = HR.bound_feat_grad_heads(g, w, G, ci, div)
    assert gf.shape == bf.shape == cv.shape
    # a repeated selector's slots each get the column's gradient; one >= D gets none
    kept = ci < D
    assert (np.abs(gf - gcv)[kept] <= bf[kept]).all()
    assert (gf[~kept] == 0).all()
    one = N.bound_bwd(HR.head_graph(g, w[0], div), G[0], ci)
    assert (bf >= one).all()  # more addends and more magnitude than any one head


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
    assert callable(mk.spgemm_forward_heads) and callable(mk.edge_weight_grad_heads)
    assert mk.MAX_HEADS == 8
    with open(os.path.join(PKG, "..", "include", "maxk_hip.h")) as f:
        assert "#define MAXK_MAX_HEADS 8" in f.read()
    assert mk.version() == 100  # an addition: the ABI version stays
    import maxk_spgemm_function as F
    assert callable(F.maxk_spgemm_heads) and hasattr(F, "MaxKSpGEMMHeadsFunction")


FWD, GRAD = "maxk_spgemm_forward_heads", "maxk_edge_weight_grad_heads"


def call(L, name, *shape, ws=None, ws_bytes=0, ptr=4096):
    """An entry with fake non-null device pointers: rejected on the host or not called with a
    launchable shape.  shape = (rows, cols, e, D, k, H, chunk)."""
    p = ctypes.c_void_p(ptr)
    return getattr(L, name)(p, p, p, p, p, None, p, *shape, ws, ws_bytes, None)


@pytest.mark.parametrize("name", [FWD, GRAD])
def test_host_side_validation(name):
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    fn = getattr(L, name)
    #                     rows cols  e   D   k  H chunk
    for H in (0, 9, -1):
        assert call(L, name, 10, 10, 5, 64, 16, H, 0) == -1
        assert b"num_heads" in L.maxk_last_error()
        assert getattr(L, name + "_workspace_size")(10, 10, 5, 64, 16, H, 0) == 0
    assert call(L, name, 10, 10, 5, 64, 65, 3, 0) == -1     # k > D
    assert b"dim_k" in L.maxk_last_error()
    assert call(L, name, 10, 10, 5, 64, 0, 3, 0) == -1      # k = 0
    assert b"dim_k" in L.maxk_last_error()
    assert call(L, name, 10, 10, 5, 257, 16, 3, 0) == -1    # D past the uint8 selector range
    assert b"dim_origin" in L.maxk_last_error()
    assert call(L, name, -1, 10, 5, 64, 16, 3, 0) == -1     # negative sizes
    assert b"num_rows" in L.maxk_last_error()
    assert call(L, name, 10, 10, -5, 64, 16, 3, 0) == -1
    assert b"num_e" in L.maxk_last_error()
    assert call(L, name, 10, 10, 5, 64, 16, 3, -1) == -1
    assert b"chunk_edges" in L.maxk_last_error()
    # null pointers with edges present
    assert fn(None, None, None, None, None, None, None, 10, 10, 5, 64, 16, 3, 0, None, 0,
              None) == -1
    assert b"NULL" in L.maxk_last_error()
    # tables past 2^24 columns are rejected, with a message naming the argument
    assert call(L, name, 10, (1 << 24) + 1, 5, 64, 16, 3, 0) == -1
    assert b"num_cols" in L.maxk_last_error()


def test_empty_problems_return_ok():
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    # the gradient: num_e == 0 launches nothing and succeeds, whatever the pointers
    assert L.maxk_edge_weight_grad_heads(None, None, None, None, None, None, None, 10, 10, 0, 64,
                                         16, 3, 0, None, 0, None) == 0
    assert L.maxk_last_error() == b""
    # the forward: no rows, nothing to write (with rows and no edges it writes zeros: a launch,
    # test_heads_gpu.py)
    assert L.maxk_spgemm_forward_heads(None, None, None, None, None, None, None, 0, 10, 0, 64,
                                       16, 3, 0, None, 0, None) == 0
    assert L.maxk_last_error() == b""
    # range errors are reported even then
    assert L.maxk_edge_weight_grad_heads(None, None, None, None, None, None, None, 10, 10, 0, 64,
                                         16, 9, 0, None, 0, None) == -1
    assert L.maxk_spgemm_forward_heads(None, None, None, None, None, None, None, 0, 10, 0, 64,
                                       65, 3, 0, None, 0, None) == -1


@pytest.mark.parametrize("name", [FWD, GRAD])
@pytest.mark.parametrize("shape", [(1000, 1000, 100000, 256, 16, 4, 0),
                                   (150, 700, 6000, 9, 7, 3, 64),
                                   (400, 400, 64000, 256, 96, 8, 0),
                                   (600, 600, 7000, 64, 3, 1, 0)])
def test_workspace_query_and_short_workspace(name, shape):
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    n = getattr(L, name + "_workspace_size")(*shape)
    assert n > 0 and n % 256 == 0
    cols, k = shape[1], shape[4]
    assert n >= cols * 6 * k  # one record [k f32 | k u16] per column
    # one byte short: rejected on the host, before anything could be launched (the device
    # pointers are fake: a launch would not return -1 with this message)
    ws = ctypes.c_void_p(1 << 20)
    assert call(L, name, *shape, ws=ws, ws_bytes=n - 1) == -1
    assert b"workspace too small" in L.maxk_last_error()
    assert call(L, name, *shape, ws=None, ws_bytes=n) == -1
    assert b"workspace too small" in L.maxk_last_error()
    assert call(L, name, *shape, ws=ctypes.c_void_p((1 << 20) + 16), ws_bytes=n) == -1
    assert b"256-B aligned" in L.maxk_last_error()
    assert getattr(L, name + "_workspace_size")(-1, 10, 5, 64, 16, 3, 0) == 0
    assert getattr(L, name + "_workspace_size")(10, 10, 5, 64, 0, 3, 0) == 0


# ------------------------------------------------------------------------------- the layer
def test_multi_head_gat_conv_parameters_and_cpu_refusal():
    import maxk_layers as ML
    conv = ML.MaxKMultiHeadGATConv(12, 5, 3, negative_slope=0.1)
    shapes = {n: tuple(p.shape) for n, p in conv.named_parameters()}
    assert shapes == {"fc.weight": (15, 12), "attn_src": (3, 5), "attn_dst": (3, 5),
                      "bias": (3, 5)}
    assert "bias" not in dict(ML.MaxKMultiHeadGATConv(12, 5, 3, bias=False).named_parameters())
    for H in (0, 9):
        with pytest.raises(ValueError):
            ML.MaxKMultiHeadGATConv(12, 5, H)
    # no CPU fall-back: the layer and both helpers refuse CPU tensors
    g = ML.CSRGraph(torch.tensor([0, 2, 5, 6]), torch.tensor([0, 1, 0, 1, 2, 2]))
    vals = torch.rand(3, 2)
    idx = torch.tensor([[0, 1], [2, 3], [1, 0]], dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        g.aggregate_heads(vals, idx, 12, torch.rand(3, 6))
    with pytest.raises(RuntimeError):
        ML.gat_edge_softmax_heads(g, torch.rand(3, 3), torch.rand(3, 3))
    xs = torch.zeros(3, 12).scatter(1, idx.long(), vals)
    with pytest.raises(RuntimeError):
        conv(g, xs, vals, idx)
