"""CPU: the max aggregation's reference helper, its C ABI surface, host validation, workspace
sizes and the layers' arguments.

tests/max_aggregate_ref.py is the yardstick of test_max_aggregate_gpu.py, so it is pinned here
against dense float64 torch (amax over the adjacency-masked scattered CBSR, and its autograd
pulled back through the scatter) on the small graph of test_dot_attention_cpu -- an empty row, a
hub, an unread column, a repeated selector and a selector past D -- and against hand-written
cases of every rule.  No kernel is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import max_aggregate_ref as MR
from conftest import PKG
from test_boundary_cpu import declared_symbols
from test_dot_attention_cpu import small_problem

FWD = "maxk_spgemm_max_forward"
BWD = "maxk_spgemm_max_backward"
SYMBOLS = (FWD, BWD, FWD + "_workspace_size", BWD + "_workspace_size")


# ------------------------------------------------------------------------------- the yardstick
def dense_x(ci, cv, D):
    """X [C, D] float64 from a float64 leaf cv [C, k]: the CBSR scattered, repeated selectors
    added, selectors >= D dropped."""
    C, k = ci.shape
    X = torch.zeros(C, 256, dtype=cv.dtype)
    X = X.index_put((torch.arange(C)[:, None].expand(-1, k), torch.from_numpy(ci.astype(np.int64))),
                    cv, accumulate=True)
    return X[:, :D]


def dense_amax(g, X):
    """[R, D]: amax over each row's neighbours of X, 0 for a row without edges."""
    A = torch.zeros(g.R, g.C, dtype=torch.bool)
    rows = np.repeat(np.arange(g.R), np.diff(g.rp))
    A[torch.from_numpy(rows), torch.from_numpy(g.col.astype(np.int64))] = True
    m = X[None].expand(g.R, -1, -1).masked_fill(~A[:, :, None], float("-inf")).amax(1)
    return torch.where(A.any(1)[:, None], m, torch.zeros_like(m))


def test_reference_agrees_with_dense_torch():
    g, ci, cv, _, D = small_problem()
    out, arg = MR.forward(g.rp, g.col, cv, ci, D)
    assert out.dtype == np.float32 and arg.dtype == np.int32 and out.shape == arg.shape == (g.R, D)
    # the repeated selector's values are added in fp32, as the record pack adds them
    X = dense_x(ci, torch.from_numpy(cv), D).double()
    want = dense_amax(g, X).numpy()
    assert np.array_equal(out.astype(np.float64), want)
    deg = np.diff(g.rp)
    assert (deg == 0).any() and (out[deg == 0] == 0).all() and (arg[deg == 0] == -1).all()
    # arg names an edge of the row whose column holds the winner's value at j
    Xn = X.numpy()
    r, j = np.nonzero(arg >= 0)
    e = arg[r, j]
    assert ((g.rp[r] <= e) & (e < g.rp[r + 1])).all()
    assert np.array_equal(Xn[g.col[e], j], out[r, j].astype(np.float64))
    assert (out[arg < 0] == 0).all()
    pos, imp, neg = MR.outcomes(g.rp, g.col, cv, ci, D, out, arg)
    assert pos > 0 and imp > 0 and neg > 0, (pos, imp, neg)


def test_reference_gradient_agrees_with_dense_torch():
    """Tie-free random values: torch autograd of the dense amax, pulled back through the scatter,
    against the reference's grad_cbsr to 1e-12; exact zeros where nothing can arrive."""
    g, ci, cv, _, D = small_problem()
    _, arg = MR.forward(g.rp, g.col, cv, ci, D)
    cvt = torch.from_numpy(cv.astype(np.float64)).requires_grad_(True)
    out = dense_amax(g, dense_x(ci, cvt, D))
    rng = np.random.default_rng(9)
    G = rng.standard_normal((g.R, D)).astype(np.float32)
    out.backward(torch.from_numpy(G.astype(np.float64)))
    b = MR.backward(g.rp, g.col, ci, arg, G)
    want = cvt.grad.numpy()
    assert b.grad.shape == b.bound.shape == want.shape
    assert np.abs(b.grad - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert ((b.bound > 0) == (b.n > 0)).all() and (b.grad[b.n == 0] == 0).all()
    assert (b.n[g.unread] == 0).all()             # a column no edge reads
    assert b.n[9, 1] == 0                         # the selector past D
    assert np.array_equal(b.grad[7, 2], b.grad[7, 0]) and b.n[7, 2] == b.n[7, 0]  # both slots
    assert b.n.max() > 1


def one_row(slots, D=4):
    """One row whose edge e reads column e; slots[e] = [(selector, value), ...] padded to k
    with a selector >= D.  Returns (out[0], arg[0])."""
    k = max(len(s) for s in slots)
    n = len(slots)
    ci = np.full((n, k), D + 1, np.uint8)
    cv = np.full((n, k), 99.0, np.float32)
    for e, s in enumerate(slots):
        for l, (j, v) in enumerate(s):
            ci[e, l], cv[e, l] = j, v
    out, arg = MR.forward(np.array([0, n], np.int32), np.arange(n, dtype=np.int32), cv, ci, D)
    return out[0], arg[0]


def bits(x):
    return int(np.float32(x).view(np.uint32))


def test_rules_by_hand():
    nan, inf = np.nan, np.inf
    # a tie between two edges: the lower edge index
    o, a = one_row([[(0, 1.0)], [(0, 1.0)], [(0, 0.5)]])
    assert o[0] == 1.0 and a[0] == 0
    o, a = one_row([[(0, 0.5)], [(0, 1.0)], [(0, 1.0)]])
    assert o[0] == 1.0 and a[0] == 1
    # nobody keeps column 3: the implicit zero alone
    assert o[3] == 0 and bits(o[3]) == 0 and a[3] == -1
    # an explicit 0 against the implicit zero: the explicit value wins the tie
    o, a = one_row([[(0, 0.0)], [(1, 2.0)]])
    assert bits(o[0]) == 0 and a[0] == 0 and o[1] == 2.0 and a[1] == 1
    # negatives: with an edge that does not keep j the implicit zero wins; without, the largest
    o, a = one_row([[(0, -1.0)], [(0, -2.0)], [(1, 5.0)]])
    assert bits(o[0]) == 0 and a[0] == -1
    o, a = one_row([[(0, -2.0)], [(0, -1.0)]])
    assert o[0] == -1.0 and a[0] == 1
    # -0.0: wins a tie against the implicit zero and keeps its sign; ties +0.0, first wins
    o, a = one_row([[(0, -0.0)], [(1, 1.0)]])
    assert bits(o[0]) == 0x80000000 and a[0] == 0
    o, a = one_row([[(0, -0.0)], [(0, 0.0)]])
    assert bits(o[0]) == 0x80000000 and a[0] == 0
    o, a = one_row([[(0, 0.0)], [(0, -0.0)]])
    assert bits(o[0]) == 0 and a[0] == 0
    o, a = one_row([[(0, -3.0)], [(0, -0.0)]])
    assert bits(o[0]) == 0x80000000 and a[0] == 1
    # a NaN wins over everything, the first one stays
    o, a = one_row([[(0, nan)], [(0, 5.0)]])
    assert np.isnan(o[0]) and a[0] == 0
    o, a = one_row([[(0, 5.0)], [(0, nan)], [(0, nan)], [(0, inf)]])
    assert np.isnan(o[0]) and a[0] == 1
    o, a = one_row([[(0, -1.0)], [(0, nan)], [(1, 1.0)]])  # ... over the implicit zero too
    assert np.isnan(o[0]) and a[0] == 1
    # infinities order as values
    o, a = one_row([[(0, 1.0)], [(0, inf)], [(0, inf)]])
    assert o[0] == inf and a[0] == 1
    o, a = one_row([[(0, -inf)], [(0, -inf)]])
    assert o[0] == -inf and a[0] == 0
    o, a = one_row([[(0, -inf)], [(1, -inf)]])
    assert bits(o[0]) == 0 and a[0] == -1 and bits(o[1]) == 0 and a[1] == -1
    o, a = one_row([[(0, -inf)], [(0, -1e30)]])
    assert o[0] == np.float32(-1e30) and a[0] == 1
    # a repeated selector is one candidate carrying the sum; a selector past D is none
    o, a = one_row([[(0, 1.0), (0, 2.0)], [(0, 2.5)]])
    assert o[0] == 3.0 and a[0] == 0
    o, a = one_row([[(0, -4.0), (0, 1.0)], [(0, -3.5)]])
    assert o[0] == -3.0 and a[0] == 0
    o, a = one_row([[(7, 9.0), (1, -1.0)]], D=4)
    assert (o[[0, 2, 3]] == 0).all() and (a[[0, 2, 3]] == -1).all() and o[1] == -1.0 and a[1] == 0
    # the backward: only the winner's slots receive, all of them; a NaN elsewhere reaches nothing
    rp, col = np.array([0, 2, 2], np.int32), np.array([0, 1], np.int32)
    ci = np.array([[0, 0, 1], [0, 1, 9]], np.uint8)
    cv = np.array([[1.0, 1.0, -1.0], [1.5, -2.0, 0.0]], np.float32)
    out, arg = MR.forward(rp, col, cv, ci, 4)
    assert arg[0].tolist() == [0, 0, -1, -1] and out[0].tolist() == [2.0, -1.0, 0.0, 0.0]
    G = np.array([[3.0, 5.0, nan, nan], [nan] * 4], np.float32)
    b = MR.backward(rp, col, ci, arg, G)
    assert b.grad.tolist() == [[3.0, 3.0, 5.0], [0.0, 0.0, 0.0]]
    assert b.n.tolist() == [[1, 1, 1], [0, 0, 0]] and (b.bound[1] == 0).all()


# ------------------------------------------------------------------------------- the C ABI
def test_symbols_declared_exported_and_bound():
    from maxk_cuda_kernels import _capi
    syms = declared_symbols()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libmaxk_hip.so"))
    for s in SYMBOLS:
        assert s in syms and hasattr(lib, s) and s in _capi.SIGNATURES, s
    i32, i64, p, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    assert _capi.SIGNATURES[FWD] == (ctypes.c_int, [p] * 6 + [i64] * 3 + [i32] * 3 + [p, sz, p])
    assert _capi.SIGNATURES[BWD] == (ctypes.c_int, [p] * 8 + [i64] * 3 + [i32] * 2 + [p, sz, p])
    assert _capi.SIGNATURES[FWD + "_workspace_size"] == (sz, [i64] * 3 + [i32] * 3)
    assert _capi.SIGNATURES[BWD + "_workspace_size"] == (sz, [i64] * 3 + [i32] * 2)
    import maxk_cuda_kernels as mk
    for name in ("spgemm_max_forward", "spgemm_max_backward"):
        assert callable(getattr(mk, name)) and name in mk.__all__
    assert mk.version() == 100  # an addition: the ABI version stays
    import maxk_layers as ML
    import maxk_spgemm_function as MF
    assert issubclass(MF.MaxKSpGEMMMaxFunction, torch.autograd.Function)
    assert callable(MF.maxk_spgemm_max) and callable(ML.CSRGraph.aggregate_max)


def test_binding_refuses_cpu_tensors():
    """No fallback: a CPU tensor is an error in the binding, the autograd function, the graph's
    method and both layers."""
    import maxk_cuda_kernels as mk
    import maxk_layers as ML
    import maxk_spgemm_function as MF
    rp = torch.tensor([0, 2, 3], dtype=torch.int32)
    col = torch.tensor([0, 1, 1], dtype=torch.int32)
    cv = torch.zeros(2, 3)
    ci = torch.zeros(2, 3, dtype=torch.uint8)
    arg = torch.zeros(2, 4, dtype=torch.int32)
    g = ML.CSRGraph(rp, col)
    x = torch.zeros(2, 4)
    calls = [lambda: mk.spgemm_max_forward(rp, col, cv, ci, 4),
             lambda: mk.spgemm_max_backward(rp, col, ci, arg, x, 3),
             lambda: MF.maxk_spgemm_max(rp, col, cv, ci, 4),
             lambda: g.aggregate_max(cv, ci, 4),
             lambda: ML.MaxKGINConv(aggregator_type="max")(g, x, cv, ci)]
    for call_ in calls:
        with pytest.raises(RuntimeError, match="must be CUDA tensor"):
            call_()


P = ctypes.c_void_p(4096)  # a fake non-null, 256-B aligned device pointer: never dereferenced


def call_fwd(L, shape, p=P, arg=P, ws=P, ws_bytes=0):
    """shape = (rows, cols, e, D, k, chunk).  ws_bytes defaults to 0: a call that passes every
    other check stops at the workspace check, before any launch."""
    return L.maxk_spgemm_max_forward(p, p, p, p, p, arg, *shape, ws, ws_bytes, None)


def call_bwd(L, shape, p=P, ws=P, ws_bytes=0):
    """shape = (rows, cols, e, D, k)."""
    return L.maxk_spgemm_max_backward(p, p, p, p, p, p, p, p, *shape, ws, ws_bytes, None)


def test_host_side_validation():
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    fsize, bsize = L.maxk_spgemm_max_forward_workspace_size, L.maxk_spgemm_max_backward_workspace_size
    for call, size, tail in ((call_fwd, fsize, (0,)), (call_bwd, bsize, ())):
        ok = (10, 10, 5, 64, 8) + tail
        for i, word in ((0, b"num_rows"), (1, b"num_cols"), (2, b"num_e")):  # negative sizes
            shape = list(ok)
            shape[i] = -5
            assert call(L, tuple(shape)) == -1, shape
            assert word in L.maxk_last_error()
            assert size(*shape) == 0
        for D, k, word in ((0, 1, b"dim_origin"), (257, 8, b"dim_origin"), (64, 0, b"dim_k"),
                           (64, 65, b"dim_k"), (-1, -1, b"dim_origin")):  # k / D range
            assert call(L, (10, 10, 5, D, k) + tail) == -1, (D, k)
            assert word in L.maxk_last_error()
            assert size(10, 10, 5, D, k, *tail) == 0
        assert call(L, ok, p=None) == -1  # null pointers
        assert b"NULL" in L.maxk_last_error()
        for D, k in ((64, 3), (256, 96), (9, 7), (256, 256), (1, 1)):  # accepted up to the workspace
            shape = (10, 10, 5, D, k) + tail
            n = size(*shape)
            assert n > 0 and n % 256 == 0
            for short in (0, n - 1):
                assert call(L, shape, ws_bytes=short) == -1
                assert b"workspace too small" in L.maxk_last_error()
            assert call(L, shape, ws=None, ws_bytes=n) == -1
            assert b"workspace too small" in L.maxk_last_error()
        assert call(L, ok, ws=ctypes.c_void_p(4096 + 16), ws_bytes=1 << 42) == -1
        assert b"256-B aligned" in L.maxk_last_error()
    # the forward alone: chunk_edges, a null arg is allowed, the packed records' limits
    assert call_fwd(L, (10, 10, 5, 64, 8, -1)) == -1 and b"chunk_edges" in L.maxk_last_error()
    assert fsize(10, 10, 5, 64, 8, -1) == 0
    assert call_fwd(L, (10, 10, 5, 64, 8, 0), arg=None) == -1
    assert b"workspace too small" in L.maxk_last_error()  # not the null check
    assert call_fwd(L, (10, 0, 5, 64, 8, 0)) == -1 and b"edges present" in L.maxk_last_error()
    assert call_fwd(L, (10, 1 << 24, 5, 64, 8, 0), ws_bytes=1 << 42) == -1
    assert b"2^24 columns" in L.maxk_last_error()
    assert call_fwd(L, (10, 1 << 23, 5, 256, 128, 0), ws_bytes=1 << 42) == -1
    assert b"4 GiB of records" in L.maxk_last_error()
    # nothing to do: no rows (forward), no columns (backward), whatever the pointers
    assert call_fwd(L, (0, 0, 0, 64, 8, 0), p=None, arg=None, ws=None) == 0
    assert L.maxk_last_error() == b""
    assert call_bwd(L, (0, 0, 0, 64, 8), p=None, ws=None) == 0


@pytest.mark.parametrize("chunk", [0, 64])
def test_workspace_query_monotone_in_edges(chunk):
    """More edges never need less workspace, in the forward and in the backward."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    es = sorted(set([0, 1, 63, 64, 65, 255, 256, 257, 5000]
                    + list(range(65536 * 256 - 1000, 65536 * 256 + 1000, 97))
                    + list(range(65536 * 64 - 3000, 65536 * 64 + 1000, 97))
                    + [int(x) for x in np.geomspace(1e4, 2 ** 31 - 2, 300)]))
    for D, k in ((256, 16), (64, 3)):
        f = [L.maxk_spgemm_max_forward_workspace_size(1000, 1000, e, D, k, chunk) for e in es]
        b = [L.maxk_spgemm_max_backward_workspace_size(1000, 1000, e, D, k) for e in es]
        for sizes in (f, b):
            assert all(s > 0 and s % 256 == 0 for s in sizes)
            assert all(x <= y for x, y in zip(sizes, sizes[1:]))
        assert all(s >= 4 * e for s, e in zip(b, es))  # the row of every CSC slot


# ------------------------------------------------------------------------------- the layers
MEAN_KEYS = ["fc_neigh.weight", "fc_self.weight", "fc_self.bias"]


def test_layer_arguments():
    import maxk_layers as ML
    for bad in ("lstm", "gcn", "max", ""):
        with pytest.raises(ValueError, match="Invalid aggregator_type. Must be one of"):
            ML.MaxKSAGEConv(12, 5, aggregator_type=bad)
    torch.manual_seed(3)
    plain = ML.MaxKSAGEConv(12, 5)
    torch.manual_seed(3)
    mean = ML.MaxKSAGEConv(12, 5, aggregator_type="mean")
    assert list(plain.state_dict()) == list(mean.state_dict()) == MEAN_KEYS
    assert not hasattr(mean, "fc_pool") and mean.aggregator_type == "mean"
    for a, b in zip(plain.state_dict().values(), mean.state_dict().values()):
        assert torch.equal(a, b)
    torch.manual_seed(3)
    pool = ML.MaxKSAGEConv(12, 5, aggregator_type="pool", pool_k=4)
    assert list(pool.state_dict()) == MEAN_KEYS + ["fc_pool.weight", "fc_pool.bias"]
    assert tuple(pool.fc_pool.weight.shape) == (12, 12) and pool.pool_k == 4
    for n in MEAN_KEYS:  # the shared parameters draw the same numbers as the mean layer's
        assert torch.equal(pool.state_dict()[n], mean.state_dict()[n])
    # Xavier with the ReLU gain: |w| <= sqrt(2) * sqrt(6 / (12 + 12))
    lim = 2 ** 0.5 * (6 / 24) ** 0.5
    assert pool.fc_pool.weight.abs().max() <= lim and pool.fc_pool.weight.abs().max() > 0.5 * lim
    assert ML.MaxKGINConv().aggregator_type == "sum"
    assert ML.MaxKGINConv(aggregator_type="max").aggregator_type == "max"
    with pytest.raises(ValueError, match="reference_compat"):
        ML.MaxKGINConv(aggregator_type="max", reference_compat=True)
    with pytest.raises(KeyError):
        ML.MaxKGINConv(aggregator_type="mean")
    assert list(ML.MaxKGINConv(aggregator_type="max").state_dict()) == \
        list(ML.MaxKGINConv().state_dict())
