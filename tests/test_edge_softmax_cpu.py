"""CPU: the edge softmax's reference helper, its C ABI surface and host validation.

tests/edge_softmax_ref.py is the yardstick of test_edge_softmax_gpu.py, so it is pinned here
against torch autograd of the PyTorch composition a user would otherwise write on a CSR
(repeat_interleave of the row ids, gathers, scatter_reduce(amax), index_add_) in float64, on the
graph S of tests/numerics.py: the forward and all three gradients.  No kernel is launched."""
import ctypes
import math

import numpy as np
import pytest
import torch

import edge_softmax_ref as ER
import numerics as N

FWD = ("maxk_edge_softmax", "maxk_gat_edge_softmax")
BWD = ("maxk_edge_softmax_backward", "maxk_gat_edge_softmax_backward")
SYMBOLS = FWD + BWD + tuple(s + "_workspace_size" for s in FWD + BWD)


def graph_s():
    from test_parity_gpu import rand_graph
    return N.named_graph("S", rand_graph)


# ------------------------------------------------------------------------------- the yardstick
def composition(rp, col, s_dst, s_src, slope, gw):
    """(w, grad_logits, grad_s_dst, grad_s_src) by torch autograd, float64."""
    R = rp.size - 1
    rows = torch.repeat_interleave(torch.arange(R), torch.from_numpy(np.diff(rp).astype(np.int64)))
    c = torch.from_numpy(col.astype(np.int64))
    sd = torch.from_numpy(s_dst.astype(np.float64)).requires_grad_(True)
    ss = torch.from_numpy(s_src.astype(np.float64)).requires_grad_(True)
    l = torch.nn.functional.leaky_relu(sd[rows] + ss[c], slope)
    l.retain_grad()
    m = torch.zeros(R, dtype=torch.float64).scatter_reduce(0, rows, l.detach(), "amax",
                                                           include_self=False)
    p = torch.exp(l - m[rows])
    s = torch.zeros(R, dtype=torch.float64).index_add_(0, rows, p)
    w = p / s[rows]
    w.backward(torch.from_numpy(gw.astype(np.float64)))
    return w.detach().numpy(), l.grad.numpy(), sd.grad.numpy(), ss.grad.numpy()


def rel(a, b):
    d = np.abs(a - b) / np.maximum(np.abs(b), 1e-30)
    return float(np.where(a == b, 0.0, d).max())


@pytest.mark.parametrize("slope", [0.2, 0.0, 1.0])
def test_reference_agrees_with_autograd(slope):
    g = graph_s()
    rng = np.random.default_rng(31)
    s_dst = rng.standard_normal(g.R).astype(np.float32)
    s_src = rng.standard_normal(g.C).astype(np.float32)
    gw = rng.standard_normal(g.col.size).astype(np.float32)
    f = ER.gat_forward(g.rp, g.col, s_dst, s_src, slope)
    b = ER.backward(g.rp, g.col, f, gw, slope, g.C)
    w, gl, gd, gs = composition(g.rp, g.col, s_dst, s_src, slope, gw)
    r = dict(w=rel(f.w, w), gl=np.abs(b.gl - gl).max(), g_dst=np.abs(b.g_dst - gd).max(),
             g_src=np.abs(b.g_src - gs).max())
    print(f"\nedge_softmax_ref vs autograd, slope {slope}: {r}")
    # gradients cancel within a row (their sum is 0): compare against the row's scale
    scale = np.abs(gw).max()
    assert r["w"] <= 1e-12
    assert np.abs(b.gl - gl).max() <= 1e-13 * scale  # l.grad: the gradient of the logits
    assert np.abs(b.g_dst - gd).max() <= 1e-12 * scale
    assert np.abs(b.g_src - gs).max() <= 1e-12 * scale
    # the plain form is the same softmax over the logits, its gradient the one of the logits
    fp = ER.forward(g.rp, f.l)
    bp = ER.backward(g.rp, g.col, fp, gw)
    assert np.array_equal(fp.w, f.w)
    assert np.array_equal(bp.gl, b.gl)
    # structure: rows sum to 1, a row of one edge is exactly (1, 0), elements without addends
    # are exactly 0 with bound 0, bounds are positive elsewhere
    deg = np.diff(g.rp)
    sums = np.add.reduceat(f.w, g.rp[:-1][deg > 0].astype(np.int64))
    assert np.abs(sums - 1).max() <= 1e-13
    one = ER.gat_forward(np.array([0, 1, 1, 2], np.int32), np.array([2, 0], np.int32),
                         s_dst[:3], s_src[:3], slope)
    assert (one.w == 1).all()
    assert (ER.backward(np.array([0, 1, 1, 2]), np.array([2, 0]), one, gw[:2], slope, 3).gl
            == 0).all()
    assert (deg == 0).any() and (b.g_dst[deg == 0] == 0).all()
    assert (b.g_dst_bound[deg == 0] == 0).all()
    if slope > 0:  # at slope 0 a row of non-positive z has only exact zeros as terms
        assert (b.g_dst_bound[deg > 0] > 0).all()
    assert b.g_src[g.unread] == 0 and b.g_src_bound[g.unread] == 0
    assert (f.bound > 0).all() and (b.gl_bound > 0).all()


def test_reference_non_finite_rows():
    """A NaN or +Inf logit makes its row NaN, a -Inf logit is exactly 0 unless the whole row is
    -Inf, and no other row changes."""
    rp = np.array([0, 3, 6, 8, 8, 11], np.int32)
    l = np.array([0.5, np.nan, 1.0, 2.0, np.inf, -1.0, -np.inf, -np.inf, 0.25, -np.inf, 3.0])
    f = ER.forward(rp, l)
    assert np.isnan(f.w[:8]).all()
    assert f.w[9] == 0 and np.isfinite(f.w[8:]).all() and abs(f.w[8:].sum() - 1) < 1e-15


# ------------------------------------------------------------------------------- the C ABI
def test_symbols_declared_exported_and_bound():
    import os

    from conftest import PKG
    from maxk_cuda_kernels import _capi
    from test_boundary_cpu import declared_symbols
    syms = declared_symbols()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libmaxk_hip.so"))
    for s in SYMBOLS:
        assert s in syms and hasattr(lib, s) and s in _capi.SIGNATURES, s
    import maxk_cuda_kernels as mk
    for name in ("edge_softmax", "edge_softmax_backward", "gat_edge_softmax",
                 "gat_edge_softmax_backward"):
        assert callable(getattr(mk, name))
    assert mk.version() == 100  # an addition: the ABI version stays


def test_binding_refuses_cpu_tensors():
    """No fallback: a CPU tensor is an error, in the binding and through the layer wrappers."""
    import maxk_cuda_kernels as mk
    import maxk_layers as ML
    rp = torch.tensor([0, 2, 3], dtype=torch.int32)
    col = torch.tensor([0, 1, 1], dtype=torch.int32)
    e, v = torch.zeros(3), torch.zeros(2)
    for call in (lambda: mk.edge_softmax(rp, e),
                 lambda: mk.edge_softmax_backward(rp, e, e),
                 lambda: mk.gat_edge_softmax(rp, col, v, v),
                 lambda: mk.gat_edge_softmax_backward(rp, col, v, v, e, e),
                 lambda: ML.EdgeSoftmax.apply(rp, e),
                 lambda: ML.GATEdgeSoftmax.apply(rp, col, v, v, 0.2)):
        with pytest.raises(RuntimeError, match="must be CUDA tensor"):
            call()


P = ctypes.c_void_p(4096)  # a fake non-null, 256-B aligned device pointer: never dereferenced


def call(L, name, shape, slope=0.2, p=P, ws=P, ws_bytes=1 << 40):
    """The entry point `name` with every pointer p: rejected on the host, or not called with a
    launchable shape."""
    if name == "maxk_edge_softmax":
        return L.maxk_edge_softmax(p, p, p, *shape, ws, ws_bytes, None)
    if name == "maxk_edge_softmax_backward":
        return L.maxk_edge_softmax_backward(p, p, p, p, *shape, ws, ws_bytes, None)
    if name == "maxk_gat_edge_softmax":
        return L.maxk_gat_edge_softmax(p, p, p, p, slope, p, *shape, ws, ws_bytes, None)
    return L.maxk_gat_edge_softmax_backward(p, p, p, p, p, p, slope, p, p, p, p, *shape, ws,
                                            ws_bytes, None)


@pytest.mark.parametrize("name", FWD + BWD)
def test_host_side_validation(name):
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    #                 rows cols  e  chunk
    for shape in ((-1, 10, 5, 0), (10, -1, 5, 0), (10, 10, -5, 0), (10, 10, 5, -1)):
        assert call(L, name, shape) == -1, shape  # negative sizes
        assert L.maxk_last_error() != b""
    assert call(L, name, (10, 10, 5, 0), p=None) == -1  # null pointers with edges present
    assert b"NULL" in L.maxk_last_error()
    if "gat" in name:
        for slope in (-0.1, 1.5, math.nan):
            assert call(L, name, (10, 10, 5, 0), slope=slope) == -1, slope
            assert b"negative_slope" in L.maxk_last_error()
            assert call(L, name, (10, 10, 0, 0), slope=slope) == -1, slope  # even without edges


@pytest.mark.parametrize("name", FWD)
def test_no_edges_forward_succeeds(name):
    """num_e == 0 launches nothing and succeeds, whatever the pointers."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    assert call(L, name, (10, 10, 0, 0), p=None, ws=None, ws_bytes=0) == 0
    assert L.maxk_last_error() == b""
    assert call(L, name, (0, 0, 0, 64), p=None, ws=None, ws_bytes=0) == 0


SHAPES = [(600, 600, 7000, 0), (600, 600, 7000, 64), (150, 700, 6000, 0), (1, 1, 1, 0),
          (232965, 232965, 114615892, 0), (2449029, 2449029, 123718280, 0)]


@pytest.mark.parametrize("name", FWD + BWD)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_workspace_query_and_short_workspace(name, shape):
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    size = getattr(L, name + "_workspace_size")
    n = size(*shape)
    assert n > 0 and n % 256 == 0  # every call keeps per-item partials: never empty
    if name == "maxk_gat_edge_softmax_backward":
        assert n >= 4 * shape[2]  # gz [num_e]
    # one byte short: rejected on the host, before anything could be launched (the device
    # pointers are fake: a launch would not return -1 with this message)
    assert call(L, name, shape, ws_bytes=n - 1) == -1
    assert b"workspace too small" in L.maxk_last_error()
    assert call(L, name, shape, ws=None, ws_bytes=n) == -1
    assert b"workspace too small" in L.maxk_last_error()
    assert call(L, name, shape, ws=ctypes.c_void_p(4096 + 16), ws_bytes=n) == -1
    assert b"256-B aligned" in L.maxk_last_error()
    assert size(-1, 10, 5, 0) == 0 and size(10, 10, -5, 0) == 0 and size(10, 10, 5, -1) == 0


@pytest.mark.parametrize("name", FWD + BWD)
@pytest.mark.parametrize("chunk", [0, 64, 1000])
def test_workspace_query_monotone_in_edges(name, chunk):
    """More edges never need less workspace -- across the auto rule's changes of item size too,
    where one more token can mean fewer, longer items."""
    from maxk_cuda_kernels import _capi
    L = _capi.load()
    size = getattr(L, name + "_workspace_size")
    rows = 1000
    # dense steps around the auto rule's thresholds (65536 items of 256 / 2048 tokens on a
    # 256-CU device), coarse steps elsewhere
    es = sorted(set([0, 1, 63, 64, 65, 255, 256, 257, 5000]
                    + list(range(65536 * 256 - 3000, 65536 * 256 + 3000, 97))
                    + list(range(65536 * 2048 - 3000, 65536 * 2048 + 3000, 97))
                    + [int(x) for x in np.geomspace(1e4, 2 ** 31 - 1, 400)]))
    sizes = [size(rows, rows, e, chunk) for e in es]
    assert all(s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
