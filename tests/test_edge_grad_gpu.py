"""GPU: the gradient of the aggregation with respect to the edge weights.

maxk_edge_weight_grad (edge_grad.hip) through the binding (mk.edge_weight_grad), the autograd
surface (graph_values.grad, both call shapes) and the layer helper (CSRGraph.aggregate), against
tests/edge_grad_ref.py: float64 dot products in numpy, pinned to torch autograd by
test_edge_grad_cpu.py.  The bound is numerics' own, (n + 8) * 2^-24 * sum|terms| with the
2^-149 floor for subnormal inputs, n the number of the destination's selectors below D; an edge
with n = 0 is exactly 0.  Shapes are the module graphs of tests/numerics.py (hub rows of 590 and
390 edges, empty rows, average degree >= 128, a rectangular shape, an unread column), each at
chunk 0 and at 64 tokens, the smallest item, where every hub row is cut over many items.
"""
import functools

import numpy as np
import pytest
import torch

import edge_grad_ref as R
import memguard as M
import numerics as N
import oracle as O
from test_numerics_gpu import dgraph, graph
from test_parity_gpu import T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CHUNKS = (0, 64)
#        (k, D)       why
SHAPES = [(3, 64),     # k % 4 != 0
          (8, 256), (16, 256), (32, 256),  # the common widths
          (24, 256),   # not a power of two
          (96, 256), (256, 256),  # more than one pass per lane
          (7, 9),      # odd D
          (64, 128)]   # the forward's dense-route shape


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


@pytest.fixture(scope="module")
def F(cuda):
    import maxk_spgemm_function
    assert maxk_spgemm_function.MAXK_KERNELS_AVAILABLE
    return maxk_spgemm_function


# ------------------------------------------------------------------------------- shared data
@functools.lru_cache(maxsize=None)
def case(name, D, k, regime="unit"):
    """Inputs and references of one (graph, shape, regime): computed once, never modified.  In
    the subnormal regime the CBSR values are subnormal-scale and G is unit, so the products do
    not all underflow."""
    g = graph(name)
    rng = np.random.default_rng(D * 1000 + k * 7 + len(regime))
    ci = N.selectors(rng, g.C, D, k)
    cv = N.values(rng, (g.C, k), regime)
    G = N.values(rng, (g.R, D), "unit" if regime == "subnormal" else regime)
    return dict(g=g, ci=ci, cv=cv, G=G, unit=N.floor_unit(regime),
                div=R.edge_grad_ref(g.rp, g.col, cv, ci, G, g.div),
                nodiv=R.edge_grad_ref(g.rp, g.col, cv, ci, G, None))


def run(mk, name, cv, ci, G, div=True, chunk=0, out=None, gt=None, validate=None):
    rp, col, _, dv = dgraph(name) if gt is None else gt
    return mk.edge_weight_grad(rp, col, cv, ci, G, row_div=dv if div else None, chunk=chunk,
                               out=out, validate=validate)


def check(y, er, unit, what):
    """Classes equal, the finite rest within the bound (an edge with n = 0: exactly 0)."""
    assert y.dtype == torch.float32 and tuple(y.shape) == er.ref.shape
    r = N.within(y, er.ref, R.bound(er, unit), what)
    print(f"{what}: err/bound {r:.3f}")
    return r


# ------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("k,D", SHAPES, ids=[f"k{k}-D{D}" for k, D in SHAPES])
@pytest.mark.parametrize("name", ["S", "Dn", "R"])
def test_parity_within_bound(mk, cuda, name, k, D):
    c = case(name, D, k)
    cv, ci, G = T(c["cv"], cuda), T(c["ci"], cuda), T(c["G"], cuda)
    for div in (True, False):
        for chunk in CHUNKS:
            y = run(mk, name, cv, ci, G, div, chunk)
            check(y, c["div" if div else "nodiv"], 0.0,
                  f"{name} k{k} D{D} div={div} chunk {chunk}")


@pytest.mark.parametrize("regime", N.REGIMES)
@pytest.mark.parametrize("k,D", [(16, 256), (24, 256)])
def test_value_regimes(mk, cuda, k, D, regime):
    c = case("S", D, k, regime)
    cv, ci, G = T(c["cv"], cuda), T(c["ci"], cuda), T(c["G"], cuda)
    for chunk in CHUNKS:
        y = run(mk, "S", cv, ci, G, True, chunk)
        check(y, c["div"], c["unit"], f"S k{k} D{D} {regime} chunk {chunk}")
        if regime == "subnormal":
            N.nonzero_where_resolved(y, c["div"].ref, R.bound(c["div"], c["unit"]))


# ------------------------------------------------------------------------------- selectors
def test_skipped_and_repeated_selectors(mk, cuda):
    """D = 100, k = 10: a vertex with two equal selectors (summed; the finite bound), a vertex
    with a selector >= D holding NaN, a vertex whose selectors are all >= D (n = 0: exactly 0,
    NaN values and all) and a NaN in a G column none of its row's destinations selects: the
    result stays finite and within the bound."""
    D, k = 100, 10
    c = case("S", D, k)
    g = c["g"]
    cv, ci, G = c["cv"].copy(), c["ci"].copy(), c["G"].copy()
    deg = np.diff(g.rp)
    hubcols = g.col[g.rp[g.hub]:g.rp[g.hub + 1]]
    a, b, z = (int(v) for v in hubcols[:3])  # read by the hub row (split at chunk 64)
    ci[a, 4] = ci[a, 1]
    ci[b, 2], cv[b, 2] = 200, np.nan
    ci[z], cv[z] = np.arange(150, 150 + k), np.nan
    r = int(np.flatnonzero((deg >= 3) & (deg <= 20))[0])
    sel = ci[g.col[g.rp[r]:g.rp[r + 1]]].ravel()
    free = np.setdiff1d(np.arange(D), sel)
    assert free.size
    G[r, free[0]] = np.nan
    for div in (g.div, None):
        er = R.edge_grad_ref(g.rp, g.col, cv, ci, G, div)
        assert np.isfinite(er.ref).all()
        assert (er.n[g.col == z] == 0).all() and (er.n[g.col == b] == k - 1).all()
        for chunk in CHUNKS:
            # validate=False: the range check of the selectors is what this case goes past
            y = run(mk, "S", T(cv, cuda), T(ci, cuda), T(G, cuda), div is not None, chunk,
                    validate=False)
            assert bool(torch.isfinite(y).all())
            check(y, er, 0.0, f"skipped/repeated div={div is not None} chunk {chunk}")
            assert not y[T(g.col == z, cuda)].any()


def test_inf_nan_classes(mk, cuda):
    """Distinct selectors; a +Inf in cbsr_val, a NaN in grad_out and each of numerics'
    NAN_PATTERNS: the NaN, +inf and -inf masks of the result equal the reference's."""
    D, k = 256, 16
    c = case("S", D, k)
    g = c["g"]
    cv, ci, G = c["cv"].copy(), c["ci"], c["G"].copy()
    hubcols = g.col[g.rp[g.hub]:g.rp[g.hub + 1]]
    verts = [int(v) for v in hubcols[:4]]
    cv[verts[0], 5] = np.inf
    for v, slot, bits in zip(verts[1:], (0, 7, k - 1), N.NAN_PATTERNS):
        N._set_bits(cv, (v, slot), bits)
    deg = np.diff(g.rp)
    r = int(np.flatnonzero((deg >= 5) & (deg <= 30))[0])
    G[r, int(ci[g.col[g.rp[r]], 0])] = np.nan  # selected by the row's first destination
    if g.unread is not None:
        cv[g.unread] = np.nan  # a vertex no edge reads
    er = R.edge_grad_ref(g.rp, g.col, cv, ci, G, g.div)
    ref = R.as_f32(er.ref)
    assert np.isnan(ref).any() and np.isinf(ref).any() and np.isfinite(ref).mean() > 0.9
    for chunk in CHUNKS:
        y = run(mk, "S", T(cv, cuda), T(ci, cuda), T(G, cuda), True, chunk)
        N.same_class(y, ref)
        check(y, er, 0.0, f"inf/nan chunk {chunk}")


# ------------------------------------------------------------------------------- bitwise
@pytest.mark.parametrize("name,k,D", [("S", 16, 256), ("Dn", 96, 256), ("R", 3, 64)])
def test_bitwise_repeatable_and_scale_equivariant(mk, cuda, name, k, D):
    c = case(name, D, k)
    cv, ci, G = T(c["cv"], cuda), T(c["ci"], cuda), T(c["G"], cuda)
    E = c["g"].col.size
    for chunk in CHUNKS:
        a = torch.full((E,), float("nan"), device=cuda)
        b = torch.full((E,), 1e30, device=cuda)
        run(mk, name, cv, ci, G, True, chunk, out=a)
        run(mk, name, cv, ci, G, True, chunk, out=b)
        assert M.same_bytes(a, b)
        s = run(mk, name, cv, ci, G * 128.0, True, chunk)
        assert M.same_bytes(s, a * 128.0)
        s = run(mk, name, cv * 0.25, ci, G, True, chunk)
        assert M.same_bytes(s, a * 0.25)
    # the item size changes which wave walks an edge, not its sum
    assert M.same_bytes(run(mk, name, cv, ci, G, True, 0), run(mk, name, cv, ci, G, True, 64))


# ------------------------------------------------------------------------------- memory
@pytest.fixture(scope="module")
def arena(cuda):
    return M.Arena(8 << 20, cuda)  # graph S: out 32 KB, records 600 x 128 B, plus the guards


@pytest.mark.parametrize("k,D", [(16, 256), (3, 64)])
def test_memory_contract(mk, arena, cuda, k, D):
    """Output and workspace from the poisoned, guarded arena (the workspace is exactly the
    queried size): the output is fully written and the same bytes in every fill regime, the
    guards are untouched, the inputs unchanged."""
    c, p = case("S", D, k), case("S", D, k, "small")
    g = c["g"]

    def factory(primer):
        s = p if primer else c
        gt = tuple(T(a, DEV) for a in (g.rp, g.col, g.ev, g.div))
        return (gt, T(s["cv"], DEV), T(s["ci"], DEV), T(s["G"], DEV))

    for chunk in CHUNKS:
        def op(gt, cv, ci, G):
            y = run(mk, "S", cv, ci, G, True, chunk, gt=gt)
            assert arena.owns(y)
            return (y,)
        res = M.run_regimes(op, factory, arena)
        assert len(arena.allocs) == 2  # the output and the workspace
        n_ws = mk._lib().maxk_edge_weight_grad_workspace_size(g.R, g.C, g.col.size, D, k, chunk)
        assert sorted(a.nbytes for a in arena.allocs) == sorted((g.col.size * 4, n_ws))
        for regime, r in res.items():
            check(r[0], c["div"], 0.0, f"memguard k{k} D{D} chunk {chunk} {regime}")
        for regime in ("stale", "ones"):
            assert M.same_bytes(res["zero"][0], res[regime][0]), regime


# ------------------------------------------------------------------------------- streams
def test_runs_on_current_stream(mk, cuda):
    c = case("S", 256, 16)
    cv, ci, G = T(c["cv"], cuda), T(c["ci"], cuda), T(c["G"], cuda)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        y = run(mk, "S", cv, ci, G)
    s.synchronize()
    check(y, c["div"], 0.0, "side stream")


def graph_topology(raw_graph):
    """(number of nodes, [(from, to), ...]) of a captured hipGraph_t, read with
    hipGraphGetNodes / hipGraphGetEdges of the HIP runtime the process has loaded."""
    import ctypes
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    gp = ctypes.c_void_p(raw_graph)
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(gp, None, ctypes.byref(n)) == 0
    ne = ctypes.c_size_t(0)
    assert hip.hipGraphGetEdges(gp, None, None, ctypes.byref(ne)) == 0
    src = (ctypes.c_void_p * max(ne.value, 1))()
    dst = (ctypes.c_void_p * max(ne.value, 1))()
    assert hip.hipGraphGetEdges(gp, src, dst, ctypes.byref(ne)) == 0
    return n.value, [(src[i], dst[i]) for i in range(ne.value)]


def test_hipgraph_capture_single_chain(mk, cuda):
    """One capture of the call into a preallocated out, replayed twice with grad_out changed in
    place between the replays; the captured graph is a single chain (the pack, then the walk:
    no node has two successors or two predecessors)."""
    c, c2 = case("S", 256, 16), case("S", 256, 16, "small")
    g = c["g"]
    cv, ci, G = T(c["cv"], cuda), T(c["ci"], cuda), T(c["G"], cuda)
    out = torch.empty(g.col.size, device=cuda)
    run(mk, "S", cv, ci, G, out=out)  # graph check and allocator warm-up outside the capture
    torch.cuda.synchronize()
    hg = torch.cuda.CUDAGraph(keep_graph=True)  # the hipGraph_t stays readable after the capture
    with torch.cuda.graph(hg):
        run(mk, "S", cv, ci, G, out=out, validate=False)
    n_nodes, edges = graph_topology(hg.raw_cuda_graph())
    print(f"captured graph: {n_nodes} nodes, {len(edges)} edges")
    assert n_nodes == 2 and len(edges) == 1, (n_nodes, edges)  # the pack, then the walk
    succ, pred = [a for a, _ in edges], [b for _, b in edges]
    assert len(set(succ)) == len(succ) and len(set(pred)) == len(pred)
    hg.instantiate()
    out.fill_(float("nan"))
    hg.replay()
    torch.cuda.synchronize()
    check(out, c["div"], 0.0, "replay 1")
    G.copy_(T(c2["G"], cuda))
    out.fill_(float("nan"))
    hg.replay()
    torch.cuda.synchronize()
    er2 = R.edge_grad_ref(g.rp, g.col, c["cv"], c["ci"], c2["G"], g.div)
    check(out, er2, 0.0, "replay 2")


# ------------------------------------------------------------------------------- autograd
def v_call(F, via, col, w, x_or_tv, ti, k, rp, dv, D):
    if via == "v1":
        return F.maxk_spgemm(col, w, x_or_tv, k, graph_indptr=rp, in_degrees=dv)
    return F.maxk_spgemm(col, w, x_or_tv, ti, None, 0, rp, dv, dim_origin=D)


@pytest.mark.parametrize("via", ["v1", "v4"])
def test_autograd_weight_grad(F, mk, cuda, monkeypatch, via):
    """graph_values.grad within the bound of the reference, in the weights' dtype; with the
    backward forced to csc the feature gradient is bitwise the one without requires_grad on the
    weights."""
    monkeypatch.setenv("MAXK_BWD_MODE", "csc")
    D, k = 256, 16
    c = case("S", D, k)
    g = c["g"]
    rp, col, ev, dv = dgraph("S")
    rng = np.random.default_rng(99)
    x = rng.standard_normal((g.C, D)).astype(np.float32)
    cvx, cix = O.topk(x, k)
    cvn, cin = (cvx, cix) if via == "v1" else (c["cv"], c["ci"])
    Gt = T(c["G"], cuda)
    er = R.edge_grad_ref(g.rp, g.col, cvn, cin, c["G"], g.div)
    grads = {}
    for wgrad, dtype in ((False, torch.float32), (True, torch.float32), (True, torch.float64)):
        w = ev.to(dtype).clone().requires_grad_(wgrad)
        feat = (T(x, cuda) if via == "v1" else T(cvn, cuda)).requires_grad_(True)
        y = v_call(F, via, col, w, feat, T(cin, cuda) if via == "v4" else None, k, rp, dv, D)
        y.backward(Gt)
        grads[(wgrad, dtype)] = feat.grad
        if wgrad:
            assert w.grad is not None and w.grad.dtype == dtype and w.grad.shape == w.shape
            check(w.grad.float(), er, 0.0, f"{via} weight grad {dtype}")
        else:
            assert w.grad is None
    base = grads[(False, torch.float32)]
    assert M.same_bytes(base, grads[(True, torch.float32)])
    assert M.same_bytes(base, grads[(True, torch.float64)])


@pytest.mark.parametrize("via", ["v1", "v4"])
def test_autograd_no_weight_grad_no_call(F, mk, cuda, monkeypatch, via):
    """Weights that do not require grad: the edge-gradient kernel is never called and nothing
    extra is saved."""
    def boom(*a, **kw):
        raise AssertionError("edge_weight_grad called without differentiable weights")
    monkeypatch.setattr(mk, "edge_weight_grad", boom)
    D, k = 256, 16
    c = case("S", D, k)
    rp, col, ev, dv = dgraph("S")
    feat = (torch.randn(c["g"].C, D, device=cuda) if via == "v1" else T(c["cv"], cuda))
    feat.requires_grad_(True)
    y = v_call(F, via, col, ev, feat, T(c["ci"], cuda), k, rp, dv, D)
    assert len(y.grad_fn.saved_tensors) == 6
    y.backward(T(c["G"], cuda))
    assert feat.grad is not None
    # and with them: called once
    monkeypatch.undo()
    calls = []
    real = mk.edge_weight_grad
    monkeypatch.setattr(mk, "edge_weight_grad", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    w = ev.clone().requires_grad_(True)
    feat.grad = None
    y = v_call(F, via, col, w, feat, T(c["ci"], cuda), k, rp, dv, D)
    assert len(y.grad_fn.saved_tensors) == 8
    y.backward(T(c["G"], cuda))
    assert calls == [1] and w.grad is not None


def test_backward_divisor_reference_leaves_weight_grad(F, mk, cuda):
    """v1 with backward_divisor="reference": the feature gradient divides by out_degrees, the
    weight gradient still by the forward's in_degrees (the exact adjoint)."""
    D, k = 256, 16
    c = case("S", D, k)
    g = c["g"]
    rp, col, ev, dv = dgraph("S")
    rng = np.random.default_rng(5)
    x = rng.standard_normal((g.C, D)).astype(np.float32)
    cvx, cix = O.topk(x, k)
    od = T(rng.uniform(1.0, 9.0, g.R).astype(np.float32), cuda)
    w = ev.clone().requires_grad_(True)
    y = F.maxk_spgemm(col, w, T(x, cuda).requires_grad_(True), k, graph_indptr=rp, in_degrees=dv,
                      out_degrees=od, backward_divisor="reference")
    y.backward(T(c["G"], cuda))
    check(w.grad, R.edge_grad_ref(g.rp, g.col, cvx, cix, c["G"], g.div), 0.0, "reference divisor")


def test_weights_changed_in_place(F, mk, cuda, monkeypatch):
    """Two SGD-style steps on a weight Parameter on graph Dn, mode auto, where "auto" would
    otherwise take a plan that embeds the weights: the second step's output, feature gradient
    and weight gradient follow the updated weights, and no pull, dense or hybrid plan was built
    for the graph."""
    monkeypatch.delenv("MAXK_BWD_MODE", raising=False)
    D, k = 256, 16
    c = case("Dn", D, k)
    g = c["g"]
    rp, col, ev, dv = (t.clone() for t in dgraph("Dn"))
    assert mk._bwd_mode("auto", k, g.col.size, g.C, g.R, D, (rp, col)) in ("pull", "dense",
                                                                          "hybrid")
    w = torch.nn.Parameter(ev.clone())
    Gt = T(c["G"], cuda)
    for step in range(2):
        tv = T(c["cv"], cuda).requires_grad_(True)
        w.grad = None
        y = F.maxk_spgemm(col, w, tv, T(c["ci"], cuda), None, 0, rp, dv, dim_origin=D)
        y.backward(Gt)
        if step == 0:
            with torch.no_grad():
                w.add_(w.grad, alpha=-0.05)  # in place: the tensor object stays, its version moves
    g2 = g._replace(ev=w.detach().cpu().numpy())
    N.within(y, N.fwd_ref(g2, c["cv"], c["ci"], D), N.bound_fwd(g2, c["cv"], c["ci"], D),
             "second step output")
    N.within(tv.grad, N.bwd_ref(g2, c["G"], c["ci"]), N.bound_bwd(g2, c["G"], c["ci"]),
             "second step feature grad")
    check(w.grad, c["div"], 0.0, "second step weight grad")
    for cache in (mk._PULL_CACHE, mk._DENSE_CACHE, mk._HYBRID_CACHE):
        assert not any(id(col) in key[:3] or id(rp) in key[:3] for key in cache._entries)


def test_layer_aggregate_weight_grad(cuda):
    """CSRGraph.aggregate(tv, ti, D, values=w, row_div=deg) with w.requires_grad."""
    from maxk_layers import CSRGraph
    D, k = 256, 16
    c = case("S", D, k)
    g = c["g"]
    rp, col, ev, dv = dgraph("S")
    assert g.R == g.C  # CSRGraph is square
    graph_ = CSRGraph(rp, col)
    w = ev.clone().requires_grad_(True)
    y = graph_.aggregate(T(c["cv"], cuda), T(c["ci"], cuda), D, values=w, row_div=dv)
    y.backward(T(c["G"], cuda))
    assert w.grad is not None
    check(w.grad, c["div"], 0.0, "CSRGraph.aggregate")


# ------------------------------------------------------------------------------- wide tables
def test_tables_past_2_24_columns(mk, cuda):
    """num_cols = 2^24 + 4099: record offsets pass the 24-bit multiply, so the walk takes its
    64-bit-address form.  A 1,500-row graph whose edges reach every part of the range, the last
    columns included, with a hub row split over items at chunk 64."""
    k, D = 8, 256
    rng = np.random.default_rng(2424)
    NC = (1 << 24) + 4099
    V = 1500
    deg = rng.integers(0, 40, V)
    deg[5] = 900
    rows = [np.sort(rng.choice(NC, int(d), replace=False)) for d in deg]
    rows[9] = np.sort(np.concatenate([rows[9], NC - 1 - np.arange(3)]))
    rp = np.zeros(V + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    rp = rp.astype(np.int32)
    col = np.concatenate(rows).astype(np.int32)
    assert int(col.max()) == NC - 1
    uc = np.unique(col)
    colc = np.searchsorted(uc, col).astype(np.int32)
    cvc = rng.standard_normal((uc.size, k)).astype(np.float32)
    cic = np.stack([rng.choice(D, k, replace=False) for _ in range(uc.size)]).astype(np.uint8)
    div = np.maximum(np.diff(rp), 1).astype(np.float32)
    G = rng.standard_normal((V, D)).astype(np.float32)
    ucg = torch.from_numpy(uc.astype(np.int64)).to(cuda)
    cv = torch.zeros(NC, k, device=cuda)
    cv[ucg] = T(cvc, cuda)
    ci = torch.arange(k, device=cuda, dtype=torch.uint8).repeat(NC, 1)
    ci[ucg] = T(cic, cuda)
    er = R.edge_grad_ref(rp, colc, cvc, cic, G, div)
    for chunk in CHUNKS:
        y = mk.edge_weight_grad(T(rp, cuda), T(col, cuda), cv, ci, T(G, cuda),
                                row_div=T(div, cuda), chunk=chunk)
        check(y, er, 0.0, f"wide chunk {chunk}")
    del cv, ci
    torch.cuda.empty_cache()
