"""GPU: the multi-head aggregation -- maxk_spgemm_forward_heads (spgemm_fwd_heads.hip, on the walk
of heads_walk.h) and maxk_edge_weight_grad_heads (edge_grad.hip) through the binding, the autograd
surface (maxk_spgemm_heads) and the layer (MaxKMultiHeadGATConv), against tests/heads_ref.py: the
oracle's forward and numpy float64 dot products per head, pinned to torch autograd by
test_heads_cpu.py.  Bounds are numerics' own, (n + 8) * 2^-24 * sum|terms| with the 2^-149 floor
for subnormal inputs.  Shapes are the module graphs of tests/numerics.py (S: hub rows of 590 and
200 edges, empty rows; Dn: average degree >= 128, a hub row of 390; R: rectangular; an unread
column in each), each at chunk 0 and at 64 tokens, the smallest item, where every hub row is cut
over many items and merged from per-item slabs.

Kernel instantiations and the tests that launch them (U = 8 throughout):

  spgemm_fwd_heads_kernel<8>   k = 3, 7, 8   test_parity_within_bound[*-k3-D64 / k7-D9 / k8-D256]
      H = 1, 2 (EP = 8, 4), H = 3 (EP = 2, two idle groups), H = 8 (EP = 1)
  spgemm_fwd_heads_kernel<16>  k = 16        test_parity_within_bound[*-k16-D256], regimes, memory
      H = 3 (EP = 1, one idle group), H = 8 (H > G: two passes of four heads)
  spgemm_fwd_heads_kernel<32>  k = 24, 32    test_parity_within_bound[*-k24-D256 / k32-D256]
      H = 3 (two passes of two and one head), H = 8 (four passes)
  spgemm_fwd_heads_kernel<64>  k = 96        test_parity_within_bound[*-k96-D256]
      one head per pass, two slots per lane
  edge_grad_heads_kernel<8 / 16 / 32 / 64>   the same cases; <64> at k = 96 takes the form that
      passes over l per head, the others the form that loads the record once for all heads
  scalar row stores / row staging (D % 4 != 0)   k7-D9
"""
import functools

import numpy as np
import pytest
import torch

import edge_grad_ref as R
import heads_ref as HR
import memguard as M
import numerics as N
from test_edge_grad_gpu import graph_topology
from test_numerics_gpu import dgraph, graph
from test_parity_gpu import T, rand_graph

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CHUNKS = (0, 64)
HMAX = 8
HEADS = (1, 2, 3, 8)
#        (k, D)       why
SHAPES = [(3, 64),     # k % 4 != 0
          (8, 256), (16, 256), (32, 256),  # the common widths; H = 8 > G from k = 16 on
          (24, 256),   # not a power of two
          (96, 256),   # several slots per lane
          (7, 9)]      # odd D


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    yield maxk_cuda_kernels
    for f in (fwd_expected, grad_expected, case):  # [8, R, D] references: not kept past the module
        f.cache_clear()


@pytest.fixture(scope="module")
def F(cuda):
    import maxk_spgemm_function
    assert maxk_spgemm_function.MAXK_KERNELS_AVAILABLE
    return maxk_spgemm_function


# ------------------------------------------------------------------------------- shared data
@functools.lru_cache(maxsize=None)
def case(name, D, k, regime="unit"):
    """Inputs of one (graph, shape, regime) for HMAX heads; fewer heads take the first H.
    Computed once, never modified.  In the subnormal regime the CBSR values are subnormal-scale
    and the weights and G unit, so the products do not all underflow."""
    g = graph(name)
    rng = np.random.default_rng(D * 1000 + k * 7 + len(regime) + 31)
    ci = N.selectors(rng, g.C, D, k)
    cv = N.values(rng, (g.C, k), regime)
    w = rng.uniform(0.5, 1.5, (HMAX, g.col.size)).astype(np.float32)
    G = N.values(rng, (HMAX, g.R, D), "unit" if regime == "subnormal" else regime)
    return dict(g=g, ci=ci, cv=cv, w=w, G=G, unit=N.floor_unit(regime))


@functools.lru_cache(maxsize=None)
def fwd_expected(name, D, k, regime, div):
    """(reference, bound), [HMAX, R, D] each."""
    c = case(name, D, k, regime)
    return (HR.fwd_heads_ref(c["g"], c["w"], c["cv"], c["ci"], D, div),
            HR.bound_fwd_heads(c["g"], c["w"], c["cv"], c["ci"], D, div, c["unit"]))


@functools.lru_cache(maxsize=None)
def grad_expected(name, D, k, regime, div):
    """EdgeRef with [HMAX, E] members; the divided one is the undivided one over row_div, as
    edge_grad_ref forms it."""
    c = case(name, D, k, regime)
    if not div:
        return HR.edge_grad_heads_ref(c["g"], c["cv"], c["ci"], c["G"], False)
    er = grad_expected(name, D, k, regime, False)
    d = c["g"].div.astype(np.float64)[R.edge_rows(c["g"].rp)]
    return R.EdgeRef(er.ref / d, er.n, er.s_abs / d)


def run_fwd(mk, name, w, cv, ci, D, div=True, chunk=0, out=None, gt=None, validate=None):
    rp, col, _, dv = dgraph(name) if gt is None else gt
    return mk.spgemm_forward_heads(rp, col, w, cv, ci, D, row_div=dv if div else None,
                                   chunk=chunk, out=out, validate=validate)


def run_grad(mk, name, cv, ci, G, div=True, chunk=0, out=None, gt=None, validate=None):
    rp, col, _, dv = dgraph(name) if gt is None else gt
    return mk.edge_weight_grad_heads(rp, col, cv, ci, G, row_div=dv if div else None,
                                     chunk=chunk, out=out, validate=validate)


def check_fwd(y, ref, bound, what):
    assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape
    r = N.within(y, ref, bound, what)
    print(f"{what}: err/bound {r:.3f}")
    return r


def check_grad(y, er, unit, what):
    assert y.dtype == torch.float32 and tuple(y.shape) == er.ref.shape
    r = N.within(y, er.ref, R.bound(er, unit), what)
    print(f"{what}: err/bound {r:.3f}")
    return r


def dev_case(c, H, cuda):
    return (T(c["w"][:H], cuda), T(c["cv"], cuda), T(c["ci"], cuda), T(c["G"][:H], cuda))


# ------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("H", HEADS, ids=[f"H{h}" for h in HEADS])
@pytest.mark.parametrize("k,D", SHAPES, ids=[f"k{k}-D{D}" for k, D in SHAPES])
@pytest.mark.parametrize("name", ["S", "Dn", "R"])
def test_parity_within_bound(mk, cuda, name, k, D, H):
    c = case(name, D, k)
    w, cv, ci, G = dev_case(c, H, cuda)
    for div in (True, False):
        yo, by = fwd_expected(name, D, k, "unit", div)
        er = HR.heads_slice(grad_expected(name, D, k, "unit", div), H)
        for chunk in CHUNKS:
            what = f"{name} k{k} D{D} H{H} div={div} chunk {chunk}"
            check_fwd(run_fwd(mk, name, w, cv, ci, D, div, chunk), yo[:H], by[:H], "fwd " + what)
            check_grad(run_grad(mk, name, cv, ci, G, div, chunk), er, 0.0, "grad " + what)


@pytest.mark.parametrize("regime", N.REGIMES)
def test_value_regimes(mk, cuda, regime):
    name, k, D, H = "S", 16, 256, 3
    c = case(name, D, k, regime)
    w, cv, ci, G = dev_case(c, H, cuda)
    yo, by = fwd_expected(name, D, k, regime, True)
    er = HR.heads_slice(grad_expected(name, D, k, regime, True), H)
    for chunk in CHUNKS:
        y = run_fwd(mk, name, w, cv, ci, D, True, chunk)
        check_fwd(y, yo[:H], by[:H], f"fwd {regime} chunk {chunk}")
        e = run_grad(mk, name, cv, ci, G, True, chunk)
        check_grad(e, er, c["unit"], f"grad {regime} chunk {chunk}")
        if regime == "subnormal":
            N.nonzero_where_resolved(y, yo[:H], by[:H])
            N.nonzero_where_resolved(e, er.ref, R.bound(er, c["unit"]))


# ------------------------------------------------------------------------------- selectors
def test_skipped_and_repeated_selectors(mk, cuda):
    """test_edge_grad_gpu's case at H = 2, both kernels.  D = 100, k = 10: a vertex with two
    equal selectors (summed), a vertex with a selector >= D holding NaN, a vertex whose
    selectors are all >= D (it contributes nothing, NaN values and all) and, for the gradient,
    a NaN in a G column none of its row's destinations selects: finite and within the bound."""
    D, k, H = 100, 10, 2
    c = case("S", D, k)
    g = c["g"]
    cv, ci, G = c["cv"].copy(), c["ci"].copy(), c["G"][:H].copy()
    w = c["w"][:H]
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
    G[:, r, free[0]] = np.nan
    for div in (True, False):
        yo = HR.fwd_heads_ref(g, w, cv, ci, D, div)
        by = HR.bound_fwd_heads(g, w, cv, ci, D, div)
        er = HR.edge_grad_heads_ref(g, cv, ci, G, div)
        assert np.isfinite(yo).all() and np.isfinite(er.ref).all()
        assert (er.n[:, g.col == z] == 0).all() and (er.n[:, g.col == b] == k - 1).all()
        for chunk in CHUNKS:
            # validate=False: the range check of the selectors is what this case goes past
            y = run_fwd(mk, "S", T(w, cuda), T(cv, cuda), T(ci, cuda), D, div, chunk,
                        validate=False)
            assert bool(torch.isfinite(y).all())
            check_fwd(y, yo, by, f"fwd skipped/repeated div={div} chunk {chunk}")
            e = run_grad(mk, "S", T(cv, cuda), T(ci, cuda), T(G, cuda), div, chunk,
                         validate=False)
            assert bool(torch.isfinite(e).all())
            check_grad(e, er, 0.0, f"grad skipped/repeated div={div} chunk {chunk}")
            assert not e[:, T(g.col == z, cuda)].any()


def test_forward_inf_nan_per_head(mk, cuda):
    """Inf and NaN in cbsr_val reach every head's slice as they reach the single-head forward:
    the class masks equal the oracle's per head."""
    D, k, H = 256, 16, 3
    c = case("S", D, k)
    g = c["g"]
    cv = c["cv"].copy()
    hubcols = g.col[g.rp[g.hub]:g.rp[g.hub + 1]]
    cv[int(hubcols[0]), 5] = np.inf
    cv[int(hubcols[1]), 0] = -np.inf
    for v, slot, bits in zip(hubcols[2:5], (0, 7, k - 1), N.NAN_PATTERNS):
        N._set_bits(cv, (int(v), slot), bits)
    cv[g.unread] = np.nan  # a vertex no edge reads
    w = c["w"][:H]
    yo = HR.fwd_heads_ref(g, w, cv, c["ci"], D)
    by = HR.bound_fwd_heads(g, w, cv, c["ci"], D)
    assert np.isnan(yo).any() and np.isinf(yo).any() and np.isfinite(yo).mean() > 0.9
    for chunk in CHUNKS:
        y = run_fwd(mk, "S", T(w, cuda), T(cv, cuda), T(c["ci"], cuda), D, True, chunk)
        check_fwd(y, yo, by, f"fwd inf/nan chunk {chunk}")


# ------------------------------------------------------------------------------- bitwise
BITWISE = [("S", 16, 256, 3), ("S", 16, 256, 8), ("S", 8, 256, 3), ("Dn", 96, 256, 2),
           ("R", 3, 64, 3), ("Dn", 32, 256, 8)]


@pytest.mark.parametrize("name,k,D,H", BITWISE,
                         ids=[f"{n}-k{k}-D{D}-H{H}" for n, k, D, H in BITWISE])
def test_bitwise(mk, cuda, name, k, D, H):
    """Two runs into differently prefilled outputs are the same bytes; head h's slice does not
    change when the other heads' weights (forward) or gradients (edge gradient) are replaced by
    other finite random values; every head's edge gradient is the single-head kernel's."""
    c = case(name, D, k)
    g = c["g"]
    w, cv, ci, G = dev_case(c, H, cuda)
    rp, col, _, dv = dgraph(name)
    E = g.col.size
    gen = torch.Generator(device=cuda).manual_seed(5)
    for chunk in CHUNKS:
        a = torch.full((H, g.R, D), float("nan"), device=cuda)
        b = torch.full((H, g.R, D), 1e30, device=cuda)
        run_fwd(mk, name, w, cv, ci, D, True, chunk, out=a)
        run_fwd(mk, name, w, cv, ci, D, True, chunk, out=b)
        assert M.same_bytes(a, b)
        ea = torch.full((H, E), float("nan"), device=cuda)
        eb = torch.full((H, E), 1e30, device=cuda)
        run_grad(mk, name, cv, ci, G, True, chunk, out=ea)
        run_grad(mk, name, cv, ci, G, True, chunk, out=eb)
        assert M.same_bytes(ea, eb)
        for h in sorted({0, H - 1}):
            w2 = torch.rand(H, E, generator=gen, device=cuda) * 3.0 - 1.5
            w2[h] = w[h]
            G2 = torch.randn(H, g.R, D, generator=gen, device=cuda)
            G2[h] = G[h]
            if H > 1:
                assert not torch.equal(w2, w)
            assert M.same_bytes(run_fwd(mk, name, w2, cv, ci, D, True, chunk)[h], a[h]), (h, chunk)
            assert M.same_bytes(run_grad(mk, name, cv, ci, G2, True, chunk)[h], ea[h]), (h, chunk)
        for h in range(H):
            one = mk.edge_weight_grad(rp, col, cv, ci, G[h], row_div=dv, chunk=chunk)
            assert M.same_bytes(one, ea[h]), (h, chunk)


@pytest.mark.parametrize("name,k,D", [("S", 16, 256), ("Dn", 96, 256), ("R", 3, 64), ("S", 7, 9)])
def test_one_head_gradient_is_the_single_head_kernel(mk, cuda, name, k, D):
    c = case(name, D, k)
    _, cv, ci, G = dev_case(c, 1, cuda)
    rp, col, _, dv = dgraph(name)
    for div in (True, False):
        for chunk in CHUNKS:
            one = mk.edge_weight_grad(rp, col, cv, ci, G[0], row_div=dv if div else None,
                                      chunk=chunk)
            assert M.same_bytes(run_grad(mk, name, cv, ci, G, div, chunk)[0], one)


def test_no_edges_forward_writes_zeros(mk, cuda):
    rp = torch.zeros(41, dtype=torch.int32, device=cuda)
    col = torch.zeros(0, dtype=torch.int32, device=cuda)
    cv = torch.randn(40, 8, device=cuda)
    ci = torch.arange(8, dtype=torch.uint8, device=cuda).repeat(40, 1)
    out = torch.full((3, 40, 64), float("nan"), device=cuda)
    mk.spgemm_forward_heads(rp, col, torch.zeros(3, 0, device=cuda), cv, ci, 64, out=out)
    assert not out.any()
    e = mk.edge_weight_grad_heads(rp, col, cv, ci, torch.randn(3, 40, 64, device=cuda))
    assert tuple(e.shape) == (3, 0)


# ------------------------------------------------------------------------------- memory
@pytest.fixture(scope="module")
def arena(cuda):
    return M.Arena(16 << 20, cuda)  # graph S, H = 8: out 4.9 MB, slabs and records < 2 MB


@pytest.mark.parametrize("k,D,H", [(16, 256, 3), (16, 256, 8), (3, 64, 3)])
def test_memory_contract(mk, arena, cuda, k, D, H):
    """Output and workspace from the poisoned, guarded arena (the workspace is exactly the
    queried size), zero-filled, stale and 0xFF-filled (NaN as floats): each output is fully
    written and the same bytes in every fill regime, the guards are untouched, the inputs
    unchanged."""
    c, p = case("S", D, k), case("S", D, k, "small")
    g = c["g"]
    E = g.col.size

    def factory(primer):
        s = p if primer else c
        gt = tuple(T(a, DEV) for a in (g.rp, g.col, g.ev, g.div))
        return (gt,) + dev_case(s, H, DEV)

    yo, by = fwd_expected("S", D, k, "unit", True)
    er = HR.heads_slice(grad_expected("S", D, k, "unit", True), H)
    for chunk in CHUNKS:
        def fwd(gt, w, cv, ci, G):
            y = run_fwd(mk, "S", w, cv, ci, D, True, chunk, gt=gt)
            assert arena.owns(y)
            return (y,)

        def grad(gt, w, cv, ci, G):
            e = run_grad(mk, "S", cv, ci, G, True, chunk, gt=gt)
            assert arena.owns(e)
            return (e,)
        shape = (g.R, g.C, E, D, k, H, chunk)
        for op, out_bytes, size_fn in (
                (fwd, H * g.R * D * 4, mk._lib().maxk_spgemm_forward_heads_workspace_size),
                (grad, H * E * 4, mk._lib().maxk_edge_weight_grad_heads_workspace_size)):
            res = M.run_regimes(op, factory, arena)
            assert len(arena.allocs) == 2  # the output and the workspace
            assert sorted(a.nbytes for a in arena.allocs) == sorted((out_bytes, size_fn(*shape)))
            for regime, r in res.items():
                what = f"memguard {op.__name__} k{k} D{D} H{H} chunk {chunk} {regime}"
                if op is fwd:
                    check_fwd(r[0], yo[:H], by[:H], what)
                else:
                    check_grad(r[0], er, 0.0, what)
            for regime in ("stale", "ones"):
                assert M.same_bytes(res["zero"][0], res[regime][0]), regime


# ------------------------------------------------------------------------------- streams
def test_runs_on_current_stream(mk, cuda):
    name, k, D, H = "S", 16, 256, 3
    c = case(name, D, k)
    w, cv, ci, G = dev_case(c, H, cuda)
    yo, by = fwd_expected(name, D, k, "unit", True)
    er = HR.heads_slice(grad_expected(name, D, k, "unit", True), H)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        y = run_fwd(mk, name, w, cv, ci, D)
        e = run_grad(mk, name, cv, ci, G)
    s.synchronize()
    check_fwd(y, yo[:H], by[:H], "fwd side stream")
    check_grad(e, er, 0.0, "grad side stream")


def test_hipgraph_capture_single_chain(mk, cuda):
    """One capture of both calls into preallocated outputs, replayed twice with the weights and
    grad_out changed in place between the replays.  The captured graph is one linear chain --
    the pack, the walk and H fix-ups of the forward, the pack and the walk of the gradient: no
    node has two successors or two predecessors."""
    name, k, D, H = "S", 16, 256, 3
    c, c2 = case(name, D, k), case(name, D, k, "small")
    g = c["g"]
    w, cv, ci, G = dev_case(c, H, cuda)
    y = torch.empty(H, g.R, D, device=cuda)
    e = torch.empty(H, g.col.size, device=cuda)

    def both(validate=None):
        run_fwd(mk, name, w, cv, ci, D, out=y, validate=validate)
        run_grad(mk, name, cv, ci, G, out=e, validate=validate)
    both()  # graph check and allocator warm-up outside the capture
    torch.cuda.synchronize()
    hg = torch.cuda.CUDAGraph(keep_graph=True)  # the hipGraph_t stays readable after the capture
    with torch.cuda.graph(hg):
        both(validate=False)
    n_nodes, edges = graph_topology(hg.raw_cuda_graph())
    print(f"captured graph: {n_nodes} nodes, {len(edges)} edges")
    assert n_nodes == (2 + H) + 2 and len(edges) == n_nodes - 1, (n_nodes, edges)
    succ, pred = [a for a, _ in edges], [b for _, b in edges]
    assert len(set(succ)) == len(succ) and len(set(pred)) == len(pred)
    hg.instantiate()
    yo, by = fwd_expected(name, D, k, "unit", True)
    er = HR.heads_slice(grad_expected(name, D, k, "unit", True), H)
    y.fill_(float("nan"))
    e.fill_(float("nan"))
    hg.replay()
    torch.cuda.synchronize()
    check_fwd(y, yo[:H], by[:H], "fwd replay 1")
    check_grad(e, er, 0.0, "grad replay 1")
    w2 = np.ascontiguousarray(c["w"][HMAX - H:])  # other weights, the same shape
    w.copy_(T(w2, cuda))
    G.copy_(T(c2["G"][:H], cuda))
    y.fill_(float("nan"))
    e.fill_(float("nan"))
    hg.replay()
    torch.cuda.synchronize()
    check_fwd(y, HR.fwd_heads_ref(g, w2, c["cv"], c["ci"], D),
              HR.bound_fwd_heads(g, w2, c["cv"], c["ci"], D), "fwd replay 2")
    check_grad(e, HR.edge_grad_heads_ref(g, c["cv"], c["ci"], c2["G"][:H]), 0.0, "grad replay 2")


# ------------------------------------------------------------------------------- autograd
def test_autograd_heads(F, mk, cuda):
    """maxk_spgemm_heads at H = 3, (16, 256), graph S: the output, graph_values.grad and
    topk_values.grad (the sum over heads: n = sum_h n_h) within the bounds of heads_ref."""
    name, k, D, H = "S", 16, 256, 3
    c = case(name, D, k)
    g = c["g"]
    rp, col, _, dv = dgraph(name)
    w, cv, ci, G = dev_case(c, H, cuda)
    w.requires_grad_(True)
    cv.requires_grad_(True)
    y = F.maxk_spgemm_heads(rp, col, w, cv, ci, D, dv)
    yo, by = fwd_expected(name, D, k, "unit", True)
    check_fwd(y, yo[:H], by[:H], "autograd output")
    y.backward(G)
    assert w.grad is not None and w.grad.shape == w.shape and w.grad.dtype == torch.float32
    check_grad(w.grad, HR.heads_slice(grad_expected(name, D, k, "unit", True), H), 0.0,
               "autograd graph_values.grad")
    assert cv.grad is not None and cv.grad.shape == cv.shape
    r = N.within(cv.grad, HR.feat_grad_heads_ref(g, c["w"][:H], c["G"][:H], c["ci"]),
                 HR.bound_feat_grad_heads(g, c["w"][:H], c["G"][:H], c["ci"]),
                 "autograd topk_values.grad")
    print(f"autograd topk_values.grad: err/bound {r:.3f}")
    # float64 weights: their gradient comes back in their dtype; no weight gradient asked, none
    w64 = T(c["w"][:H], cuda).double().requires_grad_(True)
    F.maxk_spgemm_heads(rp, col, w64, cv.detach(), ci, D, dv).backward(G)
    assert w64.grad.dtype == torch.float64
    cv2 = cv.detach().clone().requires_grad_(True)
    F.maxk_spgemm_heads(rp, col, w.detach(), cv2, ci, D, dv).backward(G)
    assert M.same_bytes(cv2.grad, cv.grad)


def test_forward_route_rule(F, mk, cuda, monkeypatch):
    """maxk_spgemm_heads takes the multi-head forward on a sparse graph (S: average degree 12)
    and H single-head forwards on a dense one (Dn: 160 >= 128), where the multi-head kernel
    measured no faster (mk.heads_forward_route); the weight gradient is the multi-head kernel
    on both.  Either way the output and the gradients are within the bounds."""
    monkeypatch.delenv("MAXK_HEADS_FWD", raising=False)
    k, D, H = 16, 256, 3
    calls = []
    for fn in ("spgemm_forward_heads", "spgemm_forward", "edge_weight_grad_heads"):
        real = getattr(mk, fn)
        monkeypatch.setattr(
            mk, fn, lambda *a, _r=real, _n=fn, **kw: calls.append(_n) or _r(*a, **kw))
    for name, route in (("S", "heads"), ("Dn", "calls")):
        g = graph(name)
        assert mk.heads_forward_route(g.R, g.col.size) == route
        c = case(name, D, k)
        rp, col, _, dv = dgraph(name)
        w, cv, ci, G = dev_case(c, H, cuda)
        w.requires_grad_(True)
        del calls[:]
        y = F.maxk_spgemm_heads(rp, col, w, cv, ci, D, dv)
        assert calls == (["spgemm_forward_heads"] if route == "heads" else ["spgemm_forward"] * H)
        yo, by = fwd_expected(name, D, k, "unit", True)
        check_fwd(y, yo[:H], by[:H], f"route {route} output")
        y.backward(G)
        assert calls[-1] == "edge_weight_grad_heads"
        check_grad(w.grad, HR.heads_slice(grad_expected(name, D, k, "unit", True), H), 0.0,
                   f"route {route} graph_values.grad")
    monkeypatch.setenv("MAXK_HEADS_FWD", "heads")
    assert mk.heads_forward_route(400, 64000) == "heads"


def test_layer_helpers(cuda):
    """CSRGraph.aggregate_heads and gat_edge_softmax_heads against their single-head forms."""
    import maxk_layers as ML
    name, k, D, H = "S", 16, 256, 3
    c = case(name, D, k)
    rp, col, _, dv = dgraph(name)
    graph_ = ML.CSRGraph(rp, col)
    w, cv, ci, G = dev_case(c, H, cuda)
    y = graph_.aggregate_heads(cv, ci, D, w, row_div=dv)
    yo, by = fwd_expected(name, D, k, "unit", True)
    check_fwd(y, yo[:H], by[:H], "aggregate_heads")
    gen = torch.Generator(device=cuda).manual_seed(9)
    sd = torch.randn(H, graph_.num_nodes, generator=gen, device=cuda)
    ss = torch.randn(H, graph_.num_nodes, generator=gen, device=cuda)
    alpha = ML.gat_edge_softmax_heads(graph_, sd, ss, 0.2)
    assert tuple(alpha.shape) == (H, col.numel())
    for h in range(H):
        assert M.same_bytes(alpha[h], ML.gat_edge_softmax(graph_, sd[h], ss[h], 0.2))


def test_multi_head_gat_conv_matches_dense(cuda):
    """MaxKMultiHeadGATConv at V = 300, in = 64, out = 8, H = 4, k = 16 against the same layer
    in dense float64 torch (masked dense softmax over the adjacency, per head): the output,
    every parameter's gradient and both input gradients at rtol = atol = 1e-4, the tolerance
    the single-head layer's test composes from the kernels' bounds."""
    import maxk_layers as ML
    torch.manual_seed(4)
    rng = np.random.default_rng(300)
    V, D, k, O_, H = 300, 64, 16, 8, 4
    rp, col = rand_graph(rng, V, 8, hubs=((7, 220),), empty=3)
    graph_ = ML.CSRGraph(T(rp.astype(np.int32), cuda), T(col.astype(np.int32), cuda))
    conv = ML.MaxKMultiHeadGATConv(D, O_, H, negative_slope=0.2).to(cuda)
    with torch.no_grad():
        conv.bias.normal_()
    x = torch.randn(V, D, device=cuda)
    xs, vals, idx = ML.maxk(x, k)
    xs = xs.detach().requires_grad_(True)
    vals = vals.detach().requires_grad_(True)
    out = conv(graph_, xs, vals, idx)
    assert tuple(out.shape) == (V, H, O_)
    gout = torch.randn_like(out)
    names = ["fc.weight", "attn_src", "attn_dst", "bias"]
    P = dict(conv.named_parameters())
    got = torch.autograd.grad(out, [P[n] for n in names] + [xs, vals], gout)

    # dense restatement, float64
    A = torch.zeros(V, V, dtype=torch.float64, device=cuda)
    rows = torch.repeat_interleave(torch.arange(V, device=cuda),
                                   T(np.diff(rp).astype(np.int64), cuda))
    A[rows, T(col.astype(np.int64), cuda)] = 1.0
    Q = {n: P[n].detach().double().requires_grad_(True) for n in names}
    xs2 = xs.detach().double().requires_grad_(True)
    vals2 = vals.detach().double().requires_grad_(True)
    xv = torch.zeros(V, D, dtype=torch.float64, device=cuda).scatter(1, idx.long(), vals2)
    # a vertex without in-edges keeps its row unmasked (a finite softmax) and is zeroed by A
    masked = (A == 0) & (A.sum(1, keepdim=True) > 0)
    heads = []
    for h in range(H):
        Wh = Q["fc.weight"][h * O_:(h + 1) * O_]
        h_s = xs2 @ Wh.t()
        e = torch.nn.functional.leaky_relu(
            (h_s @ Q["attn_dst"][h])[:, None] + (h_s @ Q["attn_src"][h])[None, :], 0.2)
        alpha = torch.softmax(e.masked_fill(masked, float("-inf")), 1) * A
        heads.append(alpha @ (xv @ Wh.t()) + Q["bias"][h])
    ref = torch.stack(heads, 1)
    want = torch.autograd.grad(ref, [Q[n] for n in names] + [xs2, vals2], gout.double())
    torch.testing.assert_close(out, ref.float(), rtol=1e-4, atol=1e-4)
    for n, a, b in zip(names + ["x_sparse", "topk_values"], got, want):
        torch.testing.assert_close(a, b.float(), rtol=1e-4, atol=1e-4, msg=lambda m: f"{n}: {m}")
    empty = T(np.diff(rp) == 0, cuda)
    assert not out[empty].sub(conv.bias).abs().max() > 0  # empty rows: the bias alone
