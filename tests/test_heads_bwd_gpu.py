"""GPU: the multi-head feature backward -- maxk_sspmm_backward_heads (sspmm_push.hip) through
the binding (sspmm_backward_heads), the autograd surface (maxk_spgemm_heads) and the layer
(MaxKMultiHeadGATConv) -- against tests/heads_ref.py: the oracle's backward per head summed in
double, within heads_ref.bound_feat_grad_heads, (n + 8) * 2^-24 * sum|terms| with n = H times
the edges into the column (plus the 2^-149 floor for subnormal inputs).  Shapes are the module
graphs of tests/numerics.py (S: hub rows of 590 and 200 edges, empty rows; Dn: average degree
160, a hub row of 390; R: rectangular; an unread column in each), each at chunk 0 and at 64
tokens, where both phases cut every hub row and every hub column over many items.

Kernel instantiations and the cases that launch them (sspmm_bwd_heads_kernel<LG, 4, HB, X4>:
HB = 4 at H <= 4 and 8 at H = 8, every shape runs both; LG lanes per edge, pow2ceil(k / 4) in
the four-l-per-lane form X4 for k % 4 == 0, pow2ceil(k) in the scalar form):

  <2, 4, HB, 1>   k = 8             <4, 4, HB, 1>   k = 16
  <8, 4, HB, 1>   k = 24, 32        <32, 4, HB, 1>  k = 96 (idle lanes q >= 24)
  <4, 4, HB, 0>   k = 3             <8, 4, HB, 0>   k = 7 (odd D = 9: scalar row staging)
  <64, 4, HB, 0>  k = 70: two passes over l (parity and the H = 1 case only)
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
SHAPES = [(3, 64), (8, 256), (16, 256), (24, 256), (32, 256), (96, 256), (7, 9)]
EXTRA_SHAPES = [(70, 256)]  # k % 4 != 0 past 64: the scalar form's passes over l


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    yield maxk_cuda_kernels
    for f in (case, per_head):  # [8, C, k] references: not kept past the module
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
    Computed once, never modified.  Weights in [0.5, 1.5), grad_out in the regime."""
    g = graph(name)
    rng = np.random.default_rng(D * 1000 + k * 11 + len(regime) + 57)
    ci = N.selectors(rng, g.C, D, k)
    w = rng.uniform(0.5, 1.5, (HMAX, g.col.size)).astype(np.float32)
    G = N.values(rng, (HMAX, g.R, D), regime)
    return dict(g=g, ci=ci, w=w, G=G, unit=N.floor_unit(regime))


@functools.lru_cache(maxsize=None)
def per_head(name, D, k, regime, div):
    """What heads_ref.feat_grad_heads_ref and bound_feat_grad_heads sum over the heads, kept per
    head so that every H shares one set of oracle runs: (the oracle's backward [HMAX, C, k] in
    double, the oracle on |w| and |G| [HMAX, C, k], the addends of one head [C, k])."""
    c = case(name, D, k, regime)
    g = c["g"]
    refs, sabs = [], []
    for h in range(HMAX):
        gh = HR.head_graph(g, c["w"][h], div)
        refs.append(N.bwd_ref(gh, c["G"][h], c["ci"]).astype(np.float64))
        sabs.append(N.O.sspmm_bwd(gh.rp, gh.col, gh.ev, N._pad(N._finite_abs(c["G"][h])), c["ci"],
                                  row_div=gh.div).astype(np.float64))
    return np.stack(refs), np.stack(sabs), N.count_bwd(g, c["ci"], D).astype(np.float64)


def expected(name, D, k, H, regime="unit", div=True):
    """(feat_grad_heads_ref, bound_feat_grad_heads) of the first H heads of case()."""
    refs, sabs, n1 = per_head(name, D, k, regime, div)
    return refs[:H].sum(0), N._bound(H * n1, sabs[:H].sum(0), N.floor_unit(regime))


def ref64(g, w, G, ci, div=True):
    """sum_h sum_{e = (r -> c)} w[h, e] * G[h, r, ci[c, l]] / div[r] in float64, G / div first as
    the kernel divides, selectors >= D reading 0: exact for small-integer inputs."""
    rows = R.edge_rows(g.rp)
    sel = ci[g.col].astype(np.int64)  # [E, k]
    out = np.zeros(ci.shape, np.float64)
    for h in range(w.shape[0]):
        Gp = np.zeros((g.R, N.FULL), np.float64)
        Gp[:, :G.shape[2]] = G[h]
        if div:
            Gp /= g.div.astype(np.float64)[:, None]
        with np.errstate(invalid="ignore"):
            np.add.at(out, g.col, w[h].astype(np.float64)[:, None] *
                      np.take_along_axis(Gp[rows], sel, 1))
    return out


def run(mk, name, w, G, ci, div=True, chunk=0, out=None, gt=None, validate=None, plan=None):
    rp, col, _, dv = dgraph(name) if gt is None else gt
    return mk.sspmm_backward_heads(rp, col, w, G, ci, row_div=dv if div else None, chunk=chunk,
                                   out=out, validate=validate, plan=plan)


def check(y, ref, bound, what):
    assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape
    r = N.within(y, ref, bound, what)
    print(f"{what}: err/bound {r:.3f}")
    return r


def dev_case(c, H, cuda):
    return T(c["w"][:H], cuda), T(c["G"][:H], cuda), T(c["ci"], cuda)


# ------------------------------------------------------------------------------- parity
def test_expected_is_heads_ref():
    """expected() restates heads_ref's two functions from per-head parts; pinned here."""
    name, D, k, H = "R", 64, 3, 3
    c = case(name, D, k)
    for div in (True, False):
        ref, bound = expected(name, D, k, H, "unit", div)
        want = HR.feat_grad_heads_ref(c["g"], c["w"][:H], c["G"][:H], c["ci"], div)
        assert np.allclose(ref, want, rtol=1e-15, atol=0)
        assert np.allclose(bound, HR.bound_feat_grad_heads(c["g"], c["w"][:H], c["G"][:H],
                                                           c["ci"], div), rtol=1e-12, atol=0)
        assert np.abs(ref - ref64(c["g"], c["w"][:H], c["G"][:H], c["ci"], div)).max() <= \
            bound.max()


@pytest.mark.parametrize("H", HEADS, ids=[f"H{h}" for h in HEADS])
@pytest.mark.parametrize("k,D", SHAPES + EXTRA_SHAPES,
                         ids=[f"k{k}-D{D}" for k, D in SHAPES + EXTRA_SHAPES])
@pytest.mark.parametrize("name", ["S", "Dn", "R"])
def test_parity_within_bound(mk, cuda, name, k, D, H):
    c = case(name, D, k)
    w, G, ci = dev_case(c, H, cuda)
    for div in (True, False):
        ref, bound = expected(name, D, k, H, "unit", div)
        for chunk in CHUNKS:
            check(run(mk, name, w, G, ci, div, chunk), ref, bound,
                  f"{name} k{k} D{D} H{H} div={div} chunk {chunk}")


ONE_HEAD = [("S", k, D) for k, D in SHAPES + EXTRA_SHAPES] + [("Dn", 16, 256), ("R", 24, 256)]


@pytest.mark.parametrize("name,k,D", ONE_HEAD, ids=[f"{n}-k{k}-D{D}" for n, k, D in ONE_HEAD])
def test_one_head_is_the_csc_backward(mk, cuda, name, k, D):
    """H = 1: bitwise sspmm_backward(mode="csc") at the same chunk -- each T element is the same
    single product and phase 2 is the same code."""
    c = case(name, D, k)
    w, G, ci = dev_case(c, 1, cuda)
    rp, col, _, dv = dgraph(name)
    for div in (True, False):
        for chunk in CHUNKS:
            one = mk.sspmm_backward(rp, col, w[0], G[0], ci, row_div=dv if div else None,
                                    chunk=chunk, mode="csc")
            assert M.same_bytes(run(mk, name, w, G, ci, div, chunk), one), (div, chunk)


@pytest.mark.parametrize("H", (1, 3, 8))
@pytest.mark.parametrize("name,k,D", [("S", 16, 256), ("S", 7, 9), ("Dn", 32, 256), ("R", 3, 64),
                                      ("S", 96, 256)])
def test_exact_on_small_integers(mk, cuda, name, k, D, H):
    """Integer weights in [-3, 3], integer grad_out in [-4, 4], row_div in {1, 2, 4}: every
    product and partial sum is a multiple of 1/4 below 2^24 (at most 8 heads x 600 edges x 12),
    so fp32 is exact in any order and the result equals the float64 reference exactly.  A dropped
    or doubled (edge, head) term, which a bound could hide, shows here."""
    g = graph(name)
    rng = np.random.default_rng(k * 100 + D + H)
    ci = case(name, D, k)["ci"]
    w = rng.integers(-3, 4, (H, g.col.size)).astype(np.float32)
    G = rng.integers(-4, 5, (H, g.R, D)).astype(np.float32)
    dv = (2.0 ** rng.integers(0, 3, g.R)).astype(np.float32)
    gd = g._replace(div=dv)
    ref = ref64(gd, w, G, ci)
    assert np.abs(ref).max() < 2 ** 22 and (ref != 0).mean() > 0.5
    rp, col, _, _ = dgraph(name)
    for chunk in CHUNKS:
        y = mk.sspmm_backward_heads(rp, col, T(w, cuda), T(G, cuda), T(ci, cuda),
                                    row_div=T(dv, cuda), chunk=chunk)
        assert np.array_equal(y.cpu().numpy().astype(np.float64), ref), chunk


@pytest.mark.parametrize("regime", N.REGIMES)
def test_value_regimes(mk, cuda, regime):
    name, k, D, H = "S", 16, 256, 3
    c = case(name, D, k, regime)
    w, G, ci = dev_case(c, H, cuda)
    ref, bound = expected(name, D, k, H, regime, True)
    for chunk in CHUNKS:
        y = run(mk, name, w, G, ci, True, chunk)
        check(y, ref, bound, f"{regime} chunk {chunk}")
        if regime == "subnormal":
            N.nonzero_where_resolved(y, ref, bound)


# ------------------------------------------------------------------------------- selectors
@pytest.mark.parametrize("H", (1, 8))
@pytest.mark.parametrize("k,D", [(7, 9), (3, 64)])
def test_selectors_past_D_and_repeated(mk, cuda, k, D, H):
    """Selector bytes anywhere in [0, 255] (most of them >= D), with repeats: a slot whose
    selector is >= D is exactly 0 -- with H rows staged at a stride below 256 an unclamped
    selector would read another head's row, and each head holds a marker value no sum of the
    right head's terms could produce --, slots with equal selectors hold equal values, and the
    rest is within the bound."""
    g = graph("S")
    rng = np.random.default_rng(k * 31 + H)
    ci = rng.integers(0, 256, (g.C, k)).astype(np.uint8)
    ci[:, 0] = rng.integers(0, D, g.C)  # at least one kept slot per column
    ci[::3, k - 1] = ci[::3, 0]         # a repeated kept selector
    ci[1::3, 1] = 255                   # the largest byte
    w = rng.uniform(0.5, 1.5, (H, g.col.size)).astype(np.float32)
    G = rng.standard_normal((H, g.R, D)).astype(np.float32)
    G += (1000.0 * (1 + np.arange(H, dtype=np.float32)))[:, None, None]  # head h lives near 1000 (h + 1)
    ref = ref64(g, w, G, ci)
    bound = HR.bound_feat_grad_heads(g, w, G, ci)
    past = ci >= D
    assert past.mean() > 0.3 and (bound[past] == 0).all() and (ref[past] == 0).all()
    for chunk in CHUNKS:
        y = run(mk, "S", T(w, cuda), T(G, cuda), T(ci, cuda), True, chunk, validate=False)
        check(y, ref, bound, f"selectors k{k} D{D} H{H} chunk {chunk}")
        yn = y.cpu().numpy()
        assert not yn[past].any()
        assert np.array_equal(yn[::3, k - 1], yn[::3, 0])
    if H > 1:  # another head's gradient replaced: the slots past D stay 0
        G2 = G.copy()
        G2[1:] = np.nan
        y = run(mk, "S", T(w, cuda), T(G2, cuda), T(ci, cuda), True, 64, validate=False)
        assert not y.cpu().numpy()[past].any()


def test_nan_inf_placement(mk, cuda):
    """A NaN and a +Inf in grad_out[h] make exactly the slots non-finite that select that (row,
    column) through an edge (the class masks equal the reference's); a NaN in a column none of
    the row's destinations selects, and a whole NaN row without edges, change nothing, bitwise."""
    name, k, D, H = "S", 16, 256, 3
    c = case(name, D, k)
    g, ci = c["g"], c["ci"]
    w, G = c["w"][:H], c["G"][:H].copy()
    deg = np.diff(g.rp)
    base = {chunk: run(mk, name, T(w, cuda), T(G, cuda), T(ci, cuda), True, chunk)
            for chunk in CHUNKS}
    # reaches nothing: an unselected column of a short row, an empty row
    r = int(np.flatnonzero((deg >= 3) & (deg <= 20))[0])
    sel = ci[g.col[g.rp[r]:g.rp[r + 1]]].ravel()
    free = np.setdiff1d(np.arange(D), sel)
    empty = np.flatnonzero(deg == 0)
    assert free.size and empty.size
    G[:, r, free[0]] = np.nan
    G[:, empty[0]] = np.nan
    for chunk in CHUNKS:
        y = run(mk, name, T(w, cuda), T(G, cuda), T(ci, cuda), True, chunk)
        assert M.same_bytes(y, base[chunk]), chunk
    # reaches its slots: the hub row (cut over items at chunk 64) and a short row, one head each
    hubcols = g.col[g.rp[g.hub]:g.rp[g.hub + 1]]
    G[1, g.hub, ci[int(hubcols[5]), 2]] = np.nan
    G[2, g.hub, ci[int(hubcols[9]), 0]] = np.inf
    G[0, r, sel[0]] = -np.inf
    ref = ref64(g, w, G, ci)
    bound = HR.bound_feat_grad_heads(g, w, G, ci)
    bad = ~np.isfinite(ref)
    assert np.isnan(ref).any() and np.isposinf(ref).any() and np.isneginf(ref).any()
    assert 3 <= bad.sum() < 0.05 * ref.size
    for chunk in CHUNKS:
        y = run(mk, name, T(w, cuda), T(G, cuda), T(ci, cuda), True, chunk)
        check(y, ref, bound, f"nan/inf chunk {chunk}")
        yn = y.cpu().numpy()
        assert np.array_equal(yn[~bad].view(np.uint32),
                              base[chunk].cpu().numpy()[~bad].view(np.uint32))


# ------------------------------------------------------------------------------- bitwise
@pytest.mark.parametrize("name,k,D,H", [("S", 16, 256, 3), ("Dn", 32, 256, 8), ("R", 3, 64, 2),
                                        ("S", 96, 256, 8)])
def test_power_of_two_scale(mk, cuda, name, k, D, H):
    """Two calls into differently prefilled outputs give the same bytes; scaling grad_out or the
    weights by a power of two scales the result, bitwise."""
    c = case(name, D, k)
    w, G, ci = dev_case(c, H, cuda)
    for chunk in CHUNKS:
        a = torch.full((c["g"].C, k), float("nan"), device=cuda)
        b = torch.full((c["g"].C, k), 1e30, device=cuda)
        run(mk, name, w, G, ci, True, chunk, out=a)
        run(mk, name, w, G, ci, True, chunk, out=b)
        assert M.same_bytes(a, b)
        assert M.same_bytes(run(mk, name, w, G * 1024.0, ci, True, chunk), a * 1024.0)
        assert M.same_bytes(run(mk, name, w * 0.25, G, ci, True, chunk), a * 0.25)


# ------------------------------------------------------------------------------- memory
@pytest.fixture(scope="module")
def arena(cuda):
    return M.Arena(16 << 20, cuda)  # graph S at k = 16: T 0.5 MB, out 38 KB


@pytest.mark.parametrize("k,D,H", [(16, 256, 3), (16, 256, 8), (3, 64, 3)])
def test_memory_contract(mk, arena, cuda, k, D, H):
    """Output and workspace from the poisoned, guarded arena (the workspace is exactly the
    queried size), zero-filled, stale and 0xFF-filled: the output is fully written and the same
    bytes in every fill regime, the guards are untouched, the inputs unchanged."""
    c, p = case("S", D, k), case("S", D, k, "small")
    g = c["g"]
    E = g.col.size

    def factory(primer):
        s = p if primer else c
        gt = tuple(T(a, DEV) for a in (g.rp, g.col, g.ev, g.div))
        plan = mk.transpose_plan(gt[1], g.C, cache=False)  # built outside the arena
        return (gt, plan) + dev_case(s, H, DEV)

    ref, bound = expected("S", D, k, H, "unit", True)
    for chunk in CHUNKS:
        def op(gt, plan, w, G, ci):
            y = run(mk, "S", w, G, ci, True, chunk, gt=gt, plan=plan)
            assert arena.owns(y)
            return (y,)
        res = M.run_regimes(op, factory, arena)
        assert len(arena.allocs) == 2  # the output and the workspace
        n = mk._lib().maxk_sspmm_backward_heads_workspace_size(g.R, g.C, E, D, k, H, chunk)
        assert sorted(a.nbytes for a in arena.allocs) == sorted((g.C * k * 4, n))
        for regime, r in res.items():
            check(r[0], ref, bound, f"memguard k{k} D{D} H{H} chunk {chunk} {regime}")
        for regime in ("stale", "ones"):
            assert M.same_bytes(res["zero"][0], res[regime][0]), regime


def test_short_workspace_writes_nothing(mk, cuda):
    name, k, D, H = "S", 16, 256, 3
    c = case(name, D, k)
    g = c["g"]
    w, G, ci = dev_case(c, H, cuda)
    rp, col, _, dv = dgraph(name)
    col_ptr, csc_eid = mk.transpose_plan(col, g.C)
    shape = (g.R, g.C, g.col.size, D, k, H, 0)
    L = mk._lib()
    n = L.maxk_sspmm_backward_heads_workspace_size(*shape)
    ws = torch.full((n,), 0x5A, dtype=torch.uint8, device=cuda)
    out = torch.full((g.C, k), 7.0, device=cuda)
    torch.cuda.synchronize()
    rc = L.maxk_sspmm_backward_heads(rp.data_ptr(), col.data_ptr(), w.data_ptr(), G.data_ptr(),
                                     dv.data_ptr(), ci.data_ptr(), col_ptr.data_ptr(),
                                     csc_eid.data_ptr(), out.data_ptr(), *shape, ws.data_ptr(),
                                     n - 1, None)
    assert rc == -1 and b"workspace too small" in L.maxk_last_error()
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()) and bool((out == 7.0).all())


def test_no_edges_writes_zeros(mk, cuda):
    rp = torch.zeros(41, dtype=torch.int32, device=cuda)
    col = torch.zeros(0, dtype=torch.int32, device=cuda)
    ci = torch.arange(8, dtype=torch.uint8, device=cuda).repeat(50, 1)
    for chunk in CHUNKS:
        out = torch.full((50, 8), float("nan"), device=cuda)
        y = mk.sspmm_backward_heads(rp, col, torch.zeros(3, 0, device=cuda),
                                    torch.randn(3, 40, 64, device=cuda), ci, chunk=chunk, out=out)
        assert y is out and not out.any()


# ------------------------------------------------------------------------------- streams
def test_runs_on_current_stream(mk, cuda):
    name, k, D, H = "S", 16, 256, 3
    w, G, ci = dev_case(case(name, D, k), H, cuda)
    ref, bound = expected(name, D, k, H)
    run(mk, name, w, G, ci)  # the transpose plan is built on the default stream
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        y = run(mk, name, w, G, ci)
    s.synchronize()
    check(y, ref, bound, "side stream")


def test_hipgraph_capture_single_chain(mk, cuda):
    """One capture of the call into a preallocated output, replayed twice with the weights and
    grad_out changed in place between the replays.  The captured graph is one linear chain --
    phase 1, the csc sum, the fix-up: no node has two successors or two predecessors."""
    name, k, D, H = "S", 16, 256, 3
    c, c2 = case(name, D, k), case(name, D, k, "small")
    g = c["g"]
    w, G, ci = dev_case(c, H, cuda)
    y = torch.empty(g.C, k, device=cuda)
    run(mk, name, w, G, ci, out=y)  # graph check, plan and allocator warm-up outside the capture
    torch.cuda.synchronize()
    hg = torch.cuda.CUDAGraph(keep_graph=True)  # the hipGraph_t stays readable after the capture
    with torch.cuda.graph(hg):
        run(mk, name, w, G, ci, out=y, validate=False)
    n_nodes, edges = graph_topology(hg.raw_cuda_graph())
    print(f"captured graph: {n_nodes} nodes, {len(edges)} edges")
    assert n_nodes == 3 and len(edges) == 2, (n_nodes, edges)
    succ, pred = [a for a, _ in edges], [b for _, b in edges]
    assert len(set(succ)) == len(succ) and len(set(pred)) == len(pred)
    hg.instantiate()
    ref, bound = expected(name, D, k, H)
    y.fill_(float("nan"))
    hg.replay()
    torch.cuda.synchronize()
    check(y, ref, bound, "replay 1")
    w2 = np.ascontiguousarray(c["w"][HMAX - H:])  # other weights, the same shape
    w.copy_(T(w2, cuda))
    G.copy_(T(c2["G"][:H], cuda))
    y.fill_(float("nan"))
    hg.replay()
    torch.cuda.synchronize()
    check(y, HR.feat_grad_heads_ref(g, w2, c2["G"][:H], c["ci"]),
          HR.bound_feat_grad_heads(g, w2, c2["G"][:H], c["ci"]), "replay 2")


# ------------------------------------------------------------------------------- autograd
def test_autograd_routes(F, mk, cuda, monkeypatch):
    """maxk_spgemm_heads(...).backward at H = 3, (16, 256), graph S: with MAXK_HEADS_BWD=heads
    one sspmm_backward_heads call and no sspmm_backward call, with calls H sspmm_backward calls;
    topk_values.grad within the bound both ways, graph_values.grad the same bytes."""
    monkeypatch.delenv("MAXK_BWD_MODE", raising=False)
    name, k, D, H = "S", 16, 256, 3
    c = case(name, D, k)
    rp, col, _, dv = dgraph(name)
    cv0 = torch.randn(c["g"].C, k, generator=torch.Generator().manual_seed(3)).to(cuda)
    calls = []
    for fn in ("sspmm_backward_heads", "sspmm_backward"):
        real = getattr(mk, fn)
        monkeypatch.setattr(
            mk, fn, lambda *a, _r=real, _n=fn, **kw: calls.append(_n) or _r(*a, **kw))
    ref, bound = expected(name, D, k, H)
    grads = {}
    for route in ("heads", "calls"):
        monkeypatch.setenv("MAXK_HEADS_BWD", route)
        w, G, ci = dev_case(c, H, cuda)
        w.requires_grad_(True)
        cv = cv0.clone().requires_grad_(True)
        y = F.maxk_spgemm_heads(rp, col, w, cv, ci, D, dv)
        del calls[:]
        y.backward(G)
        assert calls == (["sspmm_backward_heads"] if route == "heads"
                         else ["sspmm_backward"] * H), (route, calls)
        assert cv.grad is not None and cv.grad.shape == cv.shape
        check(cv.grad, ref, bound, f"route {route} topk_values.grad")
        grads[route] = (w.grad.clone(), cv.grad.clone())
    assert M.same_bytes(grads["heads"][0], grads["calls"][0])
    # unforced: the rule's route for this graph (k = 16: the H calls would run csc)
    monkeypatch.delenv("MAXK_HEADS_BWD")
    g = c["g"]
    assert mk.heads_backward_route(k, g.col.size, g.C, g.R) == "heads"


def test_multi_head_gat_conv_feature_gradient(cuda, monkeypatch):
    """A MaxKMultiHeadGATConv step on the fused route (V = 300, in = 64, out = 8, H = 4, k = 16):
    topk_values.grad against the layer restated in dense float64 torch, at the tolerance of
    test_heads_gpu.test_multi_head_gat_conv_matches_dense, rtol = atol = 1e-4."""
    import maxk_cuda_kernels as mk
    import maxk_layers as ML
    monkeypatch.setenv("MAXK_HEADS_BWD", "heads")
    calls = []
    real = mk.sspmm_backward_heads
    monkeypatch.setattr(mk, "sspmm_backward_heads",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    torch.manual_seed(4)
    rng = np.random.default_rng(300)
    V, D, k, O_, H = 300, 64, 16, 8, 4
    rp, col = rand_graph(rng, V, 8, hubs=((7, 220),), empty=3)
    graph_ = ML.CSRGraph(T(rp.astype(np.int32), cuda), T(col.astype(np.int32), cuda))
    conv = ML.MaxKMultiHeadGATConv(D, O_, H, negative_slope=0.2).to(cuda)
    x = torch.randn(V, D, device=cuda)
    xs, vals, idx = ML.maxk(x, k)
    xs = xs.detach()
    vals = vals.detach().requires_grad_(True)
    out = conv(graph_, xs, vals, idx)
    gout = torch.randn_like(out)
    (got,) = torch.autograd.grad(out, [vals], gout)
    assert calls == [1]

    A = torch.zeros(V, V, dtype=torch.float64, device=cuda)
    rows = torch.repeat_interleave(torch.arange(V, device=cuda),
                                   T(np.diff(rp).astype(np.int64), cuda))
    A[rows, T(col.astype(np.int64), cuda)] = 1.0
    P = {n: p.detach().double() for n, p in conv.named_parameters()}
    vals2 = vals.detach().double().requires_grad_(True)
    xv = torch.zeros(V, D, dtype=torch.float64, device=cuda).scatter(1, idx.long(), vals2)
    masked = (A == 0) & (A.sum(1, keepdim=True) > 0)
    heads = []
    for h in range(H):
        Wh = P["fc.weight"][h * O_:(h + 1) * O_]
        h_s = xs.double() @ Wh.t()
        e = torch.nn.functional.leaky_relu(
            (h_s @ P["attn_dst"][h])[:, None] + (h_s @ P["attn_src"][h])[None, :], 0.2)
        alpha = torch.softmax(e.masked_fill(masked, float("-inf")), 1) * A
        heads.append(alpha @ (xv @ Wh.t()) + P["bias"][h])
    (want,) = torch.autograd.grad(torch.stack(heads, 1), [vals2], gout.double())
    torch.testing.assert_close(got, want.float(), rtol=1e-4, atol=1e-4)
