"""GPU: the multi-head GAT edge softmax (edge_softmax_heads.hip) through the binding
(mk.gat_edge_softmax_heads / _backward), the autograd function GATEdgeSoftmaxHeads and
MaxKMultiHeadGATConv, against tests/heads_softmax_ref.py (the float64 reference of
edge_softmax_ref.py per head, with its derived bounds) and against the single-head entries on
each head's slice: the forward byte for byte, the backward byte for byte at H = 1 and inside
the bounds otherwise (DESIGN.md 5.9 has the reason).

Graphs: the corner graph of tests/esm_corner_graph.py and its transpose (rows and columns of
32 / 33 and 512 / 513 edges, a hub of 1700, empty rows first, in a run and last) at item sizes 0
and every entry of EG.CHUNKS, H in 1, 2, 3, 5, 8: every HP (2, 4, 8), two padded head counts
and the one head that is handed to the single-head entry.

Which kernels: at H >= 2 every non-empty forward launches esmh_interleave_kernel<HP>,
esmh_fwd_kernel<HP>, esmh_merge_kernel<0, false> and esmh_normalise_kernel; every non-empty
backward esmh_interleave_kernel<HP>, esmh_bwd_kernel<HP>, esmh_merge_kernel<1, false>,
esmh_bwd_emit_kernel<HP>, esmh_merge_kernel<2, true>, esmh_colsum_kernel<HP> and
esmh_merge_kernel<2, false>; HP = 2, 4, 8, 8 for H = 2, 3, 5, 8; H = 1 launches the
single-head kernels (test_edge_softmax_gpu.py lists them).  So test_corners and
test_equals_single_head reach every instantiation; the others run HP = 4 (H = 3) or HP = 8
(H = 5, 8) as their docstrings say.
"""
import functools

import numpy as np
import pytest
import torch

import edge_grad_ref as R
import edge_softmax_ref as ER
import esm_corner_graph as EG
import heads_softmax_ref as HS
import memguard as M
import numerics as N
import test_edge_softmax_gpu as TG
from test_memguard_gpu import Shrunk
from test_parity_gpu import T, rand_graph

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CHUNKS = (0,) + EG.CHUNKS
HEADS = (1, 2, 3, 5, 8)
HMAX = 8
SLOPE = 0.2
RATIOS: dict = {}


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


# ------------------------------------------------------------------------------- shared data
def _graph(rp, col, C, unread, seed):
    g = N.make_graph(np.random.default_rng(seed), rp, col, C)
    assert unread is None or not (g.col == unread).any()
    return g._replace(unread=unread)


@functools.lru_cache(maxsize=None)
def the_graph(name):
    if name == "corner":
        return _graph(*EG.corner_csr(), EG.NUM_COLS, EG.UNREAD, 1501)
    if name == "transpose":  # column 0: the corner graph's first row, which has no edge
        return _graph(*EG.corner_transpose(), EG.NUM_ROWS, 0, 1502)
    if name == "S":
        return TG.the_graph("S")
    rp, col, C = EG.degenerate()[name]
    return _graph(rp, col, C, None, 1504)


@functools.lru_cache(maxsize=None)
def dev_graph(name):
    g = the_graph(name)
    return T(g.rp, DEV), T(g.col, DEV)


@functools.lru_cache(maxsize=None)
def case(name):
    """HMAX heads of scores and cotangents and their float64 references: computed once, never
    modified; H heads are the first H."""
    g = the_graph(name)
    rng = np.random.default_rng(1600 + len(name))
    s_dst = rng.standard_normal((HMAX, g.R)).astype(np.float32)
    s_src = rng.standard_normal((HMAX, g.C)).astype(np.float32)
    gw = rng.standard_normal((HMAX, g.col.size)).astype(np.float32)
    f = HS.gat_forward_heads(g.rp, g.col, s_dst, s_src, SLOPE)
    b = HS.backward_heads(g.rp, g.col, f, gw, SLOPE, g.C)
    return dict(g=g, s_dst=s_dst, s_src=s_src, gw=gw, f=f, b=b)


def dev_case(c, H):
    return tuple(T(np.ascontiguousarray(c[a][:H]), DEV) for a in ("s_dst", "s_src", "gw"))


def run(mk, name, sd, ss, gw, chunk, slope=SLOPE, dt=None):
    rp, col = dev_graph(name) if dt is None else dt
    w = mk.gat_edge_softmax_heads(rp, col, sd, ss, slope, chunk=chunk)
    gd, gs = mk.gat_edge_softmax_heads_backward(rp, col, sd, ss, w, gw, slope, chunk=chunk)
    return w, gd, gs


def run_single(mk, name, sd, ss, gw, chunk, slope=SLOPE):
    """The H single-head calls the multi-head pair replaces, stacked."""
    rp, col = dev_graph(name)
    w, gd, gs = [], [], []
    for h in range(sd.shape[0]):
        w.append(mk.gat_edge_softmax(rp, col, sd[h], ss[h], slope, chunk=chunk))
        a, b = mk.gat_edge_softmax_backward(rp, col, sd[h], ss[h], w[-1], gw[h], slope,
                                            chunk=chunk)
        gd.append(a)
        gs.append(b)
    return torch.stack(w), torch.stack(gd), torch.stack(gs)


def check(y, ref, bound, what):
    assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape, (y.shape, ref.shape)
    r = N.within(y, ref, bound, what)
    RATIOS[what] = r
    print(f"{what}: err/bound {r:.3f}")
    return r


def check_all(c, H, res, what):
    g = c["g"]
    f, b = HS.heads_slice(c["f"], H), HS.heads_slice(c["b"], H)
    w, gd, gs = res
    check(w, f.w, f.bound, f"{what} w")
    for h in range(H):
        TG.check_rows_sum_to_one(w[h], f.heads[h], g, f"{what} head {h}")
    check(gd, b.g_dst, b.g_dst_bound, f"{what} grad_s_dst")
    check(gs, b.g_src, b.g_src_bound, f"{what} grad_s_src")
    assert not gd[:, T(np.diff(g.rp) == 0, DEV)].any()  # rows without edges: exactly 0
    if g.unread is not None:
        assert not gs[:, g.unread].any()  # a column no edge reads: exactly 0


# ------------------------------------------------------------------------------- the corners
@pytest.mark.parametrize("H", HEADS, ids=[f"H{h}" for h in HEADS])
@pytest.mark.parametrize("name", ["corner", "transpose"])
def test_corners(mk, cuda, name, H):
    """Both directions at every item size, inside the derived bounds; rows sum to one; exact
    zeros for empty rows and the unread column.  Every instantiation (see the module text)."""
    c = case(name)
    sd, ss, gw = dev_case(c, H)
    for chunk in CHUNKS:
        check_all(c, H, run(mk, name, sd, ss, gw, chunk), f"{name} H{H} chunk {chunk}")


# ------------------------------------------------------------------------------- equality
@pytest.mark.parametrize("H", HEADS, ids=[f"H{h}" for h in HEADS])
@pytest.mark.parametrize("name", ["corner", "transpose"])
def test_equals_single_head(mk, cuda, name, H):
    """Head h of w is byte for byte the single-head entry on slice h at the same item size, 0
    included; at H = 1 so are both gradients.  At H >= 2 the backward adds the same numbers in
    the same order but is compiled with other contractions of a multiply into the add it feeds
    (DESIGN.md 5.9): there the gradients are held to the derived bounds alone (test_corners, the
    same graphs and item sizes).  Every instantiation."""
    c = case(name)
    sd, ss, gw = dev_case(c, H)
    for chunk in CHUNKS:
        got = run(mk, name, sd, ss, gw, chunk)
        want = run_single(mk, name, sd, ss, gw, chunk)
        names = ("w", "grad_s_dst", "grad_s_src") if H == 1 else ("w",)
        for a, b, what in zip(got, want, names):
            for h in range(H):
                assert M.same_bytes(a[h].contiguous(), b[h].contiguous()), (name, H, chunk, what, h)


# ------------------------------------------------------------------------------- isolation
@pytest.mark.parametrize("H,h", [(3, 1), (8, 6), (5, 0)])
def test_head_isolation(mk, cuda, H, h):
    """Head h's outputs hold head h's inputs only: the other heads' scores and grad_w replaced
    by other numbers, then sprinkled with NaN, +Inf and -Inf, leave w[h], grad_s_dst[h] and
    grad_s_src[h] the same bytes.  HP = 4 (H = 3) and 8 (H = 8, H = 5 padded)."""
    c = case("corner")
    rng = np.random.default_rng(1700 + H)
    for chunk in (0, 64, 7):
        sd, ss, gw = dev_case(c, H)
        base = run(mk, "corner", sd, ss, gw, chunk)
        assert all(bool(torch.isfinite(t[h]).all()) for t in base)
        for poisoned in (False, True):
            arrs = []
            for a in ("s_dst", "s_src", "gw"):
                x = rng.standard_normal(c[a][:H].shape).astype(np.float32)
                if poisoned:
                    flat = x.reshape(-1)
                    at = rng.choice(flat.size, max(3, flat.size // 50), replace=False)
                    flat[at] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), at.size)
                x[h] = c[a][h]
                arrs.append(T(x, DEV))
            other = run(mk, "corner", *arrs, chunk)
            for a, b in zip(base, other):
                assert M.same_bytes(a[h].contiguous(), b[h].contiguous()), (chunk, poisoned)
            if poisoned:  # and the poison did arrive somewhere else
                assert not bool(torch.isfinite(other[0]).all())


# ------------------------------------------------------------------------------- non-finite
def test_non_finite_classes_in_one_head(mk, cuda):
    """The cases of test_edge_softmax_gpu.py::test_non_finite_classes_gat laid into head 1 of 3
    (HP = 4): a NaN in s_src at a column the hub row and a short row read, a +Inf in s_dst, a
    -Inf in s_src at a vertex whose readers all have other neighbours, a NaN at the unread
    column.  Head 1's NaN / +-Inf masks equal the reference's, the rest is within the bound;
    heads 0 and 2 stay finite and within theirs."""
    H = 3
    c = case("S")
    g = c["g"]
    deg = np.diff(g.rp)
    readers = N._readers(g)
    hubcols = g.col[g.rp[g.hub]:g.rp[g.hub + 1]]
    nan_col = next(int(v) for v in hubcols
                   if ((deg[readers[v]] <= 30) & (readers[v] != g.hub)).any())
    ninf_col = next(int(v) for v in range(g.C)
                    if v != nan_col and v != g.unread and readers[v].size >= 2
                    and (deg[readers[v]] >= 2).all() and g.hub not in readers[v]
                    and not np.isin(readers[v], readers[nan_col]).any())
    inf_row = int(np.flatnonzero((deg >= 3) & (deg <= 30)
                                 & ~np.isin(np.arange(g.R), readers[nan_col])
                                 & ~np.isin(np.arange(g.R), readers[ninf_col]))[0])
    s_dst, s_src = c["s_dst"][:H].copy(), c["s_src"][:H].copy()
    s_src[1, nan_col] = np.nan
    s_src[1, ninf_col] = -np.inf
    s_dst[1, inf_row] = np.inf
    s_src[1, g.unread] = np.nan
    gw = c["gw"][:H]
    f = HS.gat_forward_heads(g.rp, g.col, s_dst, s_src, SLOPE)
    b = HS.backward_heads(g.rp, g.col, f, gw, SLOPE, g.C)
    rows = f.heads[1].rows
    assert np.isnan(f.w[1][rows == g.hub]).all() and np.isnan(f.w[1][rows == inf_row]).all()
    assert (f.w[1][g.col == ninf_col] == 0).all() and np.isfinite(f.w[1]).mean() > 0.85
    assert np.isnan(b.g_src[1]).any() and np.isnan(b.g_dst[1]).any()
    assert not np.isnan(b.g_src[1, g.unread])
    assert np.isfinite(f.w[[0, 2]]).all() and np.isfinite(b.g_src[[0, 2]]).all()
    for chunk in (0, 64):
        sd, ss, gwt = T(s_dst, DEV), T(s_src, DEV), T(np.ascontiguousarray(gw), DEV)
        w, gd, gs = run(mk, "S", sd, ss, gwt, chunk)
        check(w, f.w, f.bound, f"poisoned head chunk {chunk} w")  # the masks: N.same_class
        assert not w[1][T(g.col == ninf_col, DEV)].any()  # exactly 0
        check(gd, b.g_dst, b.g_dst_bound, f"poisoned head chunk {chunk} grad_s_dst")
        check(gs, b.g_src, b.g_src_bound, f"poisoned head chunk {chunk} grad_s_src")


# ------------------------------------------------------------------------------- degenerate
@pytest.mark.parametrize("name", sorted(EG.degenerate()))
def test_degenerate_shapes(mk, cuda, name):
    """The shapes with one of everything at items of 0, 1 and 7 tokens, H = 3 and 8."""
    c = case(name)
    for H in (3, 8):
        sd, ss, gw = dev_case(c, H)
        for chunk in (0, 1, 7):
            check_all(c, H, run(mk, name, sd, ss, gw, chunk), f"{name} H{H} chunk {chunk}")


@pytest.mark.parametrize("H", [1, 3, 8])
def test_no_edges(mk, cuda, H):
    """num_e == 0: the forward has nothing to write, the backward writes zeros everywhere."""
    rows, cols = 40, 17
    rp = torch.zeros(rows + 1, dtype=torch.int32, device=cuda)
    col = torch.empty(0, dtype=torch.int32, device=cuda)
    sd, ss = torch.randn(H, rows, device=cuda), torch.randn(H, cols, device=cuda)
    w = mk.gat_edge_softmax_heads(rp, col, sd, ss, SLOPE)
    assert tuple(w.shape) == (H, 0)
    out = (torch.full((H, rows), float("nan"), device=cuda),
           torch.full((H, cols), float("nan"), device=cuda))
    gd, gs = mk.gat_edge_softmax_heads_backward(rp, col, sd, ss, w, w.clone(), SLOPE, out=out)
    assert tuple(gd.shape) == (H, rows) and tuple(gs.shape) == (H, cols)
    assert not gd.any() and not gs.any()
    assert not torch.isnan(gd).any() and not torch.isnan(gs).any()


# ------------------------------------------------------------------------------- bitwise
@pytest.mark.parametrize("name", ["corner", "transpose"])
def test_bitwise_repeatable(mk, cuda, name):
    """Three runs at H = 5 (HP = 8, three pad heads), the allocator's free blocks (where the next
    workspace comes from) filled differently before each: the same bytes."""
    H = 5
    c = case(name)
    g = c["g"]
    sd, ss, gw = dev_case(c, H)
    n_ws = mk._lib().maxk_gat_edge_softmax_heads_backward_workspace_size(H, g.R, g.C,
                                                                         g.col.size, 0)
    for chunk in (0, 7, 64):
        runs = []
        for fill in (0x00, 0xFF, 0x5A):
            junk = [torch.full((n,), fill, dtype=torch.uint8, device=cuda)
                    for n in (n_ws, n_ws // 2, 4 * H * g.col.size, 4096)]
            del junk
            runs.append(run(mk, name, sd, ss, gw, chunk))
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert M.same_bytes(a, b)


# ------------------------------------------------------------------------------- memory
@pytest.fixture(scope="module")
def arena(cuda):
    return M.Arena(8 << 20, cuda)


def _ops(mk, c, H, chunk):
    """name -> (op(dt, *tensors) -> outputs, input arrays, size query, output sizes)."""
    g = c["g"]
    E = g.col.size
    w32 = ER.as_f32(c["f"].w[:H])
    return {
        "fwd": (lambda dt, sd, ss: (mk.gat_edge_softmax_heads(dt[0], dt[1], sd, ss, SLOPE,
                                                              chunk=chunk),),
                ("s_dst", "s_src"), "maxk_gat_edge_softmax_heads_workspace_size", [4 * H * E]),
        "bwd": (lambda dt, sd, ss, w, gw: mk.gat_edge_softmax_heads_backward(
            dt[0], dt[1], sd, ss, w, gw, SLOPE, chunk=chunk),
            ("s_dst", "s_src", w32, "gw"), "maxk_gat_edge_softmax_heads_backward_workspace_size",
            [4 * H * g.R, 4 * H * g.C]),
    }


def _inputs(c, ins, H):
    return tuple(T(np.ascontiguousarray(c[a][:H]) if isinstance(a, str) else a, DEV)
                 for a in ins)


@pytest.mark.parametrize("H", [3, 8])
@pytest.mark.parametrize("op_name", ["fwd", "bwd"])
def test_memory_contract(mk, arena, cuda, op_name, H):
    """Outputs and workspace from the poisoned, guarded arena (the workspace exactly the queried
    size): outputs fully written and the same bytes in every fill regime, guards untouched,
    inputs unchanged.  The transpose plan is built outside the arena.  HP = 4 and 8."""
    c = case("corner")
    g = c["g"]
    for chunk in (0, 64):
        op, ins, query, out_bytes = _ops(mk, c, H, chunk)[op_name]

        def factory(primer):
            dt = (T(g.rp, DEV), T(g.col, DEV))
            mk.transpose_plan(dt[1], g.C)  # cached on this col tensor, outside the arena
            if primer:
                gen = torch.Generator(device=DEV).manual_seed(5)
                return (dt,) + tuple(torch.rand(t.shape, generator=gen, device=DEV)
                                     for t in _inputs(c, ins, H))
            return (dt,) + _inputs(c, ins, H)

        res = M.run_regimes(op, factory, arena)
        n_ws = getattr(mk._lib(), query)(H, g.R, g.C, g.col.size, chunk)
        assert sorted(a.nbytes for a in arena.allocs) == sorted(out_bytes + [n_ws])
        for regime in ("stale", "ones"):
            for a, b in zip(res["zero"], res[regime]):
                assert M.same_bytes(a, b), (op_name, regime)
        f, b = HS.heads_slice(c["f"], H), HS.heads_slice(c["b"], H)
        ref = {"fwd": [(f.w, f.bound)],
               "bwd": [(b.g_dst, b.g_dst_bound), (b.g_src, b.g_src_bound)]}[op_name]
        for y, (r, bd) in zip(res["ones"], ref):
            check(y, r, bd, f"memguard {op_name} H{H} chunk {chunk}")


@pytest.mark.parametrize("op_name", ["fwd", "bwd"])
def test_undersized_workspace_is_rejected(mk, arena, monkeypatch, op_name):
    """A workspace one byte short of the size query: "workspace too small" from the host-side
    check, before any launch -- the outputs (0xFF-filled) are unchanged, the guards intact."""
    H = 5
    c = case("corner")
    g = c["g"]
    op, ins, query, _ = _ops(mk, c, H, 0)[op_name]
    dt = (T(g.rp, DEV), T(g.col, DEV))
    mk.transpose_plan(dt[1], g.C)
    args = _inputs(c, ins, H)
    torch.cuda.synchronize()
    shrunk = Shrunk(mk._L, query)
    monkeypatch.setattr(mk, "_L", shrunk)
    with arena.active("ones"):
        with pytest.raises(RuntimeError, match="workspace too small"):
            op(dt, *args)
        made = len(arena.allocs)
    assert shrunk.sizes and all(n > 1 for n in shrunk.sizes), shrunk.sizes
    assert made >= 2  # the outputs and the short workspace came from the arena
    arena.check()
    assert arena.untouched()


# ------------------------------------------------------------------------------- capture
def test_hipgraph_capture_forward_and_backward(mk, cuda):
    """Forward and backward at H = 3 captured into one graph on a side stream -- eleven kernels,
    one chain -- and replayed twice: both replays equal the eager result bitwise."""
    H = 3
    c = case("corner")
    g = c["g"]
    rp, col = dev_graph("corner")
    sd, ss, gw = dev_case(c, H)
    for chunk in (0, 64):
        w = torch.empty(H, g.col.size, device=cuda)
        gd, gs = torch.empty(H, g.R, device=cuda), torch.empty(H, g.C, device=cuda)

        def both():
            mk.gat_edge_softmax_heads(rp, col, sd, ss, SLOPE, chunk=chunk, out=w, validate=False)
            mk.gat_edge_softmax_heads_backward(rp, col, sd, ss, w, gw, SLOPE, chunk=chunk,
                                               out=(gd, gs), validate=False)
        both()  # the transpose plan and the allocator's warm-up outside the capture
        torch.cuda.synchronize()
        eager = [t.clone() for t in (w, gd, gs)]
        hg = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        with torch.cuda.graph(hg, stream=side):
            both()
        for _ in range(2):
            for t in (w, gd, gs):
                t.fill_(float("nan"))
            hg.replay()
            torch.cuda.synchronize()
            for a, b in zip(eager, (w, gd, gs)):
                assert M.same_bytes(a, b)
        f = HS.heads_slice(c["f"], H)
        check(w, f.w, f.bound, f"captured chunk {chunk} w")


# ------------------------------------------------------------------------------- the layer
def test_autograd_matches_the_calls_route(mk, cuda, monkeypatch):
    """GATEdgeSoftmaxHeads, then aggregate_heads, a random cotangent, at H = 3 on graph S: alpha,
    the output and the gradients of both scores and of topk_values against the "calls" route (H
    GATEdgeSoftmax.apply) at rtol = atol = 1e-4, the tolerance of
    test_multi_head_gat_conv_matches_dense; and the score gradients against the float64
    reference chained with edge_grad_ref."""
    import maxk_layers as ML
    monkeypatch.setenv("MAXK_BWD_MODE", "csc")
    D, k, H = 64, 16, 3
    c = case("S")
    g = c["g"]
    rng = np.random.default_rng(1800)
    ci = N.selectors(rng, g.C, D, k)
    cv = N.values(rng, (g.C, k), "unit")
    G = np.stack([N.values(rng, (g.R, D), "unit") for _ in range(H)])
    rp, col = dev_graph("S")
    graph_ = ML.CSRGraph(rp, col)
    seen = []
    real = mk.gat_edge_softmax_heads
    monkeypatch.setattr(mk, "gat_edge_softmax_heads",
                        lambda *a, **kw: seen.append(1) or real(*a, **kw))
    res = {}
    for route in ("heads", "calls"):
        monkeypatch.setenv("MAXK_HEADS_SOFTMAX", route)
        sd, ss, _ = dev_case(c, H)
        sd.requires_grad_(True)
        ss.requires_grad_(True)
        tv = T(cv, cuda).requires_grad_(True)
        del seen[:]
        alpha = ML.gat_edge_softmax_heads(graph_, sd, ss, SLOPE)
        assert len(seen) == (1 if route == "heads" else 0)
        y = graph_.aggregate_heads(tv, T(ci, cuda), D, alpha)
        y.backward(T(G, cuda))
        res[route] = (alpha.detach(), y.detach(), sd.grad, ss.grad, tv.grad)
    for a, b, what in zip(res["heads"], res["calls"],
                          ("alpha", "out", "s_dst.grad", "s_src.grad", "topk_values.grad")):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4, msg=lambda m: f"{what}: {m}")
    f = HS.heads_slice(c["f"], H)
    check(res["heads"][0], f.w, f.bound, "autograd alpha")
    ers = [R.edge_grad_ref(g.rp, g.col, cv, ci, G[h], None) for h in range(H)]
    b = HS.backward_heads(g.rp, g.col, f, np.stack([e.ref for e in ers]), SLOPE, g.C,
                          gw_bound=np.stack([R.bound(e) for e in ers]))
    check(res["heads"][2], b.g_dst, b.g_dst_bound, "autograd s_dst.grad")
    check(res["heads"][3], b.g_src, b.g_src_bound, "autograd s_src.grad")


def test_multi_head_gat_conv_both_routes_match_dense(cuda, monkeypatch):
    """MaxKMultiHeadGATConv at V = 300, in = 64, out = 8, H = 4, k = 16 under
    MAXK_HEADS_SOFTMAX=heads and =calls against the same layer in dense float64 torch (masked
    dense softmax over the adjacency, per head): the output, every parameter's gradient and both
    input gradients at rtol = atol = 1e-4.  HP = 4."""
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
    gout = torch.randn(V, H, O_, device=cuda)
    names = ["fc.weight", "attn_src", "attn_dst", "bias"]
    P = dict(conv.named_parameters())

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
    empty = T(np.diff(rp) == 0, cuda)
    for route in ("heads", "calls"):
        monkeypatch.setenv("MAXK_HEADS_SOFTMAX", route)
        out = conv(graph_, xs, vals, idx)
        assert tuple(out.shape) == (V, H, O_)
        got = torch.autograd.grad(out, [P[n] for n in names] + [xs, vals], gout)
        torch.testing.assert_close(out, ref.float(), rtol=1e-4, atol=1e-4)
        for n, a, b in zip(names + ["x_sparse", "topk_values"], got, want):
            torch.testing.assert_close(a, b.float(), rtol=1e-4, atol=1e-4,
                                       msg=lambda m: f"{route} {n}: {m}")
        assert not out[empty].sub(conv.bias).abs().max() > 0  # empty rows: the bias alone


def test_ratios_are_reported():
    """Last in the file: the largest err/bound ratios seen, for the record."""
    for what, r in sorted(RATIOS.items(), key=lambda kv: -kv[1])[:10]:
        print(f"{r:.3f}  {what}")
    assert all(r <= 1.0 for r in RATIOS.values())
