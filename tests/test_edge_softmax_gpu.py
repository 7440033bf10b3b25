"""GPU: the edge softmax (edge_softmax.hip), both forms and both directions, through the binding
(mk.edge_softmax, mk.gat_edge_softmax and their backwards), the autograd functions and
MaxKGATConv, against tests/edge_softmax_ref.py: the formulas in numpy float64, pinned to torch
autograd by test_edge_softmax_cpu.py, with derived per-element bounds.  Graphs are the module
graphs of tests/numerics.py (S: hub rows of 590 and 200 edges and 20 empty rows, most rows short
enough for the lane groups; Dn: average degree 160, the whole-wave walk; R: rectangular, an
unread column), each at chunk 0 and at 64 tokens, where every hub row -- and hub column of the
backward's column sums -- is cut over many items and merged from their partials; a graph with
rows of 1400 and 530 edges reaches the walk of pieces longer than a wave's registers hold.

Which test launches which kernel (every non-empty call launches all of its form's kernels: the
rules of launch_fwd / launch_bwd_rows): esm_fwd_kernel<0>, esm_merge_kernel<0> and
esm_normalise_kernel by every plain forward (test_parity_within_bound), esm_fwd_kernel<1> by
every GAT forward; esm_bwd_kernel<0/1>, esm_merge_kernel<1> and esm_bwd_emit_kernel<0/1> by the
plain / GAT backward, esm_merge_kernel<2> and esm_colsum_kernel by the GAT backward (the same
test).
"""
import functools

import numpy as np
import pytest
import torch

import edge_grad_ref as R
import edge_softmax_ref as ER
import memguard as M
import numerics as N
from test_memguard_gpu import Shrunk
from test_numerics_gpu import dgraph, graph
from test_parity_gpu import T, rand_graph

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CHUNKS = (0, 64)
SLOPES = (0.2, 0.0, 1.0)
RATIOS: dict = {}


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


# ------------------------------------------------------------------------------- shared data
@functools.lru_cache(maxsize=None)
def low_degree_graph():
    """300 vertices of average degree 3 (many rows of exactly one edge), a hub row of 290, empty
    rows, an unread column: the exact values of the smallest rows."""
    rng = np.random.default_rng(7010)
    rp, col = rand_graph(rng, 300, 3, hubs=((5, 290),), empty=5)
    return N.make_graph(rng, rp, col, 300, unread=17)


@functools.lru_cache(maxsize=None)
def long_row_graph():
    """200 x 1500 with rows of 1400 and 530 edges: pieces past the 512 edges a wave holds in
    registers, whole (chunk 4096) and cut (chunk 600)."""
    rng = np.random.default_rng(7011)
    rp, col = rand_graph(rng, 200, 10, hubs=((4, 1400), (90, 530)), empty=3, cols=1500)
    return N.make_graph(rng, rp, col, 1500, unread=777)


def the_graph(name):
    return {"L": low_degree_graph, "H": long_row_graph}.get(name, lambda: graph(name))()


@functools.lru_cache(maxsize=None)
def dev_graph(name):
    g = the_graph(name)
    return T(g.rp, DEV), T(g.col, DEV)


@functools.lru_cache(maxsize=None)
def case(name, slope=0.2, scale=1.0):
    """Inputs and references of one (graph, slope, magnitude): computed once, never modified.
    The references are float64 evaluations on the fp32 inputs."""
    g = the_graph(name)
    rng = np.random.default_rng(int(slope * 10) + 13 * len(name) + int(np.log10(scale)) + 77)
    s_dst = (rng.standard_normal(g.R) * scale).astype(np.float32)
    s_src = (rng.standard_normal(g.C) * scale).astype(np.float32)
    gw = rng.standard_normal(g.col.size).astype(np.float32)
    f = ER.gat_forward(g.rp, g.col, s_dst, s_src, slope)
    lg = f.l.astype(np.float32)  # the plain form's input: these logits, as fp32
    fp = ER.forward(g.rp, lg)
    return dict(g=g, s_dst=s_dst, s_src=s_src, gw=gw, slope=slope, f=f,
                b=ER.backward(g.rp, g.col, f, gw, slope, g.C), lg=lg, fp=fp,
                bp=ER.backward(g.rp, g.col, fp, gw))


def check(y, ref, bound, what):
    assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape, (y.shape, ref.shape)
    r = N.within(y, ref, bound, what)
    RATIOS[what] = r
    print(f"{what}: err/bound {r:.3f}")
    return r


def check_rows_sum_to_one(w, f, g, what):
    deg = np.diff(g.rp)
    fin = np.isfinite(ER._row_reduce(np.add, f.w, g.rp, 0.0)) & (deg > 0)
    sums = ER._row_reduce(np.add, w.detach().cpu().numpy().astype(np.float64), g.rp, 1.0)
    b = ER.row_sum_bound(f)
    q = np.abs(sums[fin] - 1.0) / (b[fin] + 1e-15)
    print(f"{what}: row sums |sum - 1| / bound {q.max():.3f}")
    assert q.max() <= 1.0, what


def run_all(mk, name, c, chunk, dt=None):
    """(w, gat grads, plain w, plain grad) of one case at one chunk."""
    rp, col = dev_graph(name) if dt is None else dt
    sd, ss, gw = T(c["s_dst"], DEV), T(c["s_src"], DEV), T(c["gw"], DEV)
    w = mk.gat_edge_softmax(rp, col, sd, ss, c["slope"], chunk=chunk)
    gd, gs = mk.gat_edge_softmax_backward(rp, col, sd, ss, w, gw, c["slope"], chunk=chunk)
    wp = mk.edge_softmax(rp, T(c["lg"], DEV), chunk=chunk)
    gl = mk.edge_softmax_backward(rp, wp, gw, chunk=chunk)
    return w, gd, gs, wp, gl


def check_all(c, res, what):
    g = c["g"]
    w, gd, gs, wp, gl = res
    check(w, c["f"].w, c["f"].bound, f"{what} gat w")
    check_rows_sum_to_one(w, c["f"], g, f"{what} gat")
    check(gd, c["b"].g_dst, c["b"].g_dst_bound, f"{what} grad_s_dst")
    check(gs, c["b"].g_src, c["b"].g_src_bound, f"{what} grad_s_src")
    check(wp, c["fp"].w, c["fp"].bound, f"{what} plain w")
    check_rows_sum_to_one(wp, c["fp"], g, f"{what} plain")
    check(gl, c["bp"].gl, c["bp"].gl_bound, f"{what} grad_logits")
    deg = np.diff(g.rp)
    assert not gd[T(deg == 0, DEV)].any()  # a row without edges: exactly 0
    if g.unread is not None:
        assert float(gs[g.unread]) == 0.0  # a column no edge reads: exactly 0


# ------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("name", ["S", "Dn", "R"])
def test_parity_within_bound(mk, cuda, name, slope):
    c = case(name, slope)
    for chunk in CHUNKS:
        check_all(c, run_all(mk, name, c, chunk), f"{name} slope {slope} chunk {chunk}")


def test_rows_of_one_edge_are_exact(mk, cuda):
    """w = 1 and gl = gz = 0 exactly on a row of one edge, whatever its scores."""
    c = case("L")
    g = c["g"]
    deg = np.diff(g.rp)
    one = g.rp[:-1][deg == 1]
    assert one.size >= 20
    sel = T(one.astype(np.int64), DEV)
    for chunk in CHUNKS:
        res = run_all(mk, "L", c, chunk)
        check_all(c, res, f"L chunk {chunk}")
        w, gd, gs, wp, gl = res
        assert bool((w[sel] == 1).all()) and bool((wp[sel] == 1).all())
        assert not gl[sel].any() and not gd[T(deg == 1, DEV)].any()


@pytest.mark.parametrize("slope", [0.2, 1.0])
def test_pieces_past_the_register_walk(mk, cuda, slope):
    """Rows of 1400 and 530 edges at items of 600 tokens (cut pieces of up to 600 edges: the
    three-pass walk, then the second walk over staged logits), of 4096 (the rows whole) and of
    64."""
    c = case("H", slope)
    for chunk in (600, 4096, 64):
        check_all(c, run_all(mk, "H", c, chunk), f"H slope {slope} chunk {chunk}")


# ------------------------------------------------------------------------------- value regimes
@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e3])
def test_value_regimes(mk, cuda, scale):
    """Scores of magnitude 1, 1e-3 and 1e3: at 1e3 exp(l) overflows without the max subtracted,
    so everything must stay finite, and within the bound."""
    c = case("S", 0.2, scale)
    for chunk in CHUNKS:
        res = run_all(mk, "S", c, chunk)
        for t in res:
            assert bool(torch.isfinite(t).all())
        check_all(c, res, f"S scale {scale:g} chunk {chunk}")


def test_spread_past_200_underflows_inside_the_floor(mk, cuda):
    """The hub row's logits spread over 260, a short row's over 300: the smallest weights
    underflow (subnormal or 0), stay inside the bound's floor, and the rows still sum to 1."""
    c = case("S")
    g = c["g"]
    deg = np.diff(g.rp)
    lg = c["lg"].copy()
    hb, he = g.rp[g.hub], g.rp[g.hub + 1]
    lg[hb:he] = np.linspace(-260.0, 0.0, he - hb).astype(np.float32)
    r = int(np.flatnonzero((deg >= 6) & (deg <= 20))[0])
    lg[g.rp[r]:g.rp[r + 1]] = np.linspace(150.0, -150.0, deg[r]).astype(np.float32)
    fp = ER.forward(g.rp, lg)
    tiny = ER.as_f32(fp.w) < np.float32(2.0 ** -126)
    assert tiny[hb:he].sum() >= 100 and tiny[g.rp[r]:g.rp[r + 1]].any()
    rp, _ = dev_graph("S")
    for chunk in CHUNKS:
        wp = mk.edge_softmax(rp, T(lg, DEV), chunk=chunk)
        check(wp, fp.w, fp.bound, f"spread chunk {chunk}")
        check_rows_sum_to_one(wp, fp, g, f"spread chunk {chunk}")
        gl = mk.edge_softmax_backward(rp, wp, T(c["gw"], DEV), chunk=chunk)
        bp = ER.backward(g.rp, g.col, fp, c["gw"])
        check(gl, bp.gl, bp.gl_bound, f"spread chunk {chunk} grad_logits")


# ------------------------------------------------------------------------------- non-finite
def test_non_finite_classes_gat(mk, cuda):
    """A NaN in s_src at a column the hub row and a short row read; a +Inf in s_dst; a -Inf in
    s_src at a vertex whose readers all have other neighbours; a NaN at the unread column.  The
    NaN / +-inf masks equal the reference's, every other row is within the bound."""
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
    s_dst, s_src = c["s_dst"].copy(), c["s_src"].copy()
    s_src[nan_col] = np.nan
    s_src[ninf_col] = -np.inf
    s_dst[inf_row] = np.inf
    s_src[g.unread] = np.nan
    f = ER.gat_forward(g.rp, g.col, s_dst, s_src, 0.2)
    b = ER.backward(g.rp, g.col, f, c["gw"], 0.2, g.C)
    rows = f.rows
    assert np.isnan(f.w[rows == g.hub]).all() and np.isnan(f.w[rows == inf_row]).all()
    assert (f.w[g.col == ninf_col] == 0).all() and np.isfinite(f.w).mean() > 0.85
    assert np.isnan(b.g_src).any() and np.isnan(b.g_dst).any() and not np.isnan(b.g_src[g.unread])
    rp, col = dev_graph("S")
    for chunk in CHUNKS:
        sd, ss, gw = T(s_dst, DEV), T(s_src, DEV), T(c["gw"], DEV)
        w = mk.gat_edge_softmax(rp, col, sd, ss, 0.2, chunk=chunk)
        N.same_class(w, ER.as_f32(f.w))
        check(w, f.w, f.bound, f"poisoned chunk {chunk} w")
        assert not w[T(g.col == ninf_col, DEV)].any()  # exactly 0
        gd, gs = mk.gat_edge_softmax_backward(rp, col, sd, ss, w, gw, 0.2, chunk=chunk)
        check(gd, b.g_dst, b.g_dst_bound, f"poisoned chunk {chunk} grad_s_dst")
        check(gs, b.g_src, b.g_src_bound, f"poisoned chunk {chunk} grad_s_src")


def test_non_finite_classes_plain(mk, cuda):
    """Plain logits: a stretch of -Inf inside the hub row as long as two items of 64 tokens (a
    cut piece of nothing but -Inf: exactly 0, the row unharmed), a row of nothing but -Inf (all
    NaN), a row with a +Inf and a row with a NaN (all NaN)."""
    c = case("S")
    g = c["g"]
    deg = np.diff(g.rp)
    lg = c["lg"].copy()
    hb = g.rp[g.hub]
    lg[hb + 100:hb + 300] = -np.inf
    short = [int(r) for r in np.flatnonzero((deg >= 3) & (deg <= 30))[:3]]
    lg[g.rp[short[0]]:g.rp[short[0] + 1]] = -np.inf
    lg[g.rp[short[1]] + 1] = np.inf
    lg[g.rp[short[2]] + 2] = np.nan
    fp = ER.forward(g.rp, lg)
    bp = ER.backward(g.rp, g.col, fp, c["gw"])
    for r in short:
        assert np.isnan(fp.w[g.rp[r]:g.rp[r + 1]]).all()
    assert (fp.w[hb + 100:hb + 300] == 0).all() and np.isfinite(fp.w[hb:g.rp[g.hub + 1]]).all()
    rp, _ = dev_graph("S")
    for chunk in CHUNKS:
        wp = mk.edge_softmax(rp, T(lg, DEV), chunk=chunk)
        check(wp, fp.w, fp.bound, f"plain poisoned chunk {chunk} w")
        assert not wp[hb + 100:hb + 300].any()
        check_rows_sum_to_one(wp, fp, g, f"plain poisoned chunk {chunk}")
        gl = mk.edge_softmax_backward(rp, wp, T(c["gw"], DEV), chunk=chunk)
        check(gl, bp.gl, bp.gl_bound, f"plain poisoned chunk {chunk} grad_logits")


# ------------------------------------------------------------------------------- bitwise
@pytest.mark.parametrize("name", ["S", "Dn", "R"])
def test_bitwise_repeatable(mk, cuda, name):
    """Three runs of both forms and directions, the allocator's free blocks (where the next
    workspace comes from) filled differently before each: the same bytes."""
    c = case(name)
    g = c["g"]
    n_ws = mk._lib().maxk_gat_edge_softmax_backward_workspace_size(g.R, g.C, g.col.size, 0)
    for chunk in CHUNKS:
        runs = []
        for fill in (0x00, 0xFF, 0x5A):
            junk = [torch.full((n,), fill, dtype=torch.uint8, device=cuda)
                    for n in (n_ws, n_ws // 2, 4 * g.col.size, 4096)]
            del junk
            runs.append(run_all(mk, name, c, chunk))
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert M.same_bytes(a, b)


# ------------------------------------------------------------------------------- memory
@pytest.fixture(scope="module")
def arena(cuda):
    return M.Arena(8 << 20, cuda)


def _ops(mk, c, chunk):
    """name -> (op(dt, *tensors) -> outputs, input arrays, size query, output sizes)."""
    g = c["g"]
    E = g.col.size
    slope = c["slope"]
    w32, wp32 = ER.as_f32(c["f"].w), ER.as_f32(c["fp"].w)
    return {
        "plain-fwd": (lambda dt, lg: (mk.edge_softmax(dt[0], lg, chunk=chunk),),
                      ("lg",), "maxk_edge_softmax_workspace_size", [4 * E]),
        "plain-bwd": (lambda dt, w, gw: (mk.edge_softmax_backward(dt[0], w, gw, chunk=chunk),),
                      (wp32, "gw"), "maxk_edge_softmax_backward_workspace_size", [4 * E]),
        "gat-fwd": (lambda dt, sd, ss: (mk.gat_edge_softmax(dt[0], dt[1], sd, ss, slope,
                                                            chunk=chunk),),
                    ("s_dst", "s_src"), "maxk_gat_edge_softmax_workspace_size", [4 * E]),
        "gat-bwd": (lambda dt, sd, ss, w, gw: mk.gat_edge_softmax_backward(
            dt[0], dt[1], sd, ss, w, gw, slope, chunk=chunk),
            ("s_dst", "s_src", w32, "gw"), "maxk_gat_edge_softmax_backward_workspace_size",
            [4 * g.R, 4 * g.C]),
    }


@pytest.mark.parametrize("op_name", ["plain-fwd", "plain-bwd", "gat-fwd", "gat-bwd"])
def test_memory_contract(mk, arena, cuda, op_name):
    """Outputs and workspace from the poisoned, guarded arena (the workspace exactly the queried
    size): outputs fully written and the same bytes in every fill regime, guards untouched,
    inputs unchanged.  The transpose plan is built outside the arena, as a training loop's is."""
    c, p = case("S"), case("S", 0.2, 1e-3)
    g = c["g"]
    for chunk in CHUNKS:
        op, ins, query, out_bytes = _ops(mk, c, chunk)[op_name]

        def factory(primer):
            s = p if primer else c
            dt = (T(g.rp, DEV), T(g.col, DEV))
            mk.transpose_plan(dt[1], g.C)  # cached on this col tensor, outside the arena
            return (dt,) + tuple(T(s[a] if isinstance(a, str) else a, DEV) for a in ins)

        res = M.run_regimes(op, factory, arena)
        n_ws = getattr(mk._lib(), query)(g.R, g.C if "gat" in op_name else 0, g.col.size, chunk)
        assert sorted(a.nbytes for a in arena.allocs) == sorted(out_bytes + [n_ws])
        for regime in ("stale", "ones"):
            for a, b in zip(res["zero"], res[regime]):
                assert M.same_bytes(a, b), (op_name, regime)
        ref = {"plain-fwd": [(c["fp"].w, c["fp"].bound)],
               "plain-bwd": [(c["bp"].gl, c["bp"].gl_bound)],
               "gat-fwd": [(c["f"].w, c["f"].bound)],
               "gat-bwd": [(c["b"].g_dst, c["b"].g_dst_bound),
                           (c["b"].g_src, c["b"].g_src_bound)]}[op_name]
        for y, (r, b) in zip(res["ones"], ref):
            check(y, r, b, f"memguard {op_name} chunk {chunk}")


@pytest.mark.parametrize("op_name", ["plain-fwd", "plain-bwd", "gat-fwd", "gat-bwd"])
def test_undersized_workspace_is_rejected(mk, arena, monkeypatch, op_name):
    """A workspace one byte short of the size query: "workspace too small" from the host-side
    check, before any launch -- the outputs (0xFF-filled) are unchanged, the guards intact."""
    c = case("S")
    g = c["g"]
    op, ins, query, _ = _ops(mk, c, 0)[op_name]
    dt = (T(g.rp, DEV), T(g.col, DEV))
    mk.transpose_plan(dt[1], g.C)
    args = tuple(T(c[a] if isinstance(a, str) else a, DEV) for a in ins)
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
    """The GAT forward and backward captured into one graph on a side stream and replayed
    twice: both replays equal the eager result bitwise."""
    c = case("S")
    g = c["g"]
    rp, col = dev_graph("S")
    sd, ss, gw = T(c["s_dst"], cuda), T(c["s_src"], cuda), T(c["gw"], cuda)
    for chunk in CHUNKS:
        w = torch.empty(g.col.size, device=cuda)
        gd, gs = torch.empty(g.R, device=cuda), torch.empty(g.C, device=cuda)

        def both():
            mk.gat_edge_softmax(rp, col, sd, ss, 0.2, chunk=chunk, out=w, validate=False)
            mk.gat_edge_softmax_backward(rp, col, sd, ss, w, gw, 0.2, chunk=chunk, out=(gd, gs),
                                         validate=False)
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
        check(w, c["f"].w, c["f"].bound, f"captured chunk {chunk} w")


# ------------------------------------------------------------------------------- autograd
def test_autograd_through_the_aggregation(mk, cuda, monkeypatch):
    """GATEdgeSoftmax, then graph.aggregate(values=alpha), a random cotangent: s_dst.grad and
    s_src.grad against the float64 reference chained with edge_grad_ref (its bound carried
    through the softmax backward), topk_values.grad against the oracle with alpha as weights."""
    import maxk_layers as ML
    monkeypatch.setenv("MAXK_BWD_MODE", "csc")
    D, k = 64, 16
    c = case("S")
    g = c["g"]
    assert g.R == g.C
    rng = np.random.default_rng(515)
    ci = N.selectors(rng, g.C, D, k)
    cv = N.values(rng, (g.C, k), "unit")
    G = N.values(rng, (g.R, D), "unit")
    rp, col = dev_graph("S")
    graph_ = ML.CSRGraph(rp, col)
    sd = T(c["s_dst"], cuda).requires_grad_(True)
    ss = T(c["s_src"], cuda).requires_grad_(True)
    tv = T(cv, cuda).requires_grad_(True)
    alpha = ML.gat_edge_softmax(graph_, sd, ss, 0.2)
    check(alpha, c["f"].w, c["f"].bound, "autograd alpha")
    y = graph_.aggregate(tv, T(ci, cuda), D, values=alpha, row_div=None)
    y.backward(T(G, cuda))
    er = R.edge_grad_ref(g.rp, g.col, cv, ci, G, None)
    b = ER.backward(g.rp, g.col, c["f"], er.ref, 0.2, g.C, gw_bound=R.bound(er))
    check(sd.grad, b.g_dst, b.g_dst_bound, "autograd s_dst.grad")
    check(ss.grad, b.g_src, b.g_src_bound, "autograd s_src.grad")
    g2 = g._replace(ev=alpha.detach().cpu().numpy(), div=None)
    N.within(tv.grad, N.bwd_ref(g2, G, ci), N.bound_bwd(g2, G, ci), "autograd topk_values.grad")
    # the plain wrapper: the same logits give the same gradient of the logits
    lg = T(c["lg"], cuda).requires_grad_(True)
    wp = ML.edge_softmax(graph_, lg)
    wp.backward(T(c["gw"], cuda))
    check(lg.grad, c["bp"].gl, c["bp"].gl_bound, "autograd logits.grad")


# ------------------------------------------------------------------------------- the layer
def test_gat_conv_matches_dense(cuda):
    """MaxKGATConv on a 200-vertex graph, D = 64, k = 16, against a dense float64 restatement
    (masked dense softmax over the adjacency): the output, every parameter's gradient and both
    input gradients at rtol = atol = 1e-4, the tolerance of the layer tests."""
    import maxk_layers as ML
    torch.manual_seed(3)
    rng = np.random.default_rng(200)
    V, D, k, O_ = 200, 64, 16, 24
    rp, col = rand_graph(rng, V, 8, hubs=((7, 150),), empty=3)
    graph_ = ML.CSRGraph(T(rp.astype(np.int32), cuda), T(col.astype(np.int32), cuda))
    conv = ML.MaxKGATConv(D, O_, negative_slope=0.2).to(cuda)
    with torch.no_grad():
        conv.bias.normal_()
    x = torch.randn(V, D, device=cuda)
    xs, vals, idx = ML.maxk(x, k)
    xs = xs.detach().requires_grad_(True)
    vals = vals.detach().requires_grad_(True)
    out = conv(graph_, xs, vals, idx)
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
    h_s = xs2 @ Q["fc.weight"].t()
    e = torch.nn.functional.leaky_relu(
        (h_s @ Q["attn_dst"])[:, None] + (h_s @ Q["attn_src"])[None, :], 0.2)
    # a vertex without in-edges keeps its row unmasked (a finite softmax) and is zeroed by A
    masked = (A == 0) & (A.sum(1, keepdim=True) > 0)
    alpha = torch.softmax(e.masked_fill(masked, float("-inf")), 1) * A
    ref = alpha @ (xv @ Q["fc.weight"].t()) + Q["bias"]
    want = torch.autograd.grad(ref, [Q[n] for n in names] + [xs2, vals2], gout.double())
    torch.testing.assert_close(out, ref.float(), rtol=1e-4, atol=1e-4)
    for n, a, b in zip(names + ["x_sparse", "topk_values"], got, want):
        torch.testing.assert_close(a, b.float(), rtol=1e-4, atol=1e-4, msg=lambda m: f"{n}: {m}")
    assert not out[T(np.diff(rp) == 0, cuda)].sub(conv.bias).abs().max() > 0  # empty rows: bias


def test_ratios_are_reported():
    """Last in the file: the largest err/bound ratios seen, for the record."""
    for what, r in sorted(RATIOS.items(), key=lambda kv: -kv[1])[:10]:
        print(f"{r:.3f}  {what}")
    assert all(r <= 1.0 for r in RATIOS.values())
