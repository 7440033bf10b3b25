"""GPU: the partition geometry of the edge softmax (edge_softmax.hip) and of the edge-weight
gradient (edge_grad.hip), the two kinds of kernel that walk items cut at their end.

test_edge_softmax_gpu.py pins the values at item sizes 0, 64, 600 and 4096 on random graphs; this
file aims at where a row, a piece or an item ends.  The corner graph of tests/esm_corner_graph.py
(rows of 32 / 33 and 512 / 513 edges, a hub of 1700, empty rows first, in a run and last) and its
transpose (the same pointer array on the column side, for esm_colsum_kernel) run through all four
softmax entry points and mk.edge_weight_grad at every item size of EG.CHUNKS and at 0;
test_esm_corners_cpu.py asserts, without a GPU, that these (pointer array, item size) pairs hold
every corner class: whole rows and head / tail pieces of exactly those lengths, a row whose owner
holds none of it, a row ending on an item's last token, items with a head and a tail, with a head
and no row, of one empty row, and a row cut into single edges.

References and bounds are those of test_edge_softmax_gpu.py (tests/edge_softmax_ref.py through its
check_all: per-element bounds, rows summing to one, exact zeros for empty rows and an unread
column) and of test_edge_grad_gpu.py (tests/edge_grad_ref.py).  The degenerate shapes have one of
everything; the sweep at the end draws random graphs, item sizes, slopes and score magnitudes
(hypothesis, derandomized: every run draws the same cases).  The forward bound has no term for
the merge's expf and product per slot; at one token per item, where every edge of a cut row is a
slot, the largest err/bound measured is 0.15 (profiles/r11/esm_corners/), so none is added.

Which kernels: every non-empty softmax call launches all kernels of its form (esm_fwd_kernel<0/1>,
esm_merge_kernel<0>, esm_normalise_kernel; esm_bwd_kernel<0/1>, esm_merge_kernel<1>,
esm_bwd_emit_kernel<0/1>, and for GAT esm_merge_kernel<2> and esm_colsum_kernel);
edge_grad_kernel<8 / 16 / 32 / 64, 8, false> by k = 3 / 16 / 32 / 64.
"""
import functools

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import edge_grad_ref as R
import edge_softmax_ref as ER
import esm_corner_graph as EG
import memguard as M
import numerics as N
import test_edge_softmax_gpu as TG
from handout_graph import handout_csr
from test_fuzz_gpu import graph as fuzz_graph
from test_parity_gpu import T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CHUNKS = (0,) + EG.CHUNKS
TINY = (0, 1, 7)
D = 64
BY_CHUNK: dict = {}  # (softmax or edge grad, item size) -> the largest err/bound seen


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
        return _graph(*EG.corner_csr(), EG.NUM_COLS, EG.UNREAD, 1201)
    if name == "transpose":  # column 0: the corner graph's first row, which has no edge
        return _graph(*EG.corner_transpose(), EG.NUM_ROWS, 0, 1202)
    if name == "handout":
        rp, col = handout_csr()
        return _graph(rp, col, rp.size - 1, None, 1203)
    rp, col, C = EG.degenerate()[name]
    return _graph(rp, col, C, None, 1204)


@functools.lru_cache(maxsize=None)
def dev_graph(name):
    g = the_graph(name)
    return T(g.rp, DEV), T(g.col, DEV), T(g.div, DEV)


def softmax_case(g, slope, scale, seed):
    """TG.case for a graph of this file: inputs and float64 references, never modified."""
    rng = np.random.default_rng(seed)
    s_dst = (rng.standard_normal(g.R) * scale).astype(np.float32)
    s_src = (rng.standard_normal(g.C) * scale).astype(np.float32)
    gw = rng.standard_normal(g.col.size).astype(np.float32)
    f = ER.gat_forward(g.rp, g.col, s_dst, s_src, slope)
    lg = f.l.astype(np.float32)
    fp = ER.forward(g.rp, lg)
    return dict(g=g, s_dst=s_dst, s_src=s_src, gw=gw, slope=slope, f=f,
                b=ER.backward(g.rp, g.col, f, gw, slope, g.C), lg=lg, fp=fp,
                bp=ER.backward(g.rp, g.col, fp, gw))


@functools.lru_cache(maxsize=None)
def case(name, slope=0.2):
    return softmax_case(the_graph(name), slope, 1.0, 1300 + int(slope * 10) + len(name))


@functools.lru_cache(maxsize=None)
def grad_case(name, k):
    g = the_graph(name)
    rng = np.random.default_rng(1400 + k + len(name))
    ci = N.selectors(rng, g.C, D, k)
    cv = N.values(rng, (g.C, k), "unit")
    G = N.values(rng, (g.R, D), "unit")
    return dict(g=g, ci=ci, cv=cv, G=G, div=R.edge_grad_ref(g.rp, g.col, cv, ci, G, g.div),
                nodiv=R.edge_grad_ref(g.rp, g.col, cv, ci, G, None))


def noted(kind, chunk, r):
    BY_CHUNK[(kind, chunk)] = max(BY_CHUNK.get((kind, chunk), 0.0), r)


def run_softmax(mk, name, c, chunk):
    return TG.run_all(mk, name, c, chunk, dt=dev_graph(name)[:2])


def check_softmax(c, res, what, chunk):
    if c["g"].col.size == 0:  # nothing to compare per edge: both gradients are zeros
        w, gd, gs, wp, gl = res
        assert w.numel() == wp.numel() == gl.numel() == 0
        assert gd.shape == (c["g"].R,) and gs.shape == (c["g"].C,)
        assert not gd.any() and not gs.any()
        return
    TG.check_all(c, res, what)
    noted("softmax", chunk, max(v for key, v in TG.RATIOS.items() if key.startswith(what + " ")))


def run_grad(mk, name, gc, div, chunk):
    rp, col, dv = dev_graph(name)
    return mk.edge_weight_grad(rp, col, T(gc["cv"], DEV), T(gc["ci"], DEV), T(gc["G"], DEV),
                               row_div=dv if div else None, chunk=chunk)


def check_grad(y, er, what, chunk):
    assert y.dtype == torch.float32 and tuple(y.shape) == er.ref.shape
    r = N.within(y, er.ref, R.bound(er), what)
    print(f"{what}: err/bound {r:.3f}")
    noted("edge grad", chunk, r)


# ------------------------------------------------------------------------------- the corners
@pytest.mark.parametrize("slope", [0.2, 1.0])
@pytest.mark.parametrize("name", ["corner", "transpose"])
def test_corner_graph_softmax(mk, cuda, name, slope):
    c = case(name, slope)
    for chunk in CHUNKS:
        what = f"{name} slope {slope} chunk {chunk}"
        check_softmax(c, run_softmax(mk, name, c, chunk), what, chunk)


def test_corner_graph_minus_inf_pieces(mk, cuda):
    """The -Inf treatment of test_non_finite_classes_plain laid on the corners: 1150 edges of
    -Inf inside the hub (at every item size up to 513 at least one cut piece of nothing else:
    exactly 0, the row unharmed), the first 33-edge row all -Inf (all NaN), a NaN in the first
    32-edge row and a +Inf in the second (all NaN)."""
    c = case("corner")
    g = c["g"]
    deg = np.diff(g.rp)
    lg = c["lg"].copy()
    hb, he = int(g.rp[EG.HUB_ROW]), int(g.rp[EG.HUB_ROW + 1])
    a, b = hb + 100, hb + 1250
    lg[a:b] = -np.inf
    r33 = int(np.flatnonzero(deg == 33)[0])
    r32 = [int(r) for r in np.flatnonzero(deg == 32)]
    lg[g.rp[r33]:g.rp[r33 + 1]] = -np.inf
    lg[g.rp[r32[0]] + 31] = np.nan
    lg[g.rp[r32[1]]] = np.inf
    fp = ER.forward(g.rp, lg)
    bp = ER.backward(g.rp, g.col, fp, c["gw"])
    for r in (r33, r32[0], r32[1]):
        assert np.isnan(fp.w[g.rp[r]:g.rp[r + 1]]).all()
    assert (fp.w[a:b] == 0).all() and np.isfinite(fp.w[hb:he]).all()
    assert np.isnan(fp.w).sum() == 33 + 32 + 32
    for chunk in EG.CHUNKS:
        if chunk <= 513:  # a condition on the inputs: a piece of the hub inside the stretch
            cs = EG.census(g.rp, chunk)
            hub = (cs.row == EG.HUB_ROW) & (cs.se > cs.sb)
            assert (hub & (cs.sb >= a) & (cs.se <= b)).any(), chunk
    rp, _, _ = dev_graph("corner")
    for chunk in CHUNKS:
        wp = mk.edge_softmax(rp, T(lg, DEV), chunk=chunk)
        noted("softmax", chunk, TG.check(wp, fp.w, fp.bound, f"-inf corners chunk {chunk} w"))
        assert not wp[a:b].any()
        TG.check_rows_sum_to_one(wp, fp, g, f"-inf corners chunk {chunk}")
        gl = mk.edge_softmax_backward(rp, wp, T(c["gw"], DEV), chunk=chunk)
        noted("softmax", chunk,
              TG.check(gl, bp.gl, bp.gl_bound, f"-inf corners chunk {chunk} grad_logits"))


@pytest.mark.parametrize("k", [3, 16])
@pytest.mark.parametrize("name", ["corner", "transpose"])
def test_corner_graph_edge_grad(mk, cuda, name, k):
    gc = grad_case(name, k)
    for div in (True, False):
        for chunk in CHUNKS:
            y = run_grad(mk, name, gc, div, chunk)
            check_grad(y, gc["div" if div else "nodiv"],
                       f"{name} edge grad k{k} div={div} chunk {chunk}", chunk)


@pytest.mark.parametrize("k", [16, 32, 64])
def test_handout_graph_edge_grad(mk, cuda, k):
    """The hand-out graph of test_handout_gpu.py (a row with an item's last token, a hub ending
    on an item's end) at its two item sizes."""
    gc = grad_case("handout", k)
    for div in (True, False):
        for chunk in (512, 64):
            y = run_grad(mk, "handout", gc, div, chunk)
            check_grad(y, gc["div" if div else "nodiv"],
                       f"handout edge grad k{k} div={div} chunk {chunk}", chunk)


# ------------------------------------------------------------------------------- degenerate
@pytest.mark.parametrize("name", sorted(EG.degenerate()))
def test_degenerate_shapes(mk, cuda, name):
    c = case(name)
    g = c["g"]
    assert g.col.size in (600, 1, 300, 101)
    for chunk in TINY:
        check_softmax(c, run_softmax(mk, name, c, chunk), f"{name} chunk {chunk}", chunk)
        for k in (3, 16):
            gc = grad_case(name, k)
            for div in (True, False):
                check_grad(run_grad(mk, name, gc, div, chunk), gc["div" if div else "nodiv"],
                           f"{name} edge grad k{k} div={div} chunk {chunk}", chunk)


# ------------------------------------------------------------------------------- bitwise
@pytest.mark.parametrize("name", ["corner", "transpose"])
def test_bitwise_repeatable_at_tiny_items(mk, cuda, name):
    c, gc = case(name), grad_case(name, 16)
    for chunk in (1, 7):
        runs = [run_softmax(mk, name, c, chunk) + (run_grad(mk, name, gc, True, chunk),)
                for _ in range(2)]
        for a, b in zip(*runs):
            assert M.same_bytes(a, b), (name, chunk)


# ------------------------------------------------------------------------------- sweep
@st.composite
def sweeps(draw):
    V = draw(st.integers(1, 300))
    C = draw(st.integers(1, 300))
    avg = draw(st.floats(0.0, 40.0))
    hub = draw(st.booleans())
    dup = draw(st.booleans())
    empty = draw(st.sampled_from([False] * 9 + [True]))
    chunk = draw(st.sampled_from([0, 1, 2, 7, 31, 32, 33, 64, 513]))
    slope = draw(st.sampled_from([0.0, 0.2, 1.0]))
    scale = draw(st.sampled_from([1.0, 1e-3, 1e3]))
    k = draw(st.sampled_from([3, 16]))
    use_div = draw(st.booleans())
    seed = draw(st.integers(0, 2**31 - 1))
    return V, C, avg, hub, dup, empty, chunk, slope, scale, k, use_div, seed


SWEEP_EXAMPLES = 400


@settings(max_examples=SWEEP_EXAMPLES, deadline=None, derandomize=True, database=None,
          suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
@given(s=sweeps())
def test_random_graphs(mk, cuda, s):
    """R and C in 1..300, average degree 0..40, a hub of C or (with duplicate edges) 2 C edges,
    sometimes no edge at all: the four softmax calls and the edge gradient against the float64
    references with their derived bounds."""
    V, C, avg, hub, dup, empty, chunk, slope, scale, k, use_div, seed = s
    rng = np.random.default_rng(seed)
    rp, col = fuzz_graph(rng, V, C, 0.0 if empty else avg, hub and not empty, dup)
    g = _graph(rp, col, C, None, seed)
    c = softmax_case(g, slope, scale, seed + 1)
    dt = (T(g.rp, DEV), T(g.col, DEV))
    what = f"sweep V{V} C{C} E{col.size} slope {slope} scale {scale:g} chunk {chunk}"
    check_softmax(c, TG.run_all(mk, None, c, chunk, dt=dt), what, chunk)
    ci = N.selectors(rng, C, D, k)
    cv = N.values(rng, (C, k), "unit")
    G = N.values(rng, (V, D), "unit")
    y = mk.edge_weight_grad(dt[0], dt[1], T(cv, DEV), T(ci, DEV), T(G, DEV),
                            row_div=T(g.div, DEV) if use_div else None, chunk=chunk)
    er = R.edge_grad_ref(g.rp, g.col, cv, ci, G, g.div if use_div else None)
    check_grad(y, er, what + f" edge grad k{k}", chunk)


# ------------------------------------------------------------------------------- the record
def test_ratios_by_item_size():
    """Last in the file: the largest err/bound per item size, for the record."""
    for (kind, chunk), r in sorted(BY_CHUNK.items()):
        print(f"largest err/bound, {kind}, chunk {chunk}: {r:.3f}")
    assert all(r <= 1.0 for r in BY_CHUNK.values())
