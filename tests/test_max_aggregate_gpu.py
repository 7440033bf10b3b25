"""GPU: the max aggregation on CBSR features (spgemm_max.hip) through the binding
(mk.spgemm_max_forward, mk.spgemm_max_backward), the autograd function maxk_spgemm_max,
CSRGraph.aggregate_max and the layers MaxKSAGEConv(aggregator_type="pool") and
MaxKGINConv(aggregator_type="max"), against tests/max_aggregate_ref.py: the forward bitwise
(out's float bits and arg), the backward inside the reference's sum bound.

Which kernels.  The new kernels have no template instantiations: the lane-group width
KG = pow2ceil(k) (at most 64) is a run-time shift.  Every non-empty forward launches
cbsr_pack_kernel or cbsr_pack4_kernel (k % 4 == 0), max_fwd_kernel and max_fixup_kernel; a
forward without edges zero_words_kernel and fill_words_kernel; every non-empty backward
slot_row_kernel and max_bwd_kernel.  test_forward_bitwise and test_backward run KG = 4 (k = 3),
8 (k = 7, 8), 16, 32 (k = 24, 32) and 64 (k = 96: two slots per lane) at the auto item size and at
64 tokens, which cuts the hub rows of "S" and "Dn" into slabs (max_fixup_kernel's merge);
test_cut_rows runs every corner of the cut on "corner" and "transpose" from items of one token to
one item for the whole graph.  max_fwd_kernel with arg == NULL runs in test_want_arg_false and,
through the autograd function, in test_autograd; the no-edges kernels in
test_rectangular_and_empty.
"""
import functools

import numpy as np
import pytest
import torch

import esm_corner_graph as EG
import max_aggregate_ref as MR
import memguard as M
import numerics as N
import test_gat_attention_gpu as GA
from test_memguard_gpu import Shrunk
from test_parity_gpu import T, rand_graph

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CHUNKS = (0,) + EG.CHUNKS
SHAPES = [(3, 64), (8, 256), (16, 256), (32, 256), (24, 256), (96, 256), (7, 9)]
KINDS = ("unit", "ties")

the_graph = GA.the_graph    # "S", "Dn", "R" of test_numerics_gpu, "corner", "transpose"
dev_graph = GA.dev_graph


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


# ------------------------------------------------------------------------------- shared data
def make_data(g, k, D, kind, seed):
    """(ci, cv): random selectors; values of the "unit" regime with a random third negated --
    with few neighbours keeping a column, the implicit zero and explicit winners both occur --
    or ("ties") those quantised to {-1, 0, 1}.  Two outcomes need all of a row's keepers of a
    column to be negative, which random data give only to short rows (never on "Dn" and "R",
    whose rows have tens of edges), so no seed can provide them there; they are planted:
      * column 0 of every neighbour of the shortest non-empty row is kept and negative: an
        explicit negative winner in a row where every edge keeps the column;
      * column 1 of the neighbours of the shortest row of at least two edges is negative where
        kept, kept by the first and not by the last: the implicit zero beats negative candidates."""
    rng = np.random.default_rng(seed)
    ci = N.selectors(rng, g.C, D, k)
    cv = N.values(rng, (g.C, k), "unit")
    cv[rng.random(cv.shape) < 1 / 3] *= -1
    deg = np.diff(g.rp)

    def shortest(least):
        """The neighbours of the shortest row of at least `least` edges."""
        rows = np.flatnonzero(deg >= least)
        r = rows[np.argmin(deg[rows])]
        return g.col[g.rp[r]:g.rp[r + 1]]

    def slot_of(c, j, avoid):
        """The slot of vertex c that selects j, made to if none does (not one selecting avoid)."""
        at = np.flatnonzero(ci[c] == j)
        if at.size:
            return int(at[0])
        l = int(np.flatnonzero(ci[c] != avoid)[0])
        ci[c, l] = j
        return l

    for c in shortest(1):
        l = slot_of(c, 0, 1)
        cv[c, l] = -1 - abs(cv[c, l])
    nb = shortest(2)
    for c in nb:
        for l in np.flatnonzero(ci[c] == 1):
            cv[c, l] = -1 - abs(cv[c, l])
    l = slot_of(nb[0], 1, 0)
    cv[nb[0], l] = -1 - abs(cv[nb[0], l])
    for l in np.flatnonzero(ci[nb[-1]] == 1):  # the last neighbour keeps another column instead
        ci[nb[-1], l] = np.setdiff1d(np.arange(2, D), ci[nb[-1]])[0]
    if kind == "ties":
        cv = np.rint(np.clip(cv, -1, 1)).astype(np.float32)
    return ci, cv


def make_case(name, k, D, kind="unit", ci=None, cv=None):
    g = the_graph(name)
    if ci is None:
        ci, cv = make_data(g, k, D, kind, 2300 + 31 * k + D)
    out, arg = MR.forward(g.rp, g.col, cv, ci, D)
    return dict(g=g, ci=ci, cv=cv, out=out, arg=arg, D=D, k=k, name=name)


@functools.lru_cache(maxsize=None)
def case(name, k=16, D=256, kind="unit"):
    """The cases several tests share: computed once, never modified."""
    return make_case(name, k, D, kind)


def run(mk, c, chunk=0, cv=None, **kw):
    rp, col = dev_graph(c["name"])
    return mk.spgemm_max_forward(rp, col, T(c["cv"] if cv is None else cv, DEV), T(c["ci"], DEV),
                                 c["D"], chunk=chunk, **kw)


def same_out(y, ref):
    """The float bits of y equal the reference's; a NaN matches any NaN."""
    assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape
    y = y.cpu().numpy()
    nan = np.isnan(ref)
    return np.array_equal(np.isnan(y), nan) and np.array_equal(
        np.where(nan, 0, y.view(np.uint32)), np.where(nan, 0, ref.view(np.uint32)))


def check_forward(c, out, arg, what):
    assert same_out(out, c["out"]), what
    if arg is not None:
        assert arg.dtype == torch.int32
        assert np.array_equal(arg.cpu().numpy(), c["arg"]), what


# ------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("k,D", SHAPES, ids=[f"k{k}-D{D}" for k, D in SHAPES])
@pytest.mark.parametrize("name", ["S", "Dn", "R"])
def test_forward_bitwise(mk, cuda, name, k, D):
    """out's bits and arg equal the reference's at the auto item size and at 64 tokens, on random
    values and on values quantised to {-1, 0, 1} (ties everywhere); the three outcomes occur."""
    for kind in KINDS:
        c = make_case(name, k, D, kind)
        g = c["g"]
        pos, imp, neg = MR.outcomes(g.rp, g.col, c["cv"], c["ci"], D, c["out"], c["arg"])
        print(f"{name} k{k} D{D} {kind}: explicit positive {pos}, implicit zero over negatives "
              f"{imp}, explicit negative with every edge keeping {neg}")
        assert pos > 0 and imp > 0 and neg > 0
        if kind == "ties":
            assert (c["cv"] == 0).any() and set(np.unique(c["cv"])) <= {-1.0, 0.0, 1.0}
        for chunk in (0, 64):
            out, arg = run(mk, c, chunk)
            check_forward(c, out, arg, f"{name} k{k} D{D} {kind} chunk {chunk}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["corner", "transpose"])
def test_cut_rows(mk, cuda, name, kind):
    """Rows of 32 / 33 and 512 / 513 edges, the hub of 1700, empty rows first, in a run and last,
    at the auto item size and every entry of EG.CHUNKS (1 token to more than the graph)."""
    c = case(name, 16, 256, kind)
    g = c["g"]
    pos, imp, neg = MR.outcomes(g.rp, g.col, c["cv"], c["ci"], 256, c["out"], c["arg"])
    assert pos > 0 and imp > 0 and neg > 0
    for chunk in CHUNKS:
        out, arg = run(mk, c, chunk)
        check_forward(c, out, arg, f"{name} {kind} chunk {chunk}")


@pytest.mark.parametrize("name,k,D", [("corner", 16, 256), ("S", 24, 256), ("corner", 7, 9)])
def test_chunk_independence(mk, cuda, name, k, D):
    """out and arg are the same bytes at every item size, and in two runs whose workspaces come
    from allocator blocks filled with 0x00 and with 0xFF."""
    c = case(name, k, D, "ties")
    g = c["g"]
    base = run(mk, c, 0)
    for chunk in CHUNKS:
        n_ws = mk._lib().maxk_spgemm_max_forward_workspace_size(g.R, g.C, g.col.size, D, k, chunk)
        for fill in (0x00, 0xFF):
            junk = [torch.full((n,), fill, dtype=torch.uint8, device=cuda)
                    for n in (n_ws, n_ws // 2, 4 * g.R * D, 4096)]
            del junk
            out, arg = run(mk, c, chunk)
            assert M.same_bytes(out, base[0]) and M.same_bytes(arg, base[1]), (chunk, fill)
    check_forward(c, *base, f"{name} k{k} D{D}")


@pytest.mark.parametrize("name", ["corner", "S"])
def test_want_arg_false(mk, cuda, name):
    c = case(name)
    for chunk in (0, 64):
        out, arg = run(mk, c, chunk, want_arg=False)
        assert arg is None
        check_forward(c, out, None, f"{name} no arg chunk {chunk}")


def test_rectangular_and_empty(mk, cuda):
    """num_rows != num_cols both ways; num_e == 0, a graph of only empty rows: zeros and -1."""
    rng = np.random.default_rng(2900)
    for R, C, avg in ((90, 17, 6), (17, 300, 40)):
        rp, col = rand_graph(rng, R, avg, cols=C, empty=2)
        g = N.make_graph(rng, rp, col, C)
        ci, cv = make_data(g, 5, 24, "unit", 2901 + R)
        want = MR.forward(g.rp, g.col, cv, ci, 24)
        for chunk in (0, 64, 7):
            out, arg = mk.spgemm_max_forward(T(g.rp, cuda), T(g.col, cuda), T(cv, cuda),
                                             T(ci, cuda), 24, chunk=chunk)
            assert same_out(out, want[0]) and np.array_equal(arg.cpu().numpy(), want[1])
    rows, cols, D, k = 40, 17, 64, 8
    rp = torch.zeros(rows + 1, dtype=torch.int32, device=cuda)
    col = torch.empty(0, dtype=torch.int32, device=cuda)
    cv = torch.randn(cols, k, device=cuda)
    ci = torch.zeros(cols, k, dtype=torch.uint8, device=cuda)
    for want_arg in (True, False):
        out, arg = mk.spgemm_max_forward(rp, col, cv, ci, D, want_arg=want_arg)
        assert tuple(out.shape) == (rows, D) and not out.view(torch.int32).any()
        assert (arg is None) if not want_arg else bool((arg == -1).all())
    arg = torch.full((rows, D), -1, dtype=torch.int32, device=cuda)
    g = mk.spgemm_max_backward(rp, col, ci, arg, torch.randn(rows, D, device=cuda), k)
    assert tuple(g.shape) == (cols, k) and not g.view(torch.int32).any()


def test_non_finite(mk, cuda):
    """NaN, +Inf, -Inf and -0.0 laid into values that the hub row and short rows read, against
    the reference's bits (NaN-ness, not payload), inside an item and on the cut hub row (chunk
    64); a NaN behind a selector past D and in the vertex no edge reads reaches nothing."""
    base = case("S", 16, 100)
    g = base["g"]
    cv, ci = base["cv"].copy(), base["ci"].copy()
    hubcols = g.col[g.rp[g.hub]:g.rp[g.hub + 1]]
    deg = np.diff(g.rp)
    short = [int(r) for r in np.flatnonzero((deg >= 2) & (deg <= 6)) if r != g.hub]
    spots = [int(hubcols[i]) for i in (3, 50, 120, 300, 500, 580)] + \
            [int(g.col[g.rp[r] + (i % 2)]) for i, r in enumerate(short[:6])]
    for i, c_ in enumerate(spots):
        cv[c_, i % 16] = (np.nan, np.inf, -np.inf, -0.0, np.nan, -0.0)[i % 6]
        if i % 6 == 4:  # a second NaN in the same vertex, negative quiet
            cv.view(np.uint32)[c_, (i + 5) % 16] = 0xFFC00000
    # a whole short row of -Inf and one of -0.0 in column 1: every edge keeps it
    whole = [r for r in short[6:]
             if not np.isin(g.col[g.rp[r]:g.rp[r + 1]], spots).any()][:2]
    assert len(whole) == 2
    for r, v in zip(whole, (-np.inf, -0.0)):
        for c_ in g.col[g.rp[r]:g.rp[r + 1]]:
            at = np.flatnonzero(ci[c_] == 1)
            l = int(at[0]) if at.size else 0
            ci[c_, l], cv[c_, l] = 1, v
    ci[spots[0], 7] = 200  # past D = 100
    cv[spots[0], 7] = np.nan
    cv[g.unread] = np.nan
    c = make_case("S", 16, 100, ci=ci, cv=cv)
    ref = c["out"]
    assert np.isnan(ref).any() and np.isposinf(ref).any() and np.isneginf(ref).any()
    assert (ref.view(np.uint32) == 0x80000000).any()
    assert np.isnan(ref[g.hub]).any() and np.isposinf(ref[g.hub]).any()
    assert np.isneginf(ref[whole[0]]).any() and np.isfinite(ref).mean() > 0.9
    for chunk in (0, 64):
        out, arg = run(mk, c, chunk, validate=False)
        check_forward(c, out, arg, f"non-finite chunk {chunk}")


# ------------------------------------------------------------------------------- backward
def backward_case(c, seed):
    """G with NaN wherever the implicit zero or nothing won (it must reach nothing) and at a few
    winners (it reaches the winner's slots alone); the float64 reference and its bound."""
    g = c["g"]
    rng = np.random.default_rng(seed)
    G = N.values(rng, (g.R, c["D"]), "unit")
    G[c["arg"] < 0] = np.nan
    won = np.argwhere(c["arg"] >= 0)
    for i in rng.choice(len(won), 5, replace=False):
        G[tuple(won[i])] = np.nan
    return G, MR.backward(g.rp, g.col, c["ci"], c["arg"], G)


def run_backward(mk, c, G, arg=None):
    rp, col = dev_graph(c["name"])
    return mk.spgemm_max_backward(rp, col, T(c["ci"], DEV), T(c["arg"] if arg is None else arg, DEV),
                                  T(G, DEV), c["k"])


def check_backward(c, got, b, what):
    assert got.dtype == torch.float32 and tuple(got.shape) == b.grad.shape
    r = N.within(got, b.grad, b.bound, what)  # the NaN masks equal the reference's
    print(f"{what}: err/bound {r:.3f}")
    assert not got[T(b.n == 0, DEV)].view(torch.int32).any()  # exact +0.0
    return r


@pytest.mark.parametrize("k,D", SHAPES, ids=[f"k{k}-D{D}" for k, D in SHAPES])
@pytest.mark.parametrize("name", ["S", "Dn", "R"])
def test_backward(mk, cuda, name, k, D):
    """grad_cbsr inside the reference's bound from the reference's arg; exact zeros for a slot
    that never won, the unread column and the -1 winners, whose grad_out is NaN; two runs give the
    same bytes."""
    c = make_case(name, k, D, "ties")  # ties: the gradient must follow arg, not the values
    G, b = backward_case(c, 3100 + k)
    g = c["g"]
    assert (b.n[g.unread] == 0).all() and (b.n == 0).any() and (b.n > 1).any()
    got = run_backward(mk, c, G)
    check_backward(c, got, b, f"backward {name} k{k} D{D}")
    assert M.same_bytes(got, run_backward(mk, c, G))


@pytest.mark.parametrize("name", ["corner", "transpose"])
def test_backward_from_the_kernel_arg(mk, cuda, name):
    """The forward's own arg fed to the backward, on the graphs with hub rows and hub columns."""
    c = case(name, 16, 256, "unit")
    G, b = backward_case(c, 3200)
    for chunk in (0, 64):
        _, arg = run(mk, c, chunk)
        rp, col = dev_graph(name)
        got = mk.spgemm_max_backward(rp, col, T(c["ci"], DEV), arg, T(G, DEV), 16)
        check_backward(c, got, b, f"backward {name} from the forward at chunk {chunk}")


def test_backward_repeated_and_skipped_selectors(mk, cuda):
    """A quarter of the vertices repeat a selector -- both slots receive the winner's gradient --
    and selectors run past D = 100: those slots are exactly 0."""
    g = the_graph("S")
    k, D = 16, 100
    rng = np.random.default_rng(3300)
    ci = N.selectors(rng, g.C, 256, k)
    dup = rng.choice(g.C, g.C // 4, replace=False)
    ci[dup, k - 1] = ci[dup, 0]
    cv = N.values(rng, (g.C, k), "unit")
    c = make_case("S", k, D, ci=ci, cv=cv)
    out, arg = run(mk, c, 64, validate=False)
    check_forward(c, out, arg, "repeated selectors forward")
    G, b = backward_case(c, 3301)
    got = run_backward(mk, c, G)
    check_backward(c, got, b, "repeated selectors backward")
    assert (b.n[ci >= D] == 0).all() and (ci >= D).any()
    both = dup[(ci[dup, 0] < D) & (b.n[dup, 0] > 0)]
    assert both.size and M.same_bytes(got[T(both, cuda), 0], got[T(both, cuda), k - 1])


# ------------------------------------------------------------------------------- memory
@pytest.fixture(scope="module")
def arena(cuda):
    return M.Arena(24 << 20, cuda)


@pytest.mark.parametrize("k,D", [(16, 256), (3, 64)])
def test_memory_contract(mk, arena, cuda, k, D):
    """Outputs and workspaces from the poisoned, guarded arena (the workspace exactly the queried
    size): outputs fully written and the same bytes in every fill regime, guards untouched,
    inputs unchanged; forward, then backward."""
    c = case("corner", k, D, "ties")
    g = c["g"]
    E = g.col.size
    G, b = backward_case(c, 3400)
    for chunk in (0, 64):
        def factory(primer):
            dt = (T(g.rp, DEV), T(g.col, DEV))
            cv, ci = T(c["cv"], DEV), T(c["ci"], DEV)
            if primer:
                cv = torch.rand(cv.shape, generator=torch.Generator(device=DEV).manual_seed(5),
                                device=DEV)
            return dt, cv, ci

        def op(dt, cv, ci):
            return mk.spgemm_max_forward(dt[0], dt[1], cv, ci, D, chunk=chunk)

        res = M.run_regimes(op, factory, arena)
        n_ws = mk._lib().maxk_spgemm_max_forward_workspace_size(g.R, g.C, E, D, k, chunk)
        assert sorted(x.nbytes for x in arena.allocs) == sorted([4 * g.R * D, 4 * g.R * D, n_ws])
        for regime in ("stale", "ones"):
            for x, y in zip(res["zero"], res[regime]):
                assert M.same_bytes(x, y), regime
        check_forward(c, *res["ones"], f"memguard k{k} D{D} chunk {chunk}")

    def factory_bwd(primer):
        dt = (T(g.rp, DEV), T(g.col, DEV))
        plan = mk.transpose_plan(dt[1], g.C, cache=False)
        Gt = T(G, DEV)
        if primer:
            Gt = torch.rand_like(Gt)
        return dt, plan, T(c["ci"], DEV), T(c["arg"], DEV), Gt

    def op_bwd(dt, plan, ci, arg, Gt):
        return (mk.spgemm_max_backward(dt[0], dt[1], ci, arg, Gt, k, plan=plan),)

    res = M.run_regimes(op_bwd, factory_bwd, arena)
    n_ws = mk._lib().maxk_spgemm_max_backward_workspace_size(g.R, g.C, E, D, k)
    assert sorted(x.nbytes for x in arena.allocs) == sorted([4 * g.C * k, n_ws])
    for regime in ("stale", "ones"):
        assert M.same_bytes(res["zero"][0], res[regime][0]), regime
    check_backward(c, res["ones"][0], b, f"memguard backward k{k} D{D}")


@pytest.mark.parametrize("entry", ["forward", "backward"])
def test_undersized_workspace_is_rejected(mk, arena, monkeypatch, entry):
    """A workspace one byte short of the size query: "workspace too small" from the host-side
    check, before any launch -- the outputs (0xFF-filled) are unchanged, the guards intact."""
    c = case("corner", 16, 256, "ties")
    g = c["g"]
    dt = (T(g.rp, DEV), T(g.col, DEV))
    cv, ci, arg = T(c["cv"], DEV), T(c["ci"], DEV), T(c["arg"], DEV)
    G = torch.zeros(g.R, 256, device=DEV)
    plan = mk.transpose_plan(dt[1], g.C, cache=False)
    torch.cuda.synchronize()
    shrunk = Shrunk(mk._L, f"maxk_spgemm_max_{entry}_workspace_size")
    monkeypatch.setattr(mk, "_L", shrunk)
    with arena.active("ones"):
        with pytest.raises(RuntimeError, match="workspace too small"):
            if entry == "forward":
                mk.spgemm_max_forward(dt[0], dt[1], cv, ci, 256)
            else:
                mk.spgemm_max_backward(dt[0], dt[1], ci, arg, G, 16, plan=plan)
        made = len(arena.allocs)
    assert shrunk.sizes and all(n > 1 for n in shrunk.sizes), shrunk.sizes
    assert made >= 2  # the outputs and the short workspace came from the arena
    arena.check()
    assert arena.untouched()


# ------------------------------------------------------------------------------- autograd
def dense_amax(rp, col, X):
    """[R, D] on X's device: amax over each row's neighbours of X [C, D], 0 for an empty row."""
    R = rp.size - 1
    A = torch.zeros(R, X.shape[0], dtype=torch.bool, device=X.device)
    rows = np.repeat(np.arange(R), np.diff(rp))
    A[T(rows, X.device), T(col.astype(np.int64), X.device)] = True
    m = X[None].expand(R, -1, -1).masked_fill(~A[:, :, None], float("-inf")).amax(1)
    return torch.where(A.any(1)[:, None], m, torch.zeros_like(m))


def test_autograd(mk, cuda, monkeypatch):
    """maxk_spgemm_max on tie-free random values against dense float64 torch (amax of the masked
    gather): the value exact after casting, the gradient of topk_values inside the sum bound; it
    saves arg and topk_indices and no other activation; without a gradient to compute it asks the
    kernel for no winners."""
    import maxk_spgemm_function as MF
    D, k = 64, 16
    c = case("S", k, D, "unit")
    g = c["g"]
    rp, col = dev_graph("S")
    tv, ci = T(c["cv"], cuda).requires_grad_(True), T(c["ci"], cuda)
    calls = []
    real = mk.spgemm_max_forward
    monkeypatch.setattr(mk, "spgemm_max_forward",
                        lambda *a, **kw: calls.append(kw.get("want_arg")) or real(*a, **kw))
    sizes = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: sizes.append(t.numel()) or t,
                                                  lambda t: t):
        y = MF.maxk_spgemm_max(rp, col, tv, ci, D)
    assert sorted(sizes) == sorted([g.R * D, g.C * k]) and calls == [True]
    G = N.values(np.random.default_rng(3500), (g.R, D), "unit")
    y.backward(T(G, cuda))
    tv64 = T(c["cv"].astype(np.float64), cuda).requires_grad_(True)
    X = torch.zeros(g.C, D, dtype=torch.float64, device=cuda).scatter(1, ci.long(), tv64)
    want = dense_amax(g.rp, g.col, X)
    want.backward(T(G.astype(np.float64), cuda))
    assert torch.equal(y.detach().double(), want.detach())
    b = MR.backward(g.rp, g.col, c["ci"], c["arg"], G)
    assert np.abs(b.grad - tv64.grad.cpu().numpy()).max() <= 1e-12 * np.abs(b.grad).max()
    check_backward(c, tv.grad, b._replace(grad=tv64.grad.cpu().numpy()), "autograd topk_values.grad")
    # no gradient wanted: no grad mode, and an input that does not require one
    with torch.no_grad():
        y2 = MF.maxk_spgemm_max(rp, col, tv, ci, D)
    y3 = MF.maxk_spgemm_max(rp, col, tv.detach(), ci, D)
    assert calls == [True, False, False]
    assert M.same_bytes(y2, y.detach()) and M.same_bytes(y3, y.detach())
    assert not y3.requires_grad


# ------------------------------------------------------------------------------- layers
def layer_problem(cuda):
    import maxk_layers as ML
    g = the_graph("S")
    rp, col = dev_graph("S")
    graph_ = ML.CSRGraph(rp, col)
    torch.manual_seed(11)
    x = torch.randn(g.R, 64, device=cuda)
    xs, vals, idx = ML.maxk(x, 16)
    return ML, g, graph_, xs.detach(), vals.detach(), idx


def test_sage_pool_matches_dense(cuda):
    """MaxKSAGEConv(aggregator_type="pool") against the same layer in dense float64 torch --
    fc_pool, the MaxK mask the layer selected, amax over the neighbours, fc_self + fc_neigh --
    in the output, every parameter's gradient and the input's, at rtol = atol = 1e-4."""
    ML, g, graph_, xs, vals, idx = layer_problem(cuda)
    torch.manual_seed(12)
    conv = ML.MaxKSAGEConv(64, 24, aggregator_type="pool", pool_k=8).to(cuda)
    with torch.no_grad():
        conv.fc_pool.bias.normal_()
        conv.fc_self.bias.normal_()
    xs = xs.requires_grad_(True)
    out = conv(graph_, xs, vals, idx)
    gout = torch.randn_like(out)
    names = [n for n, _ in conv.named_parameters()]
    assert sorted(names) == sorted(["fc_neigh.weight", "fc_self.weight", "fc_self.bias",
                                    "fc_pool.weight", "fc_pool.bias"])
    got = torch.autograd.grad(out, [p for _, p in conv.named_parameters()] + [xs], gout)
    Q = {n: p.detach().double().requires_grad_(True) for n, p in conv.named_parameters()}
    x2 = xs.detach().double().requires_grad_(True)
    p = x2 @ Q["fc_pool.weight"].t() + Q["fc_pool.bias"]
    _, _, pi = ML.maxk(conv.fc_pool(xs.detach()), 8)
    mask = torch.zeros_like(p).scatter(1, pi.long(), 1.0)
    agg = dense_amax(g.rp, g.col, p * mask)
    ref = x2 @ Q["fc_self.weight"].t() + Q["fc_self.bias"] + agg @ Q["fc_neigh.weight"].t()
    want = torch.autograd.grad(ref, [Q[n] for n in names] + [x2], gout.double())
    torch.testing.assert_close(out, ref.float(), rtol=1e-4, atol=1e-4)
    for n, a, b_ in zip(names + ["x_sparse"], got, want):
        torch.testing.assert_close(a, b_.float(), rtol=1e-4, atol=1e-4,
                                   msg=lambda m: f"{n}: {m}")
    assert got[names.index("fc_pool.weight")].abs().max() > 0


def test_gin_max_matches_dense(cuda):
    """MaxKGINConv(aggregator_type="max") against (1 + eps) x + amax over the neighbours of the
    scattered CBSR through the same apply_func, in the output and all gradients."""
    ML, g, graph_, xs, vals, idx = layer_problem(cuda)
    torch.manual_seed(13)
    conv = ML.MaxKGINConv(torch.nn.Linear(64, 24), init_eps=0.25, learn_eps=True,
                          aggregator_type="max").to(cuda)
    x = xs.requires_grad_(True)
    tv = vals.requires_grad_(True)
    out = conv(graph_, x, tv, idx)
    gout = torch.randn_like(out)
    names = [n for n, _ in conv.named_parameters()]
    got = torch.autograd.grad(out, [p for _, p in conv.named_parameters()] + [x, tv], gout)
    Q = {n: p.detach().double().requires_grad_(True) for n, p in conv.named_parameters()}
    x2 = x.detach().double().requires_grad_(True)
    tv2 = tv.detach().double().requires_grad_(True)
    X = torch.zeros(g.C, 64, dtype=torch.float64, device=cuda).scatter(1, idx.long(), tv2)
    h = (1 + Q["eps"]) * x2 + dense_amax(g.rp, g.col, X)
    ref = h @ Q["apply_func.weight"].t() + Q["apply_func.bias"]
    want = torch.autograd.grad(ref, [Q[n] for n in names] + [x2, tv2], gout.double())
    torch.testing.assert_close(out, ref.float(), rtol=1e-4, atol=1e-4)
    for n, a, b_ in zip(names + ["x", "topk_values"], got, want):
        torch.testing.assert_close(a, b_.float(), rtol=1e-4, atol=1e-4,
                                   msg=lambda m: f"{n}: {m}")


def test_mean_and_sum_layers_keep_their_bytes(cuda):
    """aggregator_type="mean" / "sum" are the layers as they were: for the same seed the same
    parameters, and the output bytes of the composition the layers ran before the argument
    existed (aggregate with the in-degrees as divisor through linear(); (1 + eps) x + aggregate)."""
    ML, g, graph_, xs, vals, idx = layer_problem(cuda)
    outs = []
    for kw in ({}, {"aggregator_type": "mean"}):
        torch.manual_seed(14)
        conv = ML.MaxKSAGEConv(64, 24, **kw).to(cuda)
        outs.append(conv(graph_, xs, vals, idx).detach())
    agg = graph_.aggregate(vals, idx, 64, row_div=graph_.clamped("in_degrees"))
    outs.append(ML.linear(xs, conv.fc_self, agg, conv.fc_neigh).detach())
    assert M.same_bytes(outs[0], outs[1]) and M.same_bytes(outs[0], outs[2])
    outs = []
    for kw in ({}, {"aggregator_type": "sum"}):
        torch.manual_seed(15)
        conv = ML.MaxKGINConv(torch.nn.Linear(64, 24), init_eps=0.5, **kw).to(cuda)
        outs.append(conv(graph_, xs, vals, idx).detach())
    outs.append(conv.apply_func((1 + conv.eps) * xs + graph_.aggregate(vals, idx, 64)).detach())
    assert M.same_bytes(outs[0], outs[1]) and M.same_bytes(outs[0], outs[2])
