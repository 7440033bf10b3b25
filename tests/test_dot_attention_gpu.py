"""GPU: the fused multi-head dot-product attention on CBSR keys (dot_attention_heads.hip) through
the binding (mk.dot_attention_heads, mk.dot_edge_alpha_heads), the autograd functions
MaxKDotScoresHeadsFunction and MaxKDotAttentionHeadsFunction and MaxKTransformerConv, against
tests/dot_attention_ref.py (float64, with its derived bounds), against the composition it replaces
(mk.edge_weight_grad_heads, the scale, mk.edge_softmax per head, mk.spgemm_forward_heads) and
against dense float64 torch autograd.

Which kernels.  Every non-empty forward launches cbsr_pack_kernel or cbsr_pack4_kernel
(k % 4 == 0), dath_fwd_kernel<KG, 8> and softmax_fixup_kernel<false> (heads_walk.h, which also
holds the walk the forward kernel shares with the other heads forwards); every non-empty alpha
call the pack and dath_alpha_kernel<KG, 8>.  KG = 8 for k = 3, 7, 8, 16 for k = 16, 32 for k = 24, 32, 64 for
k = 96 (k > KG: the several-slots-per-lane path of record_dots and walk_dot).  The heads per pass
are HC = ceil(H / ceil(H / G)), G = 64 / KG: at H = 1, 2, 3, 5, 8 that is 1, 2, 3, 5, 8 (KG = 8),
1, 2, 3, 3, 4 (KG = 16), 1, 2, 2, 2, 2 (KG = 32) and 1 (KG = 64), so test_parity, which runs
every (k, H) of SHAPES x HEADS at the auto item size and at 64 tokens, reaches the four
dath_fwd_kernel instantiations with one and several passes, full and partly filled last passes
and idle groups (H = 3 at G = 8).  test_alpha_from_the_statistics runs k = 16 and, by
test_parity's shapes in test_alpha_shapes, every KG of dath_alpha_kernel.  The NaN pass of
dath_fwd_kernel (walk_dot<.., true>) and of softmax_fixup_kernel run in test_non_finite (rows inside
an item and the hub row at chunk 64).

The largest err / bound seen on an MI355X is in test_ratios_are_reported's output; the figures of
the first run are recorded in profiles/r18/dot_attention/README.md.
"""
import functools
import types

import numpy as np
import pytest
import torch

import dot_attention_ref as DR
import edge_grad_ref as R
import edge_softmax_ref as ER
import esm_corner_graph as EG
import memguard as M
import numerics as N
import test_dot_attention_cpu as DC
import test_edge_softmax_gpu as TG
import test_gat_attention_gpu as GA
from test_memguard_gpu import Shrunk
from test_parity_gpu import T, rand_graph

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CHUNKS = (0,) + EG.CHUNKS
HEADS = (1, 2, 3, 5, 8)
HMAX = 8
SCALES = (1.0, 0.125)
SHAPES = [(3, 64), (8, 256), (16, 256), (32, 256), (24, 256), (96, 256), (7, 9)]
RATIOS: dict = {}

the_graph = GA.the_graph    # "S", "Dn", "R" of test_numerics_gpu, "corner", "transpose"
dev_graph = GA.dev_graph


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


# ------------------------------------------------------------------------------- shared data
def make_case(name, k, D, scale=1.0, seed=0, q=None, ci=None):
    """HMAX heads of queries, a CBSR and the float64 reference; H heads are the first H."""
    g = the_graph(name)
    rng = np.random.default_rng(1800 + 31 * k + D + seed)
    if q is None:
        q = rng.standard_normal((HMAX, g.R, D)).astype(np.float32)
    ci = N.selectors(rng, g.C, D, k) if ci is None else ci
    cv = N.values(rng, (g.C, k), "unit")
    n = N.count_fwd(g, ci, D)
    a = DR.attention(g.rp, g.col, q, scale, cv, ci, D, n)
    return dict(g=g, q=q, ci=ci, cv=cv, n=n, a=a, D=D, k=k, scale=scale)


@functools.lru_cache(maxsize=None)
def case(name, k=16, D=256, scale=0.125):
    """The cases several tests share: computed once, never modified."""
    return make_case(name, k, D, scale)


def dev_case(c, H, q=None):
    return (T(np.ascontiguousarray((c["q"] if q is None else q)[:H]), DEV), T(c["cv"], DEV),
            T(c["ci"], DEV))


def run(mk, name, ops, c, chunk, dt=None, **kw):
    rp, col = dev_graph(name) if dt is None else dt
    q, cv, ci = ops
    return mk.dot_attention_heads(rp, col, q, cv, ci, c["D"], c["scale"], chunk=chunk, **kw)


def alpha(mk, name, ops, c, m, z, chunk=0, dt=None, **kw):
    rp, col = dev_graph(name) if dt is None else dt
    q, cv, ci = ops
    return mk.dot_edge_alpha_heads(rp, col, q, cv, ci, c["D"], c["scale"], m, z, chunk=chunk,
                                   **kw)


def check(y, ref, bound, what):
    assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape, (y.shape, ref.shape)
    r = N.within(y, ref, bound, what)
    RATIOS[what] = r
    print(f"{what}: err/bound {r:.3f}")
    return r


def check_all(c, H, res, what):
    """out and both statistics inside their bounds; exact zeros where nothing is added."""
    g, a = c["g"], DR.heads_slice(c["a"], H)
    out, m, z = res
    check(out, a.out, a.out_bound, f"{what} out")
    check(m, a.m, a.m_bound, f"{what} row_max")
    check(z, a.z, a.z_bound, f"{what} row_sum")
    empty = T(np.diff(g.rp) == 0, DEV)
    assert not out[:, empty].any() and not m[:, empty].any() and not z[:, empty].any()
    assert not out[:, T(c["n"] == 0, DEV)].any()  # a column no edge of the row selects


def check_alpha(c, H, w, what):
    """w inside the weight bound, every row summing to one inside the sum of its bounds."""
    g, a = c["g"], DR.heads_slice(c["a"], H)
    check(w, a.w, a.w_bound, what)
    for h in range(H):
        TG.check_rows_sum_to_one(w[h], a.heads[h]._replace(bound=a.w_bound[h]), g,
                                 f"{what} head {h}")


# ------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("k,D", SHAPES, ids=[f"k{k}-D{D}" for k, D in SHAPES])
@pytest.mark.parametrize("name", ["S", "Dn", "R"])
def test_parity(mk, cuda, name, k, D, scale):
    """out, row_max and row_sum inside the derived bounds for H in 1, 2, 3, 5, 8 at the auto item
    size and at 64 tokens.  Every dath_fwd_kernel instantiation and pass shape (see the module
    text)."""
    c = make_case(name, k, D, scale)
    for H in HEADS:
        ops = dev_case(c, H)
        for chunk in (0, 64):
            check_all(c, H, run(mk, name, ops, c, chunk),
                      f"{name} k{k} D{D} s{scale} H{H} chunk {chunk}")


# ------------------------------------------------------------------------------- cut rows
@pytest.mark.parametrize("H", [3, 8])
@pytest.mark.parametrize("name", ["corner", "transpose"])
def test_cut_rows(mk, cuda, name, H):
    """Rows of 32 / 33 and 512 / 513 edges, the hub of 1700, empty rows first, in a run and last,
    at the auto item size and every entry of EG.CHUNKS (1 token to more than the graph); the
    alpha rebuilt from each run's statistics at the same item size."""
    c = case(name)
    ops = dev_case(c, H)
    for chunk in CHUNKS:
        res = run(mk, name, ops, c, chunk)
        check_all(c, H, res, f"{name} H{H} chunk {chunk}")
        check_alpha(c, H, alpha(mk, name, ops, c, res[1], res[2], chunk),
                    f"alpha {name} H{H} chunk {chunk}")


@pytest.mark.parametrize("H", [3, 8])
def test_cut_rows_far_apart_maxima(mk, cuda, H):
    """The hub row's queries are scaled up so its logits spread over more than 160: the maxima of
    its pieces differ by more than exp can bridge in fp32, so the merge has to rescale each
    piece, neither overflow nor flush the row."""
    g = the_graph("corner")
    base = case("corner")
    q = base["q"].copy()
    q[:, g.hub] *= 8.0
    c = make_case("corner", 16, 256, 1.0, q=q, ci=base["ci"])
    lo, hi = g.rp[g.hub], g.rp[g.hub + 1]
    l = c["a"].l[0, lo:hi]
    assert l.max() - l.min() > 160
    assert np.isfinite(c["a"].out).all() and (c["a"].z[:, g.hub] >= 1).all()
    ops = dev_case(c, H)
    for chunk in (0, 64, 67, 512, 513):
        out, m, z = res = run(mk, "corner", ops, c, chunk)
        check_all(c, H, res, f"far maxima H{H} chunk {chunk}")
        assert bool(torch.isfinite(out).all()) and bool((z[:, g.hub] >= 1).all())
        assert bool(out[:, g.hub].abs().max() > 0)


# ------------------------------------------------------------------------------- composition
@pytest.mark.parametrize("H", [2, 5])
@pytest.mark.parametrize("name,k,D", [("S", 16, 256), ("Dn", 32, 256), ("R", 7, 9)])
def test_against_the_stored_composition(mk, cuda, name, k, D, H):
    """edge_weight_grad_heads(grad_output=q) times the scale, edge_softmax per head, then
    spgemm_forward_heads on the same inputs: the two results differ by at most the sum of both
    bounds (the composition's: the weight bound without the merge's 8 u carried through the
    forward's).  KG = 16, 32, 8."""
    c = make_case(name, k, D, 0.125)
    g, a = c["g"], DR.heads_slice(c["a"], H)
    stored = DR.attention(g.rp, g.col, c["q"][:H], c["scale"], c["cv"], c["ci"], D, c["n"],
                          extra=0)
    rp, col = dev_graph(name)
    q, cv, ci = ops = dev_case(c, H)
    for chunk in (0, 64):
        out = run(mk, name, ops, c, chunk)[0]
        logits = mk.edge_weight_grad_heads(rp, col, cv, ci, q, chunk=chunk).mul_(c["scale"])
        check(logits, a.l, a.l_bound, f"composition logits {name} H{H} chunk {chunk}")
        w = torch.stack([mk.edge_softmax(rp, logits[h], chunk=chunk) for h in range(H)])
        comp = mk.spgemm_forward_heads(rp, col, w, cv, ci, D, chunk=chunk)
        check(comp, stored.out, stored.out_bound, f"composition {name} H{H} chunk {chunk}")
        err = (out.double() - comp.double()).abs().cpu().numpy()
        both = a.out_bound + stored.out_bound
        assert (err <= both).all(), float((err / np.maximum(both, 1e-300)).max())
        assert bool(((out == 0) == (comp == 0))[:, T(c["n"] == 0, DEV)].all())


# ------------------------------------------------------------------------------- alpha
@pytest.mark.parametrize("H", [1, 3, 8])
@pytest.mark.parametrize("name", ["S", "corner"])
def test_alpha_from_the_statistics(mk, cuda, name, H):
    """dot_edge_alpha_heads on the fused call's statistics: w inside the weight bound, every row
    summing to one inside the sum of its bounds; the forward at item sizes that cut the long rows
    and at one that does not, the alpha entry at its own auto item size and at 64 tokens."""
    c = case(name)
    g = c["g"]
    ops = dev_case(c, H)
    for chunk in (0, 64, 4096):
        _, m, z = run(mk, name, ops, c, chunk)
        for achunk in (0, 64):
            w = alpha(mk, name, ops, c, m, z, achunk)
            check_alpha(c, H, w, f"alpha {name} H{H} chunk {chunk}/{achunk}")
    # into a given buffer of NaN: every edge is written
    buf = torch.full((H, g.col.size), float("nan"), device=cuda)
    assert alpha(mk, name, ops, c, m, z, 64, out=buf) is buf
    assert M.same_bytes(buf, w)


@pytest.mark.parametrize("k,D", SHAPES, ids=[f"k{k}-D{D}" for k, D in SHAPES])
def test_alpha_shapes(mk, cuda, k, D):
    """Every KG of dath_alpha_kernel, the one-slot and the several-slot path, odd D: graph R
    (rectangular) at H = 5."""
    H = 5
    c = make_case("R", k, D, 0.125)
    ops = dev_case(c, H)
    _, m, z = run(mk, "R", ops, c, 0)
    for achunk in (0, 64):
        check_alpha(c, H, alpha(mk, "R", ops, c, m, z, achunk), f"alpha R k{k} D{D} {achunk}")


# ------------------------------------------------------------------------------- selectors
@pytest.mark.parametrize("k,D", [(16, 100), (5, 24)])
def test_skipped_and_repeated_selectors(mk, cuda, k, D):
    """Selectors >= D (skipped), repeated inside a vertex (both values added, in the logit and in
    the sum) and output columns no edge of the row selects: the reference counts the addends, and
    an element without one is exactly 0 (check_all).  KG = 16 and 8."""
    g = the_graph("S")
    rng = np.random.default_rng(2500 + k)
    ci = N.selectors(rng, g.C, 256, k)  # selectors up to 255: many >= D
    dup = rng.choice(g.C, g.C // 4, replace=False)
    ci[dup, k - 1] = ci[dup, 0]
    c = make_case("S", k, D, 0.25, ci=ci)
    assert (ci >= D).any() and (c["n"] == 0).any() and (c["n"] > 0).any()
    ops = dev_case(c, 3)
    for chunk in (0, 64):
        res = run(mk, "S", ops, c, chunk, validate=False)
        check_all(c, 3, res, f"selectors k{k} D{D}")
        check_alpha(c, 3, alpha(mk, "S", ops, c, res[1], res[2], chunk, validate=False),
                    f"selectors alpha k{k} D{D}")


# ------------------------------------------------------------------------------- non-finite
def test_non_finite(mk, cuda):
    """Laid into head 1 of 3 on graph S, all in q: a NaN in the hub row's query at a column one
    of its neighbours selects; a +-Inf in a short row's query that makes one of its logits +Inf;
    one that makes exactly one logit of a row -Inf; a row whose logits are all -Inf; a NaN at a
    column none of the row's neighbours selects.  Head 1's NaN masks equal the reference's -- NaN
    wherever such a row has an addend, exactly 0 where it has none -- the -Inf logit adds nothing,
    the unselected NaN reaches nothing, the rest is inside the bound; heads 0 and 2 are the bytes
    of the clean run.  chunk 64 cuts the hub row: the fixup's NaN pass."""
    H, D = 3, 256
    c = case("S")
    g, ci, cv = c["g"], c["ci"], c["cv"]
    deg = np.diff(g.rp)

    def neighbours(r):
        return g.col[g.rp[r]:g.rp[r + 1]]

    def own_slot(r):
        """Per neighbour of row r, a slot whose column no other neighbour of r selects (-1 where
        it has none): an Inf of q there reaches that neighbour's logit alone."""
        s = ci[neighbours(r)]
        vals, counts = np.unique(s, return_counts=True)
        single = np.isin(s, vals[counts == 1])
        return np.where(single.any(1), single.argmax(1), -1)

    short = [int(r) for r in np.flatnonzero((deg >= 2) & (deg <= 30))
             if r != g.hub and (own_slot(int(r)) >= 0).all()]
    short.sort(key=lambda r: deg[r])
    assert len(short) >= 4
    inf_row, ninf_row, all_ninf_row, clean_row = short[:4]
    q = c["q"][:H].copy()
    c0 = neighbours(g.hub)[5]
    q[1, g.hub, ci[c0, 2]] = np.nan
    c1 = neighbours(inf_row)[0]                       # one logit +Inf, the others finite
    l1 = own_slot(inf_row)[0]
    q[1, inf_row, ci[c1, l1]] = np.copysign(np.inf, cv[c1, l1])
    c2 = neighbours(ninf_row)[1]                      # one logit -Inf, the others finite
    l2 = own_slot(ninf_row)[1]
    q[1, ninf_row, ci[c2, l2]] = -np.copysign(np.inf, cv[c2, l2])
    for cc, ll in zip(neighbours(all_ninf_row), own_slot(all_ninf_row)):  # every logit -Inf
        q[1, all_ninf_row, ci[cc, ll]] = -np.copysign(np.inf, cv[cc, ll])
    unused = np.setdiff1d(np.arange(D), ci[neighbours(clean_row)].ravel())
    q[1, clean_row, unused[:5]] = np.nan
    n = c["n"]
    a = DR.attention(g.rp, g.col, q, c["scale"], cv, ci, D, n)
    for r in (g.hub, inf_row, all_ninf_row):
        assert np.isnan(a.out[1, r][n[r] > 0]).all() and (a.out[1, r][n[r] == 0] == 0).all()
    e2 = g.rp[ninf_row] + 1
    assert a.w[1, e2] == 0 and np.isfinite(a.out[1, ninf_row]).all()
    assert np.isneginf(a.m[1, all_ninf_row]) and a.z[1, all_ninf_row] == 0
    assert np.array_equal(a.out[1, clean_row], c["a"].out[1, clean_row])
    assert np.isfinite(a.out[[0, 2]]).all() and np.isfinite(a.out[1]).mean() > 0.8
    p = dict(c, a=a, q=q)
    for chunk in (0, 64):
        clean = run(mk, "S", dev_case(c, H), c, chunk)
        ops = dev_case(c, H, q)
        res = run(mk, "S", ops, c, chunk)
        check_all(p, H, res, f"non-finite chunk {chunk}")  # the masks: N.same_class
        for x, y in zip(clean, res):
            for h in (0, 2):
                assert M.same_bytes(x[h].contiguous(), y[h].contiguous()), (chunk, h)
            assert M.same_bytes(x[1, clean_row].contiguous(), y[1, clean_row].contiguous())
        w = alpha(mk, "S", ops, c, res[1], res[2], chunk)
        check(w, a.w, a.w_bound, f"non-finite alpha chunk {chunk}")
        assert float(w[1, e2]) == 0.0  # exactly 0


@pytest.mark.parametrize("H,h", [(3, 1), (8, 6), (5, 0)])
def test_head_isolation(mk, cuda, H, h):
    """The other heads' queries replaced by other numbers, then sprinkled with NaN, +Inf and
    -Inf: head h's out, row_max and row_sum keep their bytes."""
    c = case("corner")
    rng = np.random.default_rng(2600 + H)
    for chunk in (0, 64, 7):
        base = run(mk, "corner", dev_case(c, H), c, chunk)
        for poisoned in (False, True):
            x = rng.standard_normal(c["q"][:H].shape).astype(np.float32)
            if poisoned:
                flat = x.reshape(-1)
                at = rng.choice(flat.size, max(3, flat.size // 50), replace=False)
                flat[at] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), at.size)
            x[h] = c["q"][h]
            other = run(mk, "corner", dev_case(c, H, x), c, chunk)
            for a_, b_ in zip(base, other):
                assert M.same_bytes(a_[h].contiguous(), b_[h].contiguous()), (chunk, poisoned)
            if poisoned:
                assert not bool(torch.isfinite(other[0]).all())


# ------------------------------------------------------------------------------- degenerate
@pytest.mark.parametrize("H", [1, 3, 8])
def test_no_edges(mk, cuda, H):
    """num_e == 0: zeros in all of out and both statistics; the alpha entry writes nothing."""
    rows, cols, D, k = 40, 17, 64, 8
    rp = torch.zeros(rows + 1, dtype=torch.int32, device=cuda)
    col = torch.empty(0, dtype=torch.int32, device=cuda)
    q = torch.randn(H, rows, D, device=cuda)
    cv = torch.randn(cols, k, device=cuda)
    ci = torch.zeros(cols, k, dtype=torch.uint8, device=cuda)
    buf = torch.full((H, rows, D), float("nan"), device=cuda)
    out, m, z = mk.dot_attention_heads(rp, col, q, cv, ci, D, 0.5, out=buf)
    assert out is buf and tuple(m.shape) == tuple(z.shape) == (H, rows)
    for t in (out, m, z):
        assert not t.any() and not torch.isnan(t).any()
    assert tuple(mk.dot_edge_alpha_heads(rp, col, q, cv, ci, D, 0.5, m, z).shape) == (H, 0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="scale must be finite"):
            mk.dot_attention_heads(rp, col, q, cv, ci, D, bad)


# ------------------------------------------------------------------------------- bitwise
@pytest.mark.parametrize("name", ["corner", "S"])
def test_bitwise_repeatable(mk, cuda, name):
    """Runs at H = 5 with the allocator's free blocks (where the next workspace comes from)
    filled with 0x00 and with 0xFF before each: the same bytes, the alpha too."""
    H = 5
    c = case(name)
    g = c["g"]
    ops = dev_case(c, H)
    for chunk in (0, 7, 64):
        n_ws = mk._lib().maxk_dot_attention_heads_workspace_size(g.R, g.C, g.col.size, 256, 16, H,
                                                                 chunk)
        runs = []
        for fill in (0x00, 0xFF):
            junk = [torch.full((n,), fill, dtype=torch.uint8, device=cuda)
                    for n in (n_ws, n_ws // 2, 4 * H * g.R * 256, 4096)]
            del junk
            res = run(mk, name, ops, c, chunk)
            runs.append(res + (alpha(mk, name, ops, c, res[1], res[2], chunk),))
        for x, y in zip(*runs):
            assert M.same_bytes(x, y)


# ------------------------------------------------------------------------------- memory
@pytest.fixture(scope="module")
def arena(cuda):
    return M.Arena(24 << 20, cuda)


@pytest.mark.parametrize("k,D,H", [(16, 256, 3), (16, 256, 8), (3, 64, 3)])
def test_memory_contract(mk, arena, cuda, k, D, H):
    """Outputs and workspace from the poisoned, guarded arena (the workspace exactly the queried
    size): outputs fully written and the same bytes in every fill regime, guards untouched,
    inputs unchanged; then the alpha entry the same way.  KG = 16 and 8."""
    c = case("corner", k, D)
    g = c["g"]
    E = g.col.size
    for chunk in (0, 64):
        def factory(primer):
            dt = (T(g.rp, DEV), T(g.col, DEV))
            ops = dev_case(c, H)
            if primer:
                gen = torch.Generator(device=DEV).manual_seed(5)
                ops = tuple(torch.rand(t.shape, generator=gen, device=DEV) for t in ops[:2]) \
                    + (ops[2],)
            return (dt,) + ops

        def op(dt, q, cv, ci):
            return mk.dot_attention_heads(dt[0], dt[1], q, cv, ci, D, c["scale"], chunk=chunk)

        res = M.run_regimes(op, factory, arena)
        n_ws = mk._lib().maxk_dot_attention_heads_workspace_size(g.R, g.C, E, D, k, H, chunk)
        assert sorted(x.nbytes for x in arena.allocs) == sorted(
            [4 * H * g.R * D, 4 * H * g.R, 4 * H * g.R, n_ws])
        for regime in ("stale", "ones"):
            for x, y in zip(res["zero"], res[regime]):
                assert M.same_bytes(x, y), regime
        check_all(c, H, res["ones"], f"memguard k{k} D{D} H{H} chunk {chunk}")

        m, z = res["ones"][1], res["ones"][2]

        def factory_alpha(primer):
            dt = (T(g.rp, DEV), T(g.col, DEV))
            q, cv, ci = dev_case(c, H)
            if primer:
                return dt, torch.rand_like(q), torch.rand_like(cv), ci, m.clone().abs_(), z.clone()
            return dt, q, cv, ci, m.clone(), z.clone()

        def op_alpha(dt, q, cv, ci, m_, z_):
            return (mk.dot_edge_alpha_heads(dt[0], dt[1], q, cv, ci, D, c["scale"], m_, z_,
                                            chunk=chunk),)

        res = M.run_regimes(op_alpha, factory_alpha, arena)
        n_ws = mk._lib().maxk_dot_edge_alpha_heads_workspace_size(g.R, g.C, E, D, k, H, chunk)
        assert sorted(x.nbytes for x in arena.allocs) == sorted([4 * H * E, n_ws])
        for regime in ("stale", "ones"):
            assert M.same_bytes(res["zero"][0], res[regime][0]), regime
        check(res["ones"][0], DR.heads_slice(c["a"], H).w, DR.heads_slice(c["a"], H).w_bound,
              f"memguard alpha k{k} D{D} H{H} chunk {chunk}")


@pytest.mark.parametrize("entry", ["attention", "alpha"])
def test_undersized_workspace_is_rejected(mk, arena, monkeypatch, entry):
    """A workspace one byte short of the size query: "workspace too small" from the host-side
    check, before any launch -- the outputs (0xFF-filled) are unchanged, the guards intact."""
    H = 5
    c = case("corner")
    g = c["g"]
    dt = (T(g.rp, DEV), T(g.col, DEV))
    q, cv, ci = dev_case(c, H)
    m, z = torch.zeros(H, g.R, device=DEV), torch.ones(H, g.R, device=DEV)
    torch.cuda.synchronize()
    shrunk = Shrunk(mk._L, {"attention": "maxk_dot_attention_heads_workspace_size",
                            "alpha": "maxk_dot_edge_alpha_heads_workspace_size"}[entry])
    monkeypatch.setattr(mk, "_L", shrunk)
    with arena.active("ones"):
        with pytest.raises(RuntimeError, match="workspace too small"):
            if entry == "attention":
                mk.dot_attention_heads(dt[0], dt[1], q, cv, ci, 256, c["scale"])
            else:
                mk.dot_edge_alpha_heads(dt[0], dt[1], q, cv, ci, 256, c["scale"], m, z)
        made = len(arena.allocs)
    assert shrunk.sizes and all(n > 1 for n in shrunk.sizes), shrunk.sizes
    assert made >= 2  # the outputs and the short workspace came from the arena
    arena.check()
    assert arena.untouched()


# ------------------------------------------------------------------------------- streams
def test_runs_on_the_current_stream_and_captures(mk, cuda):
    """On a side stream made current the call is ordered after work queued there before it; one
    hipGraph capture of the forward and the alpha entry -- a single chain of kernels -- replayed
    twice equals the eager result bitwise.  H = 3."""
    H = 3
    c = case("corner")
    rp, col = dev_graph("corner")
    q, cv, ci = dev_case(c, H)
    D, s = 256, c["scale"]
    for chunk in (0, 64):
        eager = mk.dot_attention_heads(rp, col, q, cv, ci, D, s, chunk=chunk)
        eager_w = mk.dot_edge_alpha_heads(rp, col, q, cv, ci, D, s, eager[1], eager[2],
                                          chunk=chunk)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            q2 = torch.zeros_like(q)
            for _ in range(20):  # queued on the side stream before the call
                q2 = q2 + q / 20
            q2.copy_(q)
            res = mk.dot_attention_heads(rp, col, q2, cv, ci, D, s, chunk=chunk)
        side.synchronize()
        for x, y in zip(eager, res):
            assert M.same_bytes(x, y)
        out = torch.empty_like(eager[0])
        w = torch.empty_like(eager_w)
        hg = torch.cuda.CUDAGraph()
        stats = []
        with torch.cuda.graph(hg, stream=side):
            _, m, z = mk.dot_attention_heads(rp, col, q, cv, ci, D, s, chunk=chunk, out=out,
                                             validate=False)
            mk.dot_edge_alpha_heads(rp, col, q, cv, ci, D, s, m, z, chunk=chunk, out=w,
                                    validate=False)
            stats += [m, z]
        for _ in range(2):
            for t in (out, w, *stats):
                t.fill_(float("nan"))
            hg.replay()
            torch.cuda.synchronize()
            for x, y in zip((*eager, eager_w), (out, *stats, w)):
                assert M.same_bytes(x, y)


# ------------------------------------------------------------------------------- autograd
def agg_ref(g, w, w_bound, cv, ci, D, n):
    """sum over a row's edges of w[e] * scatter(cv)[col[e]] for one head in float64, with the
    forward aggregation's bound and w's own bound carried through the sum."""
    rows = ER.edge_rows(g.rp)
    sel = ci[g.col].astype(np.int64)
    keep = (sel < D).ravel()
    idx = (rows[:, None].astype(np.int64) * D + sel).ravel()[keep]
    v = cv[g.col].astype(np.float64)
    size = g.R * D
    out = np.bincount(idx, (w[:, None] * v).ravel()[keep], minlength=size)
    s_abs = np.bincount(idx, np.abs(w[:, None] * v).ravel()[keep], minlength=size)
    carried = np.bincount(idx, (w_bound[:, None] * np.abs(v)).ravel()[keep], minlength=size)
    nn = np.rint(n.astype(np.float64)).ravel()
    bound = np.where(nn > 0, (nn + 8) * (DR.U * s_abs + DR.FLOOR) + carried, 0.0)
    return out.reshape(g.R, D), bound.reshape(g.R, D)


def dense_grads(g, ci, cv, q, scale, D, G, logits_cotangent=None):
    """(grad_q [H, R, D], grad_cv [C, k]) by float64 torch autograd of the dense composition of
    test_dot_attention_cpu: of the attention output under the cotangent G, or of the logits under
    logits_cotangent [H, E]."""
    cvt = torch.from_numpy(cv.astype(np.float64)).requires_grad_(True)
    C, k = ci.shape
    X = torch.zeros(C, 256, dtype=torch.float64)
    X = X.index_put((torch.arange(C)[:, None].expand(-1, k), torch.from_numpy(ci.astype(np.int64))),
                    cvt, accumulate=True)[:, :D]
    qt = torch.from_numpy(q.astype(np.float64)).requires_grad_(True)
    out, _, e = DC.dense_composition(g, X, qt, scale)
    if logits_cotangent is None:
        out.backward(torch.from_numpy(G.astype(np.float64)))
    else:
        rows = ER.edge_rows(g.rp)
        e[:, rows, g.col.astype(np.int64)].backward(torch.from_numpy(logits_cotangent))
    return qt.grad.numpy(), cvt.grad.numpy()


def test_autograd_scores(mk, cuda, monkeypatch):
    """MaxKDotScoresHeadsFunction, H = 3 on graph S with a random cotangent: the logits inside
    the logit bound, the gradient of q inside the forward aggregation's bound times scale, the
    gradient of topk_values inside the feature gradient's; the values from dense float64 torch."""
    import maxk_spgemm_function as MF
    monkeypatch.setenv("MAXK_BWD_MODE", "csc")
    D, k, H = 64, 16, 3
    c = case("S", k, D, 0.25)
    g, a = c["g"], DR.heads_slice(c["a"], H)
    s = c["scale"]
    rng = np.random.default_rng(2800)
    Gl = rng.standard_normal((H, g.col.size))
    Gl = Gl.astype(np.float32).astype(np.float64)
    rp, col = dev_graph("S")
    q, tv, ci = dev_case(c, H)
    q.requires_grad_(True)
    tv.requires_grad_(True)
    logits = MF.maxk_dot_scores_heads(rp, col, q, tv, ci, s)
    logits.backward(T(Gl.astype(np.float32), cuda))
    check(logits.detach(), a.l, a.l_bound, "scores logits")
    gq_ref, gtv_ref = dense_grads(g, c["ci"], c["cv"], c["q"][:H], s, D, None, Gl)
    zero = np.zeros(g.col.size)
    gq = [agg_ref(g, Gl[h], zero, c["cv"], c["ci"], D, c["n"]) for h in range(H)]
    gq_val = s * np.stack([x[0] for x in gq])
    assert np.abs(gq_val - gq_ref).max() <= 1e-10 * max(1.0, np.abs(gq_ref).max())
    check(q.grad, gq_ref, s * np.stack([x[1] for x in gq]), "scores q.grad")
    like = types.SimpleNamespace(w=Gl, w_bound=np.zeros_like(Gl))
    val, bound = GA.feat_grad_ref(g, like, c["q"][:H], c["ci"], D)
    assert np.abs(s * val - gtv_ref).max() <= 1e-10 * max(1.0, np.abs(gtv_ref).max())
    check(tv.grad, gtv_ref, s * bound, "scores topk_values.grad")


def test_autograd_matches_dense_and_the_stored_path(mk, cuda, monkeypatch):
    """MaxKDotAttentionHeadsFunction (CSRGraph.dot_attend_heads) and the stored path
    (maxk_dot_scores_heads, edge_softmax per head, aggregate_heads), H = 3 on graph S with a
    random cotangent, against float64 dense torch: the output inside the attention bound, the
    gradients inside bounds carried from the reference -- the weight bound and the edge
    gradient's through the softmax backward (edge_softmax_ref.backward), that through the
    aggregation onto q, and both onto topk_values -- each path inside them, so the two within
    twice; and the fused function saves the graph, q, the CBSR and the statistics and no tensor
    of H * E elements, where the stored path saves alpha [H, E]."""
    import maxk_layers as ML
    import maxk_spgemm_function as MF
    monkeypatch.setenv("MAXK_BWD_MODE", "csc")
    D, k, H = 64, 16, 3
    c = case("S", k, D, 0.25)
    g, a = c["g"], DR.heads_slice(c["a"], H)
    s = c["scale"]
    E = g.col.size
    rng = np.random.default_rng(2700)
    G = np.stack([N.values(rng, (g.R, D), "unit") for _ in range(H)])
    rp, col = dev_graph("S")
    graph_ = ML.CSRGraph(rp, col)
    res, saved = {}, {}
    for path in ("fused", "stored"):
        q, tv, ci = dev_case(c, H)
        q.requires_grad_(True)
        tv.requires_grad_(True)
        sizes = []
        with torch.autograd.graph.saved_tensors_hooks(
                lambda t: sizes.append(t.numel()) or t, lambda t: t):
            if path == "fused":
                y = graph_.dot_attend_heads(tv, ci, D, q, s)
            else:
                logits = MF.maxk_dot_scores_heads(rp, col, q, tv, ci, s)
                w = torch.stack([ML.edge_softmax(graph_, logits[h]) for h in range(H)])
                y = graph_.aggregate_heads(tv, ci, D, w)
        y.backward(T(G, cuda))
        res[path] = (y.detach(), q.grad, tv.grad)
        saved[path] = sizes
    # E = 7777 edges: the graph's indices are the only saved tensor made of edges (q [H, V, D] is
    # larger than H * E on this small graph, so sizes are told apart by their factor E)
    assert saved["fused"] and all(n == E or n % E for n in saved["fused"]), saved["fused"]
    assert sorted(set(saved["fused"])) == sorted({g.R + 1, E, H * g.R * D, g.C * k, H * g.R})
    assert H * E in saved["stored"]
    # the reference chain and its bounds
    gq_ref, gtv_ref = dense_grads(g, c["ci"], c["cv"], c["q"][:H], s, D, G)
    ers = [R.edge_grad_ref(g.rp, g.col, c["cv"], c["ci"], G[h], None) for h in range(H)]
    bs = [ER.backward(g.rp, g.col, a.heads[h]._replace(bound=a.w_bound[h]), ers[h].ref,
                      gw_bound=R.bound(ers[h])) for h in range(H)]
    gl = np.stack([b.gl for b in bs])
    gl_bound = np.stack([b.gl_bound for b in bs])
    gq = [agg_ref(g, gl[h], gl_bound[h], c["cv"], c["ci"], D, c["n"]) for h in range(H)]
    gq_val = s * np.stack([x[0] for x in gq])
    gq_bound = s * np.stack([x[1] for x in gq])
    assert np.abs(gq_val - gq_ref).max() <= 1e-10 * max(1.0, np.abs(gq_ref).max())
    v1, b1 = GA.feat_grad_ref(g, a, G, c["ci"], D)
    v2, b2 = GA.feat_grad_ref(g, types.SimpleNamespace(w=gl, w_bound=gl_bound), c["q"][:H],
                              c["ci"], D)
    assert np.abs(v1 + s * v2 - gtv_ref).max() <= 1e-10 * max(1.0, np.abs(gtv_ref).max())
    gtv_bound = b1 + s * b2 + 2 * DR.U * (np.abs(v1) + s * np.abs(v2))  # the scale and the sum
    for path in ("fused", "stored"):
        y, gq_, gt = res[path]
        check(y, a.out, a.out_bound, f"autograd {path} out")
        check(gq_, gq_ref, gq_bound, f"autograd {path} q.grad")
        check(gt, gtv_ref, gtv_bound, f"autograd {path} topk_values.grad")


def test_transformer_conv_fused_matches_stored_and_dense(cuda, monkeypatch):
    """MaxKTransformerConv at V = 300, in = 64, out = 8, H = 4, k = 16: attention="fused" and
    "stored" against the same layer in dense float64 torch (masked dense softmax of the scaled
    q . k over the adjacency, per head) -- the output, every parameter's gradient and both input
    gradients at rtol = atol = 1e-4, so fused against stored within twice that; MAXK_DOT_ATTN
    overrides the argument; attn_drop on the stored path is reproducible under a fixed
    attn_seed and raises on the fused one."""
    import maxk_cuda_kernels as mk_
    import maxk_layers as ML
    monkeypatch.delenv("MAXK_DOT_ATTN", raising=False)
    torch.manual_seed(4)
    rng = np.random.default_rng(300)
    V, D, k, O_, H = 300, 64, 16, 8, 4
    rp, col = rand_graph(rng, V, 8, hubs=((7, 220),), empty=3)
    graph_ = ML.CSRGraph(T(rp.astype(np.int32), cuda), T(col.astype(np.int32), cuda))
    conv = ML.MaxKTransformerConv(D, O_, H, attention="fused").to(cuda)
    with torch.no_grad():
        conv.bias.normal_()
    x = torch.randn(V, D, device=cuda)
    xs, vals, idx = ML.maxk(x, k)
    xs = xs.detach().requires_grad_(True)
    vals = vals.detach().requires_grad_(True)
    gout = torch.randn(V, H, O_, device=cuda)
    names = ["fc_q.weight", "fc_k.weight", "fc_v.weight", "bias"]
    P = dict(conv.named_parameters())

    A = torch.zeros(V, V, dtype=torch.float64, device=cuda)
    rows = torch.repeat_interleave(torch.arange(V, device=cuda),
                                   T(np.diff(rp).astype(np.int64), cuda))
    A[rows, T(col.astype(np.int64), cuda)] = 1.0
    Q = {n: P[n].detach().double().requires_grad_(True) for n in names}
    xs2 = xs.detach().double().requires_grad_(True)
    vals2 = vals.detach().double().requires_grad_(True)
    xv = torch.zeros(V, D, dtype=torch.float64, device=cuda).scatter(1, idx.long(), vals2)
    masked = (A == 0) & (A.sum(1, keepdim=True) > 0)
    heads = []
    for h in range(H):
        Wq, Wk, Wv = (Q[n][h * O_:(h + 1) * O_] for n in names[:3])
        e = (xs2 @ Wq.t()) @ (xv @ Wk.t()).t() / O_ ** 0.5
        al = torch.softmax(e.masked_fill(masked, float("-inf")), 1) * A
        heads.append(al @ (xv @ Wv.t()) + Q["bias"][h])
    ref = torch.stack(heads, 1)
    want = torch.autograd.grad(ref, [Q[n] for n in names] + [xs2, vals2], gout.double())
    empty = T(np.diff(rp) == 0, cuda)
    calls = []
    real = mk_.dot_attention_heads
    monkeypatch.setattr(mk_, "dot_attention_heads",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    outs = {}
    for arg, env, fused in (("fused", None, True), ("stored", None, False),
                            ("stored", "fused", True), ("fused", "stored", False)):
        conv.attention = arg
        if env is None:
            monkeypatch.delenv("MAXK_DOT_ATTN", raising=False)
        else:
            monkeypatch.setenv("MAXK_DOT_ATTN", env)
        del calls[:]
        out = conv(graph_, xs, vals, idx)
        assert len(calls) == (1 if fused else 0), (arg, env)
        assert tuple(out.shape) == (V, H, O_)
        got = torch.autograd.grad(out, [P[n] for n in names] + [xs, vals], gout)
        torch.testing.assert_close(out, ref.float(), rtol=1e-4, atol=1e-4)
        for n, a, b in zip(names + ["x_sparse", "topk_values"], got, want):
            torch.testing.assert_close(a, b.float(), rtol=1e-4, atol=1e-4,
                                       msg=lambda m: f"{arg} {env} {n}: {m}")
        assert not out[empty].sub(conv.bias).abs().max() > 0  # empty rows: the bias alone
        outs[fused] = (out.detach(), got)
    torch.testing.assert_close(outs[True][0], outs[False][0], rtol=2e-4, atol=2e-4)
    for a, b in zip(outs[True][1], outs[False][1]):
        torch.testing.assert_close(a, b, rtol=2e-4, atol=2e-4)
    # attention dropout: the stored path, reproducible under a fixed seed
    monkeypatch.delenv("MAXK_DOT_ATTN", raising=False)
    conv.attention, conv.attn_drop = "stored", 0.4
    conv.train()
    d1 = conv(graph_, xs, vals, idx, attn_seed=11)
    g1 = torch.autograd.grad(d1, [P[n] for n in names] + [xs, vals], gout)
    d2 = conv(graph_, xs, vals, idx, attn_seed=11)
    g2 = torch.autograd.grad(d2, [P[n] for n in names] + [xs, vals], gout)
    assert M.same_bytes(d1.detach(), d2.detach())
    for a, b in zip(g1, g2):
        assert M.same_bytes(a, b)
    assert not M.same_bytes(d1.detach(), conv(graph_, xs, vals, idx, attn_seed=12).detach())
    assert not M.same_bytes(d1.detach(), outs[False][0])
    conv.eval()  # no dropout in eval: the bytes of the layer without the argument
    assert M.same_bytes(conv(graph_, xs, vals, idx).detach(), outs[False][0])
    conv.train()
    conv.attention = "fused"
    with pytest.raises(ValueError, match="no dropout yet"):
        conv(graph_, xs, vals, idx)


def test_ratios_are_reported():
    """Last in the file: the largest err/bound ratios seen, for the record."""
    for what, r in sorted(RATIOS.items(), key=lambda kv: -kv[1])[:12]:
        print(f"{r:.3f}  {what}")
    assert all(r <= 1.0 for r in RATIOS.values())
