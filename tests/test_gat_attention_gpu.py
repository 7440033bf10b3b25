"""GPU: the fused multi-head GAT attention (gat_attention_heads.hip) through the binding
(mk.gat_attention_heads, mk.gat_edge_alpha_heads), the autograd function
MaxKGATAttentionHeadsFunction and MaxKMultiHeadGATConv(attention="fused"), against
tests/gat_attention_ref.py (float64, with its derived bounds), against the composition it
replaces (mk.gat_edge_softmax_heads then mk.spgemm_forward_heads) and against the stored path's
autograd.

Which kernels.  Every non-empty forward launches cbsr_pack_kernel or cbsr_pack4_kernel
(k % 4 == 0), gath_interleave_kernel<HP>, gath_fwd_kernel<KG, HP, 8> and softmax_fixup_kernel<false>
(heads_walk.h, which also holds the walk the forward kernel shares with the other heads forwards);
every non-empty alpha call gath_interleave_kernel<HP> and gath_alpha_kernel<HP>.  HP = 2, 2, 4, 8,
8 for H = 1, 2, 3, 5, 8; KG = 8 for k = 3, 7, 8, 16 for k = 16, 32 for k = 24, 32, 64 for k = 96.
test_parity runs every (k, H) of SHAPES x HEADS, so it reaches the twelve gath_fwd_kernel
instantiations (KG in 8, 16, 32, 64 x HP in 2, 4, 8) and the three interleaves;
test_alpha_from_the_statistics runs H in 1, 3, 8: the three gath_alpha_kernel instantiations.
The others run KG = 16 with HP = 4 (H = 3) or HP = 8 (H = 8) unless their docstrings say
otherwise.  The NaN pass of gath_fwd_kernel (walk_attn<.., true>) and of softmax_fixup_kernel run
in test_non_finite (rows inside an item and the hub row at chunk 64).

The largest err / bound seen on an MI355X is in test_ratios_are_reported's output; the figures
of the first run are recorded in profiles/r15/gat_attention/README.md.
"""
import functools

import numpy as np
import pytest
import torch

import edge_grad_ref as R
import edge_softmax_ref as ER
import esm_corner_graph as EG
import gat_attention_ref as AR
import heads_softmax_ref as HS
import memguard as M
import numerics as N
import test_edge_softmax_gpu as TG
import test_numerics_gpu as TN
from test_memguard_gpu import Shrunk
from test_parity_gpu import T, rand_graph

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CHUNKS = (0,) + EG.CHUNKS
HEADS = (1, 2, 3, 5, 8)
HMAX = 8
SLOPE = 0.2
SHAPES = [(3, 64), (8, 256), (16, 256), (32, 256), (24, 256), (96, 256), (7, 9)]
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
    return TN.graph(name)  # "S", "Dn", "R"


@functools.lru_cache(maxsize=None)
def dev_graph(name):
    g = the_graph(name)
    return T(g.rp, DEV), T(g.col, DEV)


def make_case(name, k, D, seed=0, scores=None, ci=None):
    """HMAX heads of scores, a CBSR and the float64 reference; H heads are the first H."""
    g = the_graph(name)
    rng = np.random.default_rng(2400 + 31 * k + D + seed)
    if scores is None:
        scores = (rng.standard_normal((HMAX, g.R)).astype(np.float32),
                  rng.standard_normal((HMAX, g.C)).astype(np.float32))
    s_dst, s_src = scores
    ci = N.selectors(rng, g.C, D, k) if ci is None else ci
    cv = N.values(rng, (g.C, k), "unit")
    n = N.count_fwd(g, ci, D)
    a = AR.attention(g.rp, g.col, s_dst, s_src, SLOPE, cv, ci, D, n)
    return dict(g=g, s_dst=s_dst, s_src=s_src, ci=ci, cv=cv, n=n, a=a, D=D, k=k)


@functools.lru_cache(maxsize=None)
def case(name, k=16, D=256):
    """The cases several tests share: computed once, never modified."""
    return make_case(name, k, D)


def dev_case(c, H, s_dst=None, s_src=None):
    return (T(np.ascontiguousarray((c["s_dst"] if s_dst is None else s_dst)[:H]), DEV),
            T(np.ascontiguousarray((c["s_src"] if s_src is None else s_src)[:H]), DEV),
            T(c["cv"], DEV), T(c["ci"], DEV))


def run(mk, name, ops, D, chunk, dt=None, **kw):
    rp, col = dev_graph(name) if dt is None else dt
    sd, ss, cv, ci = ops
    return mk.gat_attention_heads(rp, col, sd, ss, cv, ci, D, SLOPE, chunk=chunk, **kw)


def check(y, ref, bound, what):
    assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape, (y.shape, ref.shape)
    r = N.within(y, ref, bound, what)
    RATIOS[what] = r
    print(f"{what}: err/bound {r:.3f}")
    return r


def check_all(c, H, res, what):
    """out and both statistics inside their bounds; exact zeros where nothing is added."""
    g, a = c["g"], AR.heads_slice(c["a"], H)
    out, m, z = res
    check(out, a.out, a.out_bound, f"{what} out")
    check(m, a.m, a.m_bound, f"{what} row_max")
    check(z, a.z, a.z_bound, f"{what} row_sum")
    empty = T(np.diff(g.rp) == 0, DEV)
    assert not out[:, empty].any() and not m[:, empty].any() and not z[:, empty].any()
    assert not out[:, T(c["n"] == 0, DEV)].any()  # a column no edge of the row selects


# ------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("k,D", SHAPES, ids=[f"k{k}-D{D}" for k, D in SHAPES])
@pytest.mark.parametrize("name", ["S", "Dn", "R"])
def test_parity(mk, cuda, name, k, D):
    """out, row_max and row_sum inside the derived bounds for H in 1, 2, 3, 5, 8 at the auto
    item size and at 64 tokens.  Every gath_fwd_kernel and gath_interleave_kernel
    instantiation (see the module text)."""
    c = make_case(name, k, D)
    for H in HEADS:
        ops = dev_case(c, H)
        for chunk in (0, 64):
            check_all(c, H, run(mk, name, ops, D, chunk), f"{name} k{k} D{D} H{H} chunk {chunk}")


# ------------------------------------------------------------------------------- cut rows
@pytest.mark.parametrize("H", [3, 8])
@pytest.mark.parametrize("name", ["corner", "transpose"])
def test_cut_rows(mk, cuda, name, H):
    """Rows of 32 / 33 and 512 / 513 edges, the hub of 1700, empty rows first, in a run and last,
    at the auto item size and every entry of EG.CHUNKS (1 token to more than the graph)."""
    c = case(name)
    ops = dev_case(c, H)
    for chunk in CHUNKS:
        check_all(c, H, run(mk, name, ops, 256, chunk), f"{name} H{H} chunk {chunk}")


@pytest.mark.parametrize("H", [3, 8])
def test_cut_rows_far_apart_maxima(mk, cuda, H):
    """The hub row's source scores ramp from -50 to 150 along its edges, so the maxima of its
    pieces differ by more than 80 (exp(-80) underflows fp32's normal range): the merge has to
    rescale each piece, neither overflow nor flush the row."""
    g = the_graph("corner")
    base = case("corner")
    lo, hi = g.rp[g.hub], g.rp[g.hub + 1]
    s_src = base["s_src"].copy()
    s_src[:, g.col[lo:hi]] += np.linspace(-50, 150, hi - lo, dtype=np.float32)[None]
    c = make_case("corner", 16, 256, scores=(base["s_dst"], s_src), ci=base["ci"])
    l = c["a"].heads[0].l
    assert l[hi - 300:hi].max() - l[lo:lo + 300].max() > 80
    assert np.isfinite(c["a"].out).all() and (c["a"].z[:, g.hub] >= 1).all()
    ops = dev_case(c, H)
    for chunk in (0, 64, 67, 512, 513):
        out, m, z = res = run(mk, "corner", ops, 256, chunk)
        check_all(c, H, res, f"far maxima H{H} chunk {chunk}")
        assert bool(torch.isfinite(out).all()) and bool((z[:, g.hub] >= 1).all())
        assert bool(out[:, g.hub].abs().max() > 0)


# ------------------------------------------------------------------------------- composition
@pytest.mark.parametrize("H", [2, 5])
@pytest.mark.parametrize("name,k,D", [("S", 16, 256), ("Dn", 32, 256), ("R", 7, 9)])
def test_against_the_stored_composition(mk, cuda, name, k, D, H):
    """gat_edge_softmax_heads then spgemm_forward_heads on the same inputs: the two results
    differ by at most the sum of both bounds (the composition's: the edge softmax's bound of w
    carried through the forward's).  KG = 16, 32, 8; HP = 2 and 8."""
    c = make_case(name, k, D)
    g, a = c["g"], AR.heads_slice(c["a"], H)
    stored = AR.attention(g.rp, g.col, c["s_dst"][:H], c["s_src"][:H], SLOPE, c["cv"], c["ci"], D,
                          c["n"], extra=0)
    rp, col = dev_graph(name)
    sd, ss, cv, ci = ops = dev_case(c, H)
    for chunk in (0, 64):
        out = run(mk, name, ops, D, chunk)[0]
        w = mk.gat_edge_softmax_heads(rp, col, sd, ss, SLOPE, chunk=chunk)
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
    """gat_edge_alpha_heads on the fused call's statistics: w inside the edge softmax's forward
    bound, every row summing to one inside row_sum_bound; at item sizes that cut the long rows
    and at one that does not.  gath_alpha_kernel<2>, <4>, <8>."""
    c = case(name)
    g, a = c["g"], AR.heads_slice(c["a"], H)
    rp, col = dev_graph(name)
    sd, ss, _, _ = ops = dev_case(c, H)
    for chunk in (0, 64, 4096):
        _, m, z = run(mk, name, ops, 256, chunk)
        w = mk.gat_edge_alpha_heads(rp, col, sd, ss, m, z, SLOPE)
        check(w, a.w, a.w_bound, f"alpha {name} H{H} chunk {chunk}")
        for h in range(H):
            TG.check_rows_sum_to_one(w[h], a.heads[h], g, f"alpha {name} H{H} head {h}")
    # into a given buffer of NaN: every edge is written
    buf = torch.full((H, g.col.size), float("nan"), device=cuda)
    assert mk.gat_edge_alpha_heads(rp, col, sd, ss, m, z, SLOPE, out=buf) is buf
    assert M.same_bytes(buf, w)


# ------------------------------------------------------------------------------- selectors
@pytest.mark.parametrize("k,D", [(16, 100), (5, 24)])
def test_skipped_and_repeated_selectors(mk, cuda, k, D):
    """Selectors >= D (skipped), repeated inside a vertex (both values added) and output columns
    no edge of the row selects: the reference counts the addends, and an element without one is
    exactly 0 (check_all).  KG = 16 and 8, HP = 4."""
    g = the_graph("S")
    rng = np.random.default_rng(2500 + k)
    ci = N.selectors(rng, g.C, 256, k)  # selectors up to 255: many >= D
    dup = rng.choice(g.C, g.C // 4, replace=False)
    ci[dup, k - 1] = ci[dup, 0]
    c = make_case("S", k, D, ci=ci)
    assert (ci >= D).any() and (c["n"] == 0).any() and (c["n"] > 0).any()
    ops = dev_case(c, 3)
    for chunk in (0, 64):
        check_all(c, 3, run(mk, "S", ops, D, chunk, validate=False), f"selectors k{k} D{D}")


# ------------------------------------------------------------------------------- non-finite
def test_non_finite(mk, cuda):
    """Laid into head 1 of 3 on graph S: a NaN in s_src at a column the hub row and a short row
    read, a +Inf in s_src at another column and in s_dst of a short row, a -Inf in s_src at a
    vertex whose readers all have other neighbours, a row of only -Inf (s_dst = -Inf), a NaN at
    the unread column.  Head 1's NaN masks equal the reference's -- NaN wherever such a row has
    an addend, exactly 0 where it has none -- the -Inf logit adds nothing, the rest is inside
    the bound; heads 0 and 2 are the bytes of the clean run.  chunk 64 cuts the hub row: the
    fixup's NaN pass."""
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
    taken = np.concatenate([readers[nan_col], readers[ninf_col]])
    inf_col = next(int(v) for v in range(g.C)
                   if v not in (nan_col, ninf_col, g.unread) and readers[v].size >= 2
                   and g.hub not in readers[v] and not np.isin(readers[v], taken).any())
    taken = np.concatenate([taken, readers[inf_col]])
    free = ~np.isin(np.arange(g.R), taken) & (deg >= 3) & (deg <= 30)
    inf_row, ninf_row = (int(r) for r in np.flatnonzero(free)[:2])
    s_dst, s_src = c["s_dst"][:H].copy(), c["s_src"][:H].copy()
    s_src[1, nan_col] = np.nan
    s_src[1, inf_col] = np.inf
    s_src[1, ninf_col] = -np.inf
    s_dst[1, inf_row] = np.inf
    s_dst[1, ninf_row] = -np.inf
    s_src[1, g.unread] = np.nan
    a = AR.attention(g.rp, g.col, s_dst, s_src, SLOPE, c["cv"], c["ci"], 256, c["n"])
    n = c["n"]
    for r in (g.hub, inf_row, ninf_row, *readers[inf_col]):
        assert np.isnan(a.out[1, r][n[r] > 0]).all() and (a.out[1, r][n[r] == 0] == 0).all()
    assert (a.w[1][g.col == ninf_col] == 0).all() and np.isfinite(a.out[1]).mean() > 0.8
    assert np.isfinite(a.out[[0, 2]]).all()
    p = dict(c, a=a)
    for chunk in (0, 64):
        clean = run(mk, "S", dev_case(c, H), 256, chunk)
        res = run(mk, "S", dev_case(c, H, s_dst, s_src), 256, chunk)
        check_all(p, H, res, f"non-finite chunk {chunk}")  # the masks: N.same_class
        for x, y in zip(clean, res):
            for h in (0, 2):
                assert M.same_bytes(x[h].contiguous(), y[h].contiguous()), (chunk, h)
        rp, col = dev_graph("S")
        w = mk.gat_edge_alpha_heads(rp, col, T(s_dst, DEV), T(s_src, DEV), res[1], res[2], SLOPE)
        check(w, a.w, a.w_bound, f"non-finite alpha chunk {chunk}")
        assert not w[1][T(g.col == ninf_col, DEV)].any()  # exactly 0


@pytest.mark.parametrize("H,h", [(3, 1), (8, 6), (5, 0)])
def test_head_isolation(mk, cuda, H, h):
    """The other heads' scores replaced by other numbers, then sprinkled with NaN, +Inf and
    -Inf: head h's out, row_max and row_sum keep their bytes.  HP = 4 and 8."""
    c = case("corner")
    rng = np.random.default_rng(2600 + H)
    for chunk in (0, 64, 7):
        base = run(mk, "corner", dev_case(c, H), 256, chunk)
        for poisoned in (False, True):
            arrs = []
            for name in ("s_dst", "s_src"):
                x = rng.standard_normal(c[name][:H].shape).astype(np.float32)
                if poisoned:
                    flat = x.reshape(-1)
                    at = rng.choice(flat.size, max(3, flat.size // 50), replace=False)
                    flat[at] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), at.size)
                x[h] = c[name][h]
                arrs.append(x)
            other = run(mk, "corner", dev_case(c, H, *arrs), 256, chunk)
            for x, y in zip(base, other):
                assert M.same_bytes(x[h].contiguous(), y[h].contiguous()), (chunk, poisoned)
            if poisoned:
                assert not bool(torch.isfinite(other[0]).all())


# ------------------------------------------------------------------------------- degenerate
@pytest.mark.parametrize("H", [1, 3, 8])
def test_no_edges(mk, cuda, H):
    """num_e == 0: zeros in all of out and both statistics; the alpha entry writes nothing."""
    rows, cols, D, k = 40, 17, 64, 8
    rp = torch.zeros(rows + 1, dtype=torch.int32, device=cuda)
    col = torch.empty(0, dtype=torch.int32, device=cuda)
    sd, ss = torch.randn(H, rows, device=cuda), torch.randn(H, cols, device=cuda)
    cv = torch.randn(cols, k, device=cuda)
    ci = torch.zeros(cols, k, dtype=torch.uint8, device=cuda)
    buf = torch.full((H, rows, D), float("nan"), device=cuda)
    out, m, z = mk.gat_attention_heads(rp, col, sd, ss, cv, ci, D, out=buf)
    assert out is buf and tuple(m.shape) == tuple(z.shape) == (H, rows)
    for t in (out, m, z):
        assert not t.any() and not torch.isnan(t).any()
    assert tuple(mk.gat_edge_alpha_heads(rp, col, sd, ss, m, z).shape) == (H, 0)


# ------------------------------------------------------------------------------- bitwise
@pytest.mark.parametrize("name", ["corner", "S"])
def test_bitwise_repeatable(mk, cuda, name):
    """Runs at H = 5 (HP = 8) with the allocator's free blocks (where the next workspace comes
    from) filled with 0x00 and with 0xFF before each: the same bytes."""
    H = 5
    c = case(name)
    g = c["g"]
    ops = dev_case(c, H)
    for chunk in (0, 7, 64):
        n_ws = mk._lib().maxk_gat_attention_heads_workspace_size(g.R, g.C, g.col.size, 256, 16, H,
                                                                 chunk)
        runs = []
        for fill in (0x00, 0xFF):
            junk = [torch.full((n,), fill, dtype=torch.uint8, device=cuda)
                    for n in (n_ws, n_ws // 2, 4 * H * g.R * 256, 4096)]
            del junk
            runs.append(run(mk, name, ops, 256, chunk))
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
    inputs unchanged; then the alpha entry the same way.  KG = 16 and 8, HP = 4 and 8."""
    c = case("corner", k, D)
    g, a = c["g"], AR.heads_slice(c["a"], H)
    E = g.col.size
    for chunk in (0, 64):
        def factory(primer):
            dt = (T(g.rp, DEV), T(g.col, DEV))
            ops = dev_case(c, H)
            if primer:
                gen = torch.Generator(device=DEV).manual_seed(5)
                ops = tuple(torch.rand(t.shape, generator=gen, device=DEV) for t in ops[:3]) \
                    + (ops[3],)
            return (dt,) + ops

        def op(dt, sd, ss, cv, ci):
            return mk.gat_attention_heads(dt[0], dt[1], sd, ss, cv, ci, D, SLOPE, chunk=chunk)

        res = M.run_regimes(op, factory, arena)
        n_ws = mk._lib().maxk_gat_attention_heads_workspace_size(g.R, g.C, E, D, k, H, chunk)
        assert sorted(x.nbytes for x in arena.allocs) == sorted(
            [4 * H * g.R * D, 4 * H * g.R, 4 * H * g.R, n_ws])
        for regime in ("stale", "ones"):
            for x, y in zip(res["zero"], res[regime]):
                assert M.same_bytes(x, y), regime
        check_all(c, H, res["ones"], f"memguard k{k} D{D} H{H} chunk {chunk}")

        m, z = res["ones"][1], res["ones"][2]

        def factory_alpha(primer):
            dt = (T(g.rp, DEV), T(g.col, DEV))
            sd, ss = dev_case(c, H)[:2]
            if primer:
                return dt, torch.rand_like(sd), torch.rand_like(ss), m.clone().abs_(), z.clone()
            return dt, sd, ss, m.clone(), z.clone()

        def op_alpha(dt, sd, ss, m_, z_):
            return (mk.gat_edge_alpha_heads(dt[0], dt[1], sd, ss, m_, z_, SLOPE),)

        res = M.run_regimes(op_alpha, factory_alpha, arena)
        n_ws = mk._lib().maxk_gat_edge_alpha_heads_workspace_size(H, g.R, g.C, E)
        assert sorted(x.nbytes for x in arena.allocs) == sorted([4 * H * E, n_ws])
        for regime in ("stale", "ones"):
            assert M.same_bytes(res["zero"][0], res[regime][0]), regime
        check(res["ones"][0], a.w, a.w_bound, f"memguard alpha k{k} D{D} H{H} chunk {chunk}")


@pytest.mark.parametrize("entry", ["attention", "alpha"])
def test_undersized_workspace_is_rejected(mk, arena, monkeypatch, entry):
    """A workspace one byte short of the size query: "workspace too small" from the host-side
    check, before any launch -- the outputs (0xFF-filled) are unchanged, the guards intact."""
    H = 5
    c = case("corner")
    g = c["g"]
    dt = (T(g.rp, DEV), T(g.col, DEV))
    sd, ss, cv, ci = dev_case(c, H)
    m, z = torch.zeros(H, g.R, device=DEV), torch.ones(H, g.R, device=DEV)
    torch.cuda.synchronize()
    shrunk = Shrunk(mk._L, {"attention": "maxk_gat_attention_heads_workspace_size",
                            "alpha": "maxk_gat_edge_alpha_heads_workspace_size"}[entry])
    monkeypatch.setattr(mk, "_L", shrunk)
    with arena.active("ones"):
        with pytest.raises(RuntimeError, match="workspace too small"):
            if entry == "attention":
                mk.gat_attention_heads(dt[0], dt[1], sd, ss, cv, ci, 256, SLOPE)
            else:
                mk.gat_edge_alpha_heads(dt[0], dt[1], sd, ss, m, z, SLOPE)
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
    g = c["g"]
    rp, col = dev_graph("corner")
    sd, ss, cv, ci = dev_case(c, H)
    for chunk in (0, 64):
        eager = mk.gat_attention_heads(rp, col, sd, ss, cv, ci, 256, SLOPE, chunk=chunk)
        eager_w = mk.gat_edge_alpha_heads(rp, col, sd, ss, eager[1], eager[2], SLOPE)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            sd2 = torch.zeros_like(sd)
            for _ in range(20):  # queued on the side stream before the call
                sd2 = sd2 + sd / 20
            sd2.copy_(sd)
            res = mk.gat_attention_heads(rp, col, sd2, ss, cv, ci, 256, SLOPE, chunk=chunk)
        side.synchronize()
        for x, y in zip(eager, res):
            assert M.same_bytes(x, y)
        out = torch.empty_like(eager[0])
        w = torch.empty_like(eager_w)
        hg = torch.cuda.CUDAGraph()
        stats = []
        with torch.cuda.graph(hg, stream=side):
            _, m, z = mk.gat_attention_heads(rp, col, sd, ss, cv, ci, 256, SLOPE, chunk=chunk,
                                             out=out, validate=False)
            mk.gat_edge_alpha_heads(rp, col, sd, ss, m, z, SLOPE, out=w, validate=False)
            stats += [m, z]
        for _ in range(2):
            for t in (out, w, *stats):
                t.fill_(float("nan"))
            hg.replay()
            torch.cuda.synchronize()
            for x, y in zip((*eager, eager_w), (out, *stats, w)):
                assert M.same_bytes(x, y)


# ------------------------------------------------------------------------------- autograd
def feat_grad_ref(g, a, G, ci, D):
    """grad of topk_values [C, k] in float64 with its bound: sum over heads and over the edges
    into c of alpha[h, e] G[h, row(e), ci[c, l]]; (n + 8) u sum|terms| plus the weight bound
    carried through, n = H times the in-degree where the selector is below D."""
    H = a.w.shape[0]
    C, k = ci.shape
    rows = ER.edge_rows(g.rp)
    sel = ci[g.col].astype(np.int64)
    ok = sel < D
    idx = (g.col[:, None].astype(np.int64) * k + np.arange(k)[None]).ravel()
    ref = np.zeros(C * k)
    s_abs = np.zeros(C * k)
    carried = np.zeros(C * k)
    for h in range(H):
        Gs = np.where(ok, G[h][rows[:, None], np.minimum(sel, D - 1)].astype(np.float64), 0.0)
        ref += np.bincount(idx, (a.w[h][:, None] * Gs).ravel(), minlength=C * k)
        s_abs += np.bincount(idx, np.abs(a.w[h][:, None] * Gs).ravel(), minlength=C * k)
        carried += np.bincount(idx, (a.w_bound[h][:, None] * np.abs(Gs)).ravel(),
                               minlength=C * k)
    n = H * np.bincount(idx, ok.ravel().astype(np.float64), minlength=C * k)
    bound = np.where(n > 0, (n + 8) * AR.U * s_abs + carried, 0.0)
    return ref.reshape(C, k), bound.reshape(C, k)


def test_autograd_matches_the_stored_path(mk, cuda, monkeypatch):
    """maxk_gat_attention_heads against gat_edge_softmax_heads followed by maxk_spgemm_heads,
    H = 3 on graph S with a random cotangent: the output inside the attention bound, the
    gradients of both scores inside the edge softmax reference's bounds chained with
    edge_grad_ref, the gradient of topk_values inside feat_grad_ref's; and the fused function
    saves no tensor of H * E or more elements, where the stored path saves alpha."""
    import maxk_layers as ML
    monkeypatch.setenv("MAXK_BWD_MODE", "csc")
    D, k, H = 64, 16, 3
    c = case("S", k, D)
    g, a = c["g"], AR.heads_slice(c["a"], H)
    E = g.col.size
    rng = np.random.default_rng(2700)
    G = np.stack([N.values(rng, (g.R, D), "unit") for _ in range(H)])
    rp, col = dev_graph("S")
    graph_ = ML.CSRGraph(rp, col)
    res, saved = {}, {}
    for path in ("fused", "stored"):
        sd, ss, tv, ci = dev_case(c, H)
        for t in (sd, ss, tv):
            t.requires_grad_(True)
        sizes = []
        with torch.autograd.graph.saved_tensors_hooks(
                lambda t: sizes.append(t.numel()) or t, lambda t: t):
            if path == "fused":
                y = graph_.attend_heads(tv, ci, D, sd, ss, SLOPE)
            else:
                y = graph_.aggregate_heads(tv, ci, D, ML.gat_edge_softmax_heads(graph_, sd, ss,
                                                                               SLOPE))
        y.backward(T(G, cuda))
        res[path] = (y.detach(), sd.grad, ss.grad, tv.grad)
        saved[path] = sizes
    assert saved["fused"] and max(saved["fused"]) < H * E, saved["fused"]
    assert max(saved["stored"]) >= H * E
    ers = [R.edge_grad_ref(g.rp, g.col, c["cv"], c["ci"], G[h], None) for h in range(H)]
    f = HS.HeadsFwd(a.heads, a.w, a.w_bound)
    b = HS.backward_heads(g.rp, g.col, f, np.stack([e.ref for e in ers]), SLOPE, g.C,
                          gw_bound=np.stack([R.bound(e) for e in ers]))
    gtv, gtv_bound = feat_grad_ref(g, a, G, c["ci"], D)
    for path in ("fused", "stored"):
        y, gsd, gss, gt = res[path]
        check(y, a.out, a.out_bound, f"autograd {path} out")
        check(gsd, b.g_dst, b.g_dst_bound, f"autograd {path} s_dst.grad")
        check(gss, b.g_src, b.g_src_bound, f"autograd {path} s_src.grad")
        check(gt, gtv, gtv_bound, f"autograd {path} topk_values.grad")


def test_multi_head_gat_conv_fused_matches_dense(cuda, monkeypatch):
    """MaxKMultiHeadGATConv(attention="fused") at V = 300, in = 64, out = 8, H = 4, k = 16
    against the same layer in dense float64 torch (masked dense softmax over the adjacency, per
    head), as test_heads_gpu.py::test_multi_head_gat_conv_matches_dense: the output, every
    parameter's gradient and both input gradients at rtol = atol = 1e-4; attention="stored" on
    the same parameters gives what it gave before (the same comparison), and MAXK_HEADS_ATTN
    overrides the argument.  HP = 4."""
    import maxk_cuda_kernels as mk_
    import maxk_layers as ML
    monkeypatch.delenv("MAXK_HEADS_ATTN", raising=False)
    torch.manual_seed(4)
    rng = np.random.default_rng(300)
    V, D, k, O_, H = 300, 64, 16, 8, 4
    rp, col = rand_graph(rng, V, 8, hubs=((7, 220),), empty=3)
    graph_ = ML.CSRGraph(T(rp.astype(np.int32), cuda), T(col.astype(np.int32), cuda))
    conv = ML.MaxKMultiHeadGATConv(D, O_, H, negative_slope=0.2, attention="fused").to(cuda)
    with torch.no_grad():
        conv.bias.normal_()
    x = torch.randn(V, D, device=cuda)
    xs, vals, idx = ML.maxk(x, k)
    xs = xs.detach().requires_grad_(True)
    vals = vals.detach().requires_grad_(True)
    gout = torch.randn(V, H, O_, device=cuda)
    names = ["fc.weight", "attn_src", "attn_dst", "bias"]
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
        Wh = Q["fc.weight"][h * O_:(h + 1) * O_]
        h_s = xs2 @ Wh.t()
        e = torch.nn.functional.leaky_relu(
            (h_s @ Q["attn_dst"][h])[:, None] + (h_s @ Q["attn_src"][h])[None, :], 0.2)
        alpha = torch.softmax(e.masked_fill(masked, float("-inf")), 1) * A
        heads.append(alpha @ (xv @ Wh.t()) + Q["bias"][h])
    ref = torch.stack(heads, 1)
    want = torch.autograd.grad(ref, [Q[n] for n in names] + [xs2, vals2], gout.double())
    empty = T(np.diff(rp) == 0, cuda)
    calls = []
    real = mk_.gat_attention_heads
    monkeypatch.setattr(mk_, "gat_attention_heads",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    for arg, env, fused in (("fused", None, True), ("stored", None, False),
                            ("stored", "fused", True), ("fused", "stored", False)):
        conv.attention = arg
        if env is None:
            monkeypatch.delenv("MAXK_HEADS_ATTN", raising=False)
        else:
            monkeypatch.setenv("MAXK_HEADS_ATTN", env)
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


def test_ratios_are_reported():
    """Last in the file: the largest err/bound ratios seen, for the record."""
    for what, r in sorted(RATIOS.items(), key=lambda kv: -kv[1])[:12]:
        print(f"{r:.3f}  {what}")
    assert all(r <= 1.0 for r in RATIOS.values())
