"""GPU: the fused backward of the multi-head GAT attention (gat_attention_heads_bwd.hip) through
the binding (mk.gat_attention_heads_backward), MaxKGATAttentionHeadsFunction(backward="fused")
and MaxKMultiHeadGATConv(attention="fused", attention_backward="fused"), against
tests/gat_attention_bwd_ref.py (float64, with its derived bounds), against the four calls it
replaces and against the rebuilt backward.

Which kernels.  Every non-empty call launches cbsr_pack_kernel or cbsr_pack4_kernel,
esmh_interleave_kernel<HP>, gath_bwd_kernel<KG, HP, 4>, esmh_merge_kernel, esmh_colsum_kernel<HP>
with its merge, and csc_sum_kernel with slab_fixup_kernel.  HP = 2, 2, 4, 8, 8 for H = 1, 2, 3,
5, 8; KG = 8 for k = 3, 7, 8, 16 for k = 16, 32 for k = 24, 32, 64 for k = 96 (the passes over
l: k > 64).  test_parity runs every (k, H) of SHAPES x HEADS: the twelve gath_bwd_kernel
instantiations.  The others run KG = 16 unless they say otherwise.

The inputs out, row_max and row_sum are either the float64 reference rounded to fp32 ("ref":
out_err = u |out|) or what mk.gat_attention_heads returned ("own": out_err = its out_bound).
The largest err / bound seen on an MI355X is in test_ratios_are_reported's output and in
profiles/r16/gat_attention_bwd/README.md.
"""
import functools

import numpy as np
import pytest
import torch

import edge_grad_ref as R
import esm_corner_graph as EG
import gat_attention_bwd_ref as BR
import gat_attention_ref as AR
import heads_softmax_ref as HS
import memguard as M
import numerics as N
from test_gat_attention_gpu import (DEV, HMAX, SLOPE, case, dev_case, dev_graph, feat_grad_ref,
                                    make_case, the_graph)
from test_memguard_gpu import Shrunk
from test_parity_gpu import T, rand_graph

pytestmark = pytest.mark.gpu

CHUNKS = (0,) + EG.CHUNKS
HEADS = (1, 2, 3, 5, 8)
SHAPES = [(3, 64), (8, 256), (16, 256), (32, 256), (24, 256), (96, 256), (7, 9)]
RATIOS: dict = {}
NAMES = ("grad_s_dst", "grad_s_src", "grad_cbsr")


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


# ------------------------------------------------------------------------------- shared data
def cotangent(c, seed=0):
    """G [HMAX, R, D]: the gradient of out."""
    g = c["g"]
    rng = np.random.default_rng(2900 + c["k"] + c["D"] + seed)
    return np.stack([N.values(rng, (g.R, c["D"]), "unit") for _ in range(HMAX)])


class Refs:
    """The references of one case and one G, at HMAX heads, for both regimes of `out`; the
    feature gradient per number of heads (it sums them)."""

    def __init__(self, c, G):
        self.c, self.G = c, G
        g, a = c["g"], c["a"]
        ers = BR.edge_grads(g, c["cv"], c["ci"], G)
        self.b = {"ref": BR.backward(g, a, c["cv"], c["ci"], G, SLOPE, c["D"],
                                     BR.rounded_out_err(a), ers=ers),
                  "own": BR.backward(g, a, c["cv"], c["ci"], G, SLOPE, c["D"], a.out_bound,
                                     ers=ers)}
        self.ers = ers

    @functools.lru_cache(maxsize=None)
    def feat(self, H):
        c = self.c
        with np.errstate(invalid="ignore", over="ignore"):
            return feat_grad_ref(c["g"], AR.heads_slice(c["a"], H), self.G[:H], c["ci"], c["D"])


@functools.lru_cache(maxsize=None)
def shared(name, k=16, D=256):
    """The case several tests share with its cotangent and references: computed once."""
    c = case(name, k, D)
    G = cotangent(c)
    return c, G, Refs(c, G)


def ref_forward(c, H):
    """out, row_max, row_sum of the float64 reference, rounded to fp32."""
    a = c["a"]
    with np.errstate(over="ignore", invalid="ignore"):
        return tuple(T(np.ascontiguousarray(x[:H]).astype(np.float32), DEV)
                     for x in (a.out, a.m, a.z))


def own_forward(mk, name, ops, D, chunk=0, dt=None):
    rp, col = dev_graph(name) if dt is None else dt
    sd, ss, cv, ci = ops
    return mk.gat_attention_heads(rp, col, sd, ss, cv, ci, D, SLOPE, chunk=chunk)


def run(mk, name, ops, fwd, G, chunk, dt=None, **kw):
    rp, col = dev_graph(name) if dt is None else dt
    sd, ss, cv, ci = ops
    out, m, z = fwd
    return mk.gat_attention_heads_backward(rp, col, sd, ss, cv, ci, out, m, z, G, SLOPE,
                                           chunk=chunk, **kw)


def check(y, ref, bound, what):
    assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape, (y.shape, ref.shape)
    r = N.within(y, ref, bound, what)
    RATIOS[what] = r
    print(f"{what}: err/bound {r:.3f}")
    return r


def check_all(c, H, res, b, feat, what):
    """The three gradients inside their bounds, no element excluded; exact zeros where nothing
    is added: a row without edges, an unread column, a selector >= D."""
    g = c["g"]
    g_dst, g_src, g_cbsr = res
    check(g_dst, b.g_dst[:H], b.g_dst_bound[:H], f"{what} grad_s_dst")
    check(g_src, b.g_src[:H], b.g_src_bound[:H], f"{what} grad_s_src")
    check(g_cbsr, feat[0], feat[1], f"{what} grad_cbsr")
    assert not g_dst[:, T(np.diff(g.rp) == 0, DEV)].any()
    if g.unread is not None:
        assert not g_src[:, g.unread].any() and not g_cbsr[g.unread].any()
    if bool(np.isfinite(feat[0]).all()):
        assert not g_cbsr[T(c["ci"] >= c["D"], DEV)].any()


# ------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("k,D", SHAPES, ids=[f"k{k}-D{D}" for k, D in SHAPES])
@pytest.mark.parametrize("name", ["S", "Dn", "R"])
def test_parity(mk, cuda, name, k, D):
    """The three gradients inside the derived bounds for H in 1, 2, 3, 5, 8 at the auto item
    size and at 64 tokens, with the reference's forward results and with the kernel's own.
    Every gath_bwd_kernel instantiation (see the module text)."""
    c = make_case(name, k, D)
    G = cotangent(c)
    refs = Refs(c, G)
    for H in HEADS:
        ops = dev_case(c, H)
        Gd = T(np.ascontiguousarray(G[:H]), DEV)
        fwd = {"ref": ref_forward(c, H), "own": own_forward(mk, name, ops, D)}
        for regime in ("ref", "own"):
            for chunk in (0, 64):
                check_all(c, H, run(mk, name, ops, fwd[regime], Gd, chunk), refs.b[regime],
                          refs.feat(H), f"{name} k{k} D{D} H{H} {regime} chunk {chunk}")


# ------------------------------------------------------------------------------- cut rows
@pytest.mark.parametrize("H", [3, 8])
@pytest.mark.parametrize("name", ["corner", "transpose"])
def test_cut_rows(mk, cuda, name, H):
    """Rows of 32 / 33 and 512 / 513 edges, the hub of 1700, empty rows first, in a run and last,
    at the auto item size and every entry of EG.CHUNKS (1 token to more than the graph): the
    pieces' slots and their merge, the cut columns of both CSC sums."""
    c, G, refs = shared(name)
    ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    fwd = own_forward(mk, name, ops, 256)
    for chunk in CHUNKS:
        res = run(mk, name, ops, fwd, Gd, chunk)
        assert all(bool(torch.isfinite(t).all()) for t in res)
        check_all(c, H, res, refs.b["own"], refs.feat(H), f"{name} H{H} chunk {chunk}")


@pytest.mark.parametrize("H", [3, 8])
def test_cut_rows_far_apart_maxima(mk, cuda, H):
    """The hub row's source scores ramp from -50 to 150 along its edges (the case of
    test_gat_attention_gpu.py): the coefficients come from the row's statistics, so the pieces
    need no rescaling; everything finite and inside the bounds."""
    g = the_graph("corner")
    base = case("corner")
    lo, hi = g.rp[g.hub], g.rp[g.hub + 1]
    s_src = base["s_src"].copy()
    s_src[:, g.col[lo:hi]] += np.linspace(-50, 150, hi - lo, dtype=np.float32)[None]
    c = make_case("corner", 16, 256, scores=(base["s_dst"], s_src), ci=base["ci"])
    G = cotangent(c)
    refs = Refs(c, G)
    ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    fwd = own_forward(mk, "corner", ops, 256)
    for chunk in (0, 64, 67, 512, 513):
        res = run(mk, "corner", ops, fwd, Gd, chunk)
        assert all(bool(torch.isfinite(t).all()) for t in res)
        check_all(c, H, res, refs.b["own"], refs.feat(H), f"far maxima H{H} chunk {chunk}")
        assert bool(res[0][:, g.hub].abs().max() > 0)


# ------------------------------------------------------------------------------- composition
@pytest.mark.parametrize("H", [2, 5])
@pytest.mark.parametrize("name,k,D", [("S", 16, 256), ("Dn", 32, 256), ("R", 7, 9)])
def test_against_the_four_calls_it_replaces(mk, cuda, name, k, D, H):
    """gat_edge_alpha_heads -> edge_weight_grad_heads -> gat_edge_softmax_heads_backward ->
    sspmm_backward_heads on the same inputs: each result differs from the fused call's by at
    most the sum of both paths' bounds (the stored path's: the edge softmax reference's
    backward with the edge gradient's bound carried, and feat_grad_ref)."""
    c = make_case(name, k, D)
    g, a = c["g"], AR.heads_slice(c["a"], H)
    G = cotangent(c)
    refs = Refs(c, G)
    st = HS.backward_heads(g.rp, g.col, HS.HeadsFwd(a.heads, a.w, a.w_bound),
                           np.stack([e.ref for e in refs.ers[:H]]), SLOPE, g.C,
                           gw_bound=np.stack([R.bound(e) for e in refs.ers[:H]]))
    rp, col = dev_graph(name)
    sd, ss, cv, ci = ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    out, m, z = fwd = own_forward(mk, name, ops, D)
    b, feat = refs.b["own"], refs.feat(H)
    for chunk in (0, 64):
        fused = run(mk, name, ops, fwd, Gd, chunk)
        alpha = mk.gat_edge_alpha_heads(rp, col, sd, ss, m, z, SLOPE)
        gw = mk.edge_weight_grad_heads(rp, col, cv, ci, Gd, chunk=chunk)
        s_dst_, s_src_ = mk.gat_edge_softmax_heads_backward(rp, col, sd, ss, alpha, gw, SLOPE,
                                                            chunk=chunk)
        cb = mk.sspmm_backward_heads(rp, col, alpha, Gd, ci, chunk=chunk)
        for x, y, both, what in (
                (fused[0], s_dst_, b.g_dst_bound[:H] + st.g_dst_bound, "grad_s_dst"),
                (fused[1], s_src_, b.g_src_bound[:H] + st.g_src_bound, "grad_s_src"),
                (fused[2], cb, 2 * feat[1], "grad_cbsr")):
            err = (x.double() - y.double()).abs().cpu().numpy()
            assert (err <= both).all(), (what, chunk, float((err / np.maximum(both, 1e-300)).max()))


# ------------------------------------------------------------------------------- selectors
@pytest.mark.parametrize("k,D", [(16, 100), (5, 24)])
def test_skipped_and_repeated_selectors(mk, cuda, k, D):
    """Selectors >= D (their slots get an exact 0) and repeated inside a vertex (the pack folds
    the values; each slot still receives the column's gradient).  KG = 16 and 8, HP = 4."""
    g = the_graph("S")
    rng = np.random.default_rng(2500 + k)
    ci = N.selectors(rng, g.C, 256, k)  # selectors up to 255: many >= D
    dup = rng.choice(g.C, g.C // 4, replace=False)
    ci[dup, k - 1] = ci[dup, 0]
    c = make_case("S", k, D, ci=ci)
    assert (ci >= D).any() and (c["n"] == 0).any()
    G = cotangent(c)
    refs = Refs(c, G)
    ops = dev_case(c, 3)
    Gd = T(np.ascontiguousarray(G[:3]), DEV)
    fwd = {"ref": ref_forward(c, 3),
           "own": mk.gat_attention_heads(*dev_graph("S"), *ops, D, SLOPE, validate=False)}
    for regime in ("ref", "own"):
        for chunk in (0, 64):
            res = run(mk, "S", ops, fwd[regime], Gd, chunk, validate=False)
            check_all(c, 3, res, refs.b[regime], refs.feat(3), f"selectors k{k} D{D} {regime}")
            kept = dup[ci[dup, 0] < D]
            assert M.same_bytes(res[2][T(kept, DEV), k - 1].contiguous(),
                                res[2][T(kept, DEV), 0].contiguous())


# ------------------------------------------------------------------------------- non-finite
def test_non_finite(mk, cuda):
    """Head 1 of 3 on graph S.  A NaN in s_src[1, c] reaches head 1's grad_s_dst rows that read
    c, the grad_s_src columns those rows read and grad_cbsr of those columns (the reference's
    masks, by N.same_class); a -Inf in s_src at a vertex whose readers have other neighbours
    gives gz = 0: its grad_s_src is an exact 0; heads 0 and 2 keep the bytes of their score
    gradients.  A NaN of grad_out in every column a row does not select reaches nothing: the
    bytes of the clean run."""
    H = 3
    c, G, refs = shared("S")
    g = c["g"]
    deg = np.diff(g.rp)
    readers = N._readers(g)
    # a column no hub row reads (a hub row reads nearly every column, and would carry the NaN to
    # nearly all of grad_s_src), and one whose readers are other rows with other neighbours
    hubs = np.flatnonzero(deg > 100)
    nan_col = next(int(v) for v in range(g.C)
                   if readers[v].size >= 2 and not np.isin(readers[v], hubs).any())
    ninf_col = next(int(v) for v in range(g.C)
                    if v != nan_col and readers[v].size >= 2 and (deg[readers[v]] >= 2).all()
                    and not np.isin(readers[v], readers[nan_col]).any())
    s_dst, s_src = c["s_dst"][:H].copy(), c["s_src"][:H].copy()
    s_src[1, nan_col] = np.nan
    s_src[1, ninf_col] = -np.inf
    a = AR.attention(g.rp, g.col, s_dst, s_src, SLOPE, c["cv"], c["ci"], 256, c["n"])
    p = dict(c, a=a)
    b = BR.backward(g, a, c["cv"], c["ci"], G[:H], SLOPE, 256, a.out_bound, ers=refs.ers[:H])
    with np.errstate(invalid="ignore", over="ignore"):
        feat = feat_grad_ref(g, a, G[:H], c["ci"], 256)
    hit = readers[nan_col]
    assert np.isnan(b.g_dst[1, hit]).all() and np.isfinite(b.g_dst[[0, 2]]).all()
    assert np.isnan(b.g_src[1, nan_col]) and np.isnan(feat[0][nan_col]).all()
    assert b.g_src[1, ninf_col] == 0 and np.isfinite(b.g_src[1]).mean() > 0.3
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    G2 = G[:H].copy()
    G2[:, c["n"] == 0] = np.nan
    assert np.isnan(G2).any()
    for chunk in (0, 64):
        ops = dev_case(c, H)
        fwd = own_forward(mk, "S", ops, 256, chunk)
        clean = run(mk, "S", ops, fwd, Gd, chunk)
        ops_p = dev_case(c, H, s_dst, s_src)
        res = run(mk, "S", ops_p, own_forward(mk, "S", ops_p, 256, chunk), Gd, chunk)
        check_all(p, H, res, b, feat, f"non-finite chunk {chunk}")
        assert not res[1][1, ninf_col].any()  # exactly 0
        for x, y in zip(clean[:2], res[:2]):
            for h in (0, 2):
                assert M.same_bytes(x[h].contiguous(), y[h].contiguous()), (chunk, h)
        nan_g = run(mk, "S", ops, fwd, T(G2, DEV), chunk)
        for x, y in zip(clean, nan_g):
            assert M.same_bytes(x, y), chunk


@pytest.mark.parametrize("H,h", [(3, 1), (8, 6), (5, 0)])
def test_head_isolation(mk, cuda, H, h):
    """The other heads' scores (and with them their out, row_max and row_sum) replaced by other
    numbers: head h's grad_s_dst and grad_s_src keep their bytes.  HP = 4 and 8."""
    c, G, _ = shared("corner")
    rng = np.random.default_rng(2600 + H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    for chunk in (0, 64, 7):
        ops = dev_case(c, H)
        base = run(mk, "corner", ops, own_forward(mk, "corner", ops, 256, chunk), Gd, chunk)
        arrs = []
        for name in ("s_dst", "s_src"):
            x = rng.standard_normal(c[name][:H].shape).astype(np.float32)
            x[h] = c[name][h]
            arrs.append(x)
        ops2 = dev_case(c, H, *arrs)
        other = run(mk, "corner", ops2, own_forward(mk, "corner", ops2, 256, chunk), Gd, chunk)
        for x, y in zip(base[:2], other[:2]):
            assert M.same_bytes(x[h].contiguous(), y[h].contiguous()), chunk
        assert not M.same_bytes(base[2], other[2])  # grad_cbsr sums the heads


# ------------------------------------------------------------------------------- degenerate
@pytest.mark.parametrize("H", [1, 3, 8])
def test_no_edges(mk, cuda, H):
    """num_e == 0: zeros in all three gradients."""
    rows, cols, D, k = 40, 17, 64, 8
    rp = torch.zeros(rows + 1, dtype=torch.int32, device=cuda)
    col = torch.empty(0, dtype=torch.int32, device=cuda)
    sd, ss = torch.randn(H, rows, device=cuda), torch.randn(H, cols, device=cuda)
    cv = torch.randn(cols, k, device=cuda)
    ci = torch.zeros(cols, k, dtype=torch.uint8, device=cuda)
    out, m, z = mk.gat_attention_heads(rp, col, sd, ss, cv, ci, D)
    G = torch.randn(H, rows, D, device=cuda)
    junk = [torch.full((n,), float("nan"), device=cuda) for n in (H * rows, H * cols, cols * k)]
    del junk
    res = mk.gat_attention_heads_backward(rp, col, sd, ss, cv, ci, out, m, z, G)
    assert [tuple(t.shape) for t in res] == [(H, rows), (H, cols), (cols, k)]
    for t in res:
        assert not t.any() and not torch.isnan(t).any()


# ------------------------------------------------------------------------------- bitwise
@pytest.mark.parametrize("name", ["corner", "S"])
def test_bitwise_repeatable(mk, cuda, name):
    """Runs at H = 5 (HP = 8) with the allocator's free blocks (where the next workspace comes
    from) filled with 0x00 and with 0xFF before each: the same bytes."""
    H = 5
    c, G, _ = shared(name)
    g = c["g"]
    ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    fwd = own_forward(mk, name, ops, 256)
    for chunk in (0, 7, 64):
        n_ws = mk._lib().maxk_gat_attention_heads_backward_workspace_size(
            g.R, g.C, g.col.size, 256, 16, H, chunk)
        runs = []
        for fill in (0x00, 0xFF):
            junk = [torch.full((n,), fill, dtype=torch.uint8, device=cuda)
                    for n in (n_ws, n_ws // 2, 4 * H * g.R, 4 * g.C * 16, 4096)]
            del junk
            runs.append(run(mk, name, ops, fwd, Gd, chunk))
        for x, y in zip(*runs):
            assert M.same_bytes(x, y)


# ------------------------------------------------------------------------------- memory
@pytest.fixture(scope="module")
def arena(cuda):
    return M.Arena(48 << 20, cuda)


@pytest.mark.parametrize("k,D,H", [(16, 256, 3), (16, 256, 8), (3, 64, 3)])
def test_memory_contract(mk, arena, cuda, k, D, H):
    """Outputs and workspace from the poisoned, guarded arena (the workspace exactly the queried
    size): outputs fully written and the same bytes in every fill regime, guards untouched,
    inputs unchanged.  KG = 16 and 8, HP = 4 and 8."""
    c, G, refs = shared("corner", k, D)
    g = c["g"]
    E = g.col.size
    fwd = own_forward(mk, "corner", dev_case(c, H), D)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    for chunk in (0, 64):
        def factory(primer):
            dt = (T(g.rp, DEV), T(g.col, DEV))
            plan = mk.transpose_plan(dt[1], g.C, cache=False)
            ops = dev_case(c, H)
            rest = tuple(t.clone() for t in fwd) + (Gd.clone(),)
            if primer:
                gen = torch.Generator(device=DEV).manual_seed(5)
                ops = tuple(torch.rand(t.shape, generator=gen, device=DEV) for t in ops[:3]) \
                    + (ops[3],)
                rest = tuple(torch.rand(t.shape, generator=gen, device=DEV) + 0.5 for t in rest)
            return (dt, plan) + ops + rest

        def op(dt, plan, sd, ss, cv, ci, out, m, z, G_):
            return mk.gat_attention_heads_backward(dt[0], dt[1], sd, ss, cv, ci, out, m, z, G_,
                                                   SLOPE, chunk=chunk, plan=plan)

        res = M.run_regimes(op, factory, arena)
        n_ws = mk._lib().maxk_gat_attention_heads_backward_workspace_size(g.R, g.C, E, D, k, H,
                                                                          chunk)
        assert sorted(x.nbytes for x in arena.allocs) == sorted(
            [4 * H * g.R, 4 * H * g.C, 4 * g.C * k, n_ws])
        for regime in ("stale", "ones"):
            for x, y in zip(res["zero"], res[regime]):
                assert M.same_bytes(x, y), regime
        check_all(c, H, res["ones"], refs.b["own"], refs.feat(H),
                  f"memguard k{k} D{D} H{H} chunk {chunk}")


def test_undersized_workspace_is_rejected(mk, arena, monkeypatch):
    """A workspace one byte short of the size query: "workspace too small" from the host-side
    check, before any launch -- the outputs (0xFF-filled) are unchanged, the guards intact."""
    H = 5
    c, G, _ = shared("corner")
    g = c["g"]
    dt = (T(g.rp, DEV), T(g.col, DEV))
    plan = mk.transpose_plan(dt[1], g.C, cache=False)
    ops = dev_case(c, H)
    fwd = own_forward(mk, "corner", ops, 256, dt=dt)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    torch.cuda.synchronize()
    shrunk = Shrunk(mk._L, "maxk_gat_attention_heads_backward_workspace_size")
    monkeypatch.setattr(mk, "_L", shrunk)
    with arena.active("ones"):
        with pytest.raises(RuntimeError, match="workspace too small"):
            run(mk, "corner", ops, fwd, Gd, 0, dt=dt, plan=plan)
        made = len(arena.allocs)
    assert shrunk.sizes and all(n > 1 for n in shrunk.sizes), shrunk.sizes
    assert made >= 4  # the outputs and the short workspace came from the arena
    arena.check()
    assert arena.untouched()


# ------------------------------------------------------------------------------- streams
def test_runs_on_the_current_stream_and_captures(mk, cuda):
    """On a side stream made current the call is ordered after work queued there before it; one
    hipGraph capture of the forward followed by the backward -- a single chain of kernels --
    replayed twice equals the eager result bitwise.  H = 3."""
    H = 3
    c, G, _ = shared("corner")
    g = c["g"]
    rp, col = dev_graph("corner")
    plan = mk.transpose_plan(col, g.C)
    sd, ss, cv, ci = ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    for chunk in (0, 64):
        fwd = own_forward(mk, "corner", ops, 256, chunk)
        eager = run(mk, "corner", ops, fwd, Gd, chunk)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            G2 = torch.zeros_like(Gd)
            for _ in range(20):  # queued on the side stream before the call
                G2 = G2 + Gd / 20
            G2.copy_(Gd)
            res = run(mk, "corner", ops, fwd, G2, chunk)
        side.synchronize()
        for x, y in zip(eager, res):
            assert M.same_bytes(x, y)
        hg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(hg, stream=side):
            f2 = mk.gat_attention_heads(rp, col, sd, ss, cv, ci, 256, SLOPE, chunk=chunk,
                                        validate=False)
            got = mk.gat_attention_heads_backward(rp, col, sd, ss, cv, ci, *f2, Gd, SLOPE,
                                                  chunk=chunk, validate=False, plan=plan)
        for _ in range(2):
            for t in (*f2, *got):
                t.fill_(float("nan"))
            hg.replay()
            torch.cuda.synchronize()
            for x, y in zip((*fwd, *eager), (*f2, *got)):
                assert M.same_bytes(x, y)


# ------------------------------------------------------------------------------- autograd
def test_autograd_fused_backward(mk, cuda, monkeypatch):
    """maxk_gat_attention_heads(backward="fused") against backward="rebuilt" and the references,
    H = 3 on graph S: the fused function saves `out` (and only then), its backward is one
    gat_attention_heads_backward call that allocates the three gradients and a workspace of the
    queried size and no float tensor of H * E elements, where the rebuilt one allocates alpha
    and grad_w.  It falls back to the rebuilt backward when a gradient is not needed and when
    MAXK_BWD_MODE forces a mode."""
    import maxk_layers as ML
    monkeypatch.delenv("MAXK_BWD_MODE", raising=False)
    monkeypatch.delenv("MAXK_HEADS_ATTN_BWD", raising=False)
    D, k, H = 64, 16, 3
    c, G, refs = shared("S", k, D)
    g = c["g"]
    E = g.col.size
    rp, col = dev_graph("S")
    graph_ = ML.CSRGraph(rp, col)
    mk.transpose_plan(col, g.C)  # cached: not an allocation of the backward
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    calls = []
    for fn in ("gat_attention_heads_backward", "gat_edge_alpha_heads", "edge_weight_grad_heads"):
        real = getattr(mk, fn)
        monkeypatch.setattr(mk, fn, lambda *a, _r=real, _n=fn, **kw: calls.append(_n) or
                            _r(*a, **kw))
    real_empty = torch.empty
    res, saved, allocs = {}, {}, {}

    def run_path(path, need=(True, True, True), **kw):
        sd, ss, tv, ci = dev_case(c, H)
        for t, n in zip((sd, ss, tv), need):
            t.requires_grad_(n)
        sizes = []
        with torch.autograd.graph.saved_tensors_hooks(
                lambda t: sizes.append(tuple(t.shape)) or t, lambda t: t):
            y = graph_.attend_heads(tv, ci, D, sd, ss, SLOPE, **kw)
        made = []

        def empty(*a, **k_):
            t = real_empty(*a, **k_)
            made.append((t.dtype, t.numel()))
            return t
        del calls[:]
        monkeypatch.setattr(torch, "empty", empty)
        y.backward(Gd)
        monkeypatch.setattr(torch, "empty", real_empty)
        res[path] = (y.detach(), sd.grad, ss.grad, tv.grad)
        saved[path], allocs[path] = sizes, made
        return list(calls)

    assert run_path("fused", backward="fused") == ["gat_attention_heads_backward"]
    assert "gat_attention_heads_backward" not in run_path("rebuilt")
    assert (H, g.R, D) in saved["fused"] and (H, g.R, D) not in saved["rebuilt"]
    assert len(saved["fused"]) == len(saved["rebuilt"]) + 1
    assert all(int(np.prod(s)) < H * E for s in saved["fused"] if s != (H, g.R, D))
    n_ws = mk._lib().maxk_gat_attention_heads_backward_workspace_size(g.R, g.C, E, D, k, H, 0)
    f32 = [n for dt, n in allocs["fused"] if dt == torch.float32]
    assert sorted(f32) == sorted([H * g.R, H * g.C, g.C * k]) and max(f32) < H * E
    assert [n for dt, n in allocs["fused"] if dt == torch.uint8] == [n_ws]
    assert sum(n == H * E for dt, n in allocs["rebuilt"] if dt == torch.float32) >= 2
    b, feat = refs.b["own"], refs.feat(H)
    a = AR.heads_slice(c["a"], H)
    for path in ("fused", "rebuilt"):
        y, gsd, gss, gt = res[path]
        check(y, a.out, a.out_bound, f"autograd {path} out")
        check(gsd, b.g_dst[:H], b.g_dst_bound[:H], f"autograd {path} s_dst.grad")
        check(gss, b.g_src[:H], b.g_src_bound[:H], f"autograd {path} s_src.grad")
        check(gt, feat[0], feat[1], f"autograd {path} topk_values.grad")
    # the fallbacks, and the environment's override of the argument
    assert "gat_attention_heads_backward" not in run_path("partial", (True, True, False),
                                                          backward="fused")
    assert M.same_bytes(res["partial"][1], res["rebuilt"][1])
    monkeypatch.setenv("MAXK_BWD_MODE", "csc")
    assert "gat_attention_heads_backward" not in run_path("forced", backward="fused")
    monkeypatch.delenv("MAXK_BWD_MODE")
    monkeypatch.setenv("MAXK_HEADS_ATTN_BWD", "fused")
    assert run_path("env") == ["gat_attention_heads_backward"]
    monkeypatch.setenv("MAXK_HEADS_ATTN_BWD", "rebuilt")
    assert "gat_attention_heads_backward" not in run_path("env2", backward="fused")
    for x, y in zip(res["env"], res["fused"]):
        assert M.same_bytes(x, y)


def test_multi_head_gat_conv_fused_backward_matches_dense(cuda, monkeypatch):
    """MaxKMultiHeadGATConv(attention="fused", attention_backward="fused") at V = 300, in = 64,
    out = 8, H = 4, k = 16 against the same layer in dense float64 torch, as
    test_gat_attention_gpu.py::test_multi_head_gat_conv_fused_matches_dense: the output, every
    parameter's gradient and both input gradients at rtol = atol = 1e-4; MAXK_HEADS_ATTN_BWD
    overrides the argument, and it has no effect where the attention is "stored"."""
    import maxk_cuda_kernels as mk_
    import maxk_layers as ML
    monkeypatch.delenv("MAXK_HEADS_ATTN", raising=False)
    monkeypatch.delenv("MAXK_HEADS_ATTN_BWD", raising=False)
    monkeypatch.delenv("MAXK_BWD_MODE", raising=False)
    torch.manual_seed(4)
    rng = np.random.default_rng(300)
    V, D, k, O_, H = 300, 64, 16, 8, 4
    rp, col = rand_graph(rng, V, 8, hubs=((7, 220),), empty=3)
    graph_ = ML.CSRGraph(T(rp.astype(np.int32), cuda), T(col.astype(np.int32), cuda))
    conv = ML.MaxKMultiHeadGATConv(D, O_, H, negative_slope=0.2, attention="fused",
                                   attention_backward="fused").to(cuda)
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
    calls = []
    real = mk_.gat_attention_heads_backward
    monkeypatch.setattr(mk_, "gat_attention_heads_backward",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    for attn, arg, env, fused in (("fused", "fused", None, True), ("fused", "rebuilt", None, False),
                                  ("fused", "rebuilt", "fused", True),
                                  ("fused", "fused", "rebuilt", False),
                                  ("stored", "fused", "fused", False)):
        conv.attention, conv.attention_backward = attn, arg
        if env is None:
            monkeypatch.delenv("MAXK_HEADS_ATTN_BWD", raising=False)
        else:
            monkeypatch.setenv("MAXK_HEADS_ATTN_BWD", env)
        del calls[:]
        out = conv(graph_, xs, vals, idx)
        got = torch.autograd.grad(out, [P[n] for n in names] + [xs, vals], gout)
        assert len(calls) == (1 if fused else 0), (attn, arg, env)
        torch.testing.assert_close(out, ref.float(), rtol=1e-4, atol=1e-4)
        for n, a, b in zip(names + ["x_sparse", "topk_values"], got, want):
            torch.testing.assert_close(a, b.float(), rtol=1e-4, atol=1e-4,
                                       msg=lambda m: f"{attn} {arg} {env} {n}: {m}")


def test_ratios_are_reported():
    """Last in the file: the largest err/bound ratios seen per output, for the record."""
    for out in NAMES:
        rs = {w: r for w, r in RATIOS.items() if w.endswith(out)}
        if rs:
            w = max(rs, key=rs.get)
            print(f"{out}: largest err/bound {rs[w]:.3f} ({w})")
    assert all(r <= 1.0 for r in RATIOS.values())
