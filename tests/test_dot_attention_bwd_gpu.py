"""GPU: the fused backward of the multi-head dot-product attention on CBSR keys
(dot_attention_heads_bwd.hip) through the binding (mk.dot_attention_heads_backward),
MaxKDotAttentionHeadsFunction(backward="fused") and MaxKTransformerConv(attention="fused",
attention_backward="fused"), against tests/dot_attention_bwd_ref.py (float64, with its derived
bounds), against the sequence of calls it replaces and against dense float64 torch.

Which kernels.  Every non-empty call launches cbsr_pack_kernel or cbsr_pack4_kernel,
datb_walk_kernel<KG, HP, 4> (walk A), datb_gq_kernel<KG, 8> (aggregation B) with
slab_fixup_kernel<0> per head, and csc_sum_kernel with slab_fixup_kernel<1>.  HP = 2, 2, 4, 8, 8
for H = 1, 2, 3, 5, 8; KG = 8 for k = 3, 7, 8, 16 for k = 16, 32 for k = 24, 32, 64 for k = 96
(the passes over l: k > 64).  B's heads per pass are HC = ceil(H / ceil(H / G)), G = 64 / KG, as
in test_dot_attention_gpu.py.  test_parity runs every (k, H) of SHAPES x HEADS at both scales: the
twelve datb_walk_kernel instantiations and the four datb_gq_kernel ones with one and several
passes, full and partly filled last passes and idle groups.  The others run KG = 16 unless they
say otherwise; test_cut_rows reaches walk A's item ends, B's hub slabs and their sum and the cut
columns of the CSC sum.

The inputs out, row_max and row_sum are either the float64 reference rounded to fp32 ("ref":
out_err = u |out|) or what mk.dot_attention_heads returned ("own": out_err = its out_bound).
The largest err / bound seen on an MI355X is in test_ratios_are_reported's output and in
profiles/r20/dot_attention_bwd/README.md.
"""
import functools
import types

import numpy as np
import pytest
import torch

import dot_attention_bwd_ref as BR
import dot_attention_ref as DR
import edge_grad_ref as R
import edge_softmax_ref as ER
import esm_corner_graph as EG
import memguard as M
import numerics as N
import test_dot_attention_gpu as DG
import test_gat_attention_gpu as GA
from test_dot_attention_gpu import DEV, HMAX, case, dev_case, dev_graph, make_case, the_graph
from test_memguard_gpu import Shrunk
from test_parity_gpu import T, rand_graph

pytestmark = pytest.mark.gpu

CHUNKS = (0,) + EG.CHUNKS
HEADS = (1, 2, 3, 5, 8)
SCALES = (1.0, 0.125)
SHAPES = [(3, 64), (8, 256), (16, 256), (32, 256), (24, 256), (96, 256), (7, 9)]
RATIOS: dict = {}
NAMES = ("grad_q", "grad_cbsr")


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


# ------------------------------------------------------------------------------- shared data
def cotangent(c, seed=0):
    """G [HMAX, R, D]: the gradient of out."""
    g = c["g"]
    rng = np.random.default_rng(3100 + c["k"] + c["D"] + seed)
    return np.stack([N.values(rng, (g.R, c["D"]), "unit") for _ in range(HMAX)])


class Refs:
    """The references of one case and one G, at the case's heads, for both regimes of `out`;
    the feature gradient per number of heads (it sums them)."""

    def __init__(self, c, G, H=HMAX, regimes=("ref", "own")):
        self.c, self.G = c, G
        g, a = c["g"], DR.heads_slice(c["a"], H)
        self.ers = BR.edge_grads(g, c["cv"], c["ci"], G[:H])
        err = {"ref": BR.rounded_out_err(a), "own": a.out_bound}
        self.b, base = {}, None
        for r in regimes:  # the values are computed once, the bounds per regime
            self.b[r] = base = BR.backward(g, a, c["q"][:H], c["scale"], c["cv"], c["ci"], G[:H],
                                           c["D"], err[r], c["n"], ers=self.ers, base=base)

    @functools.lru_cache(maxsize=None)
    def feat(self, regime, H):
        return BR.cbsr(self.b[regime], H)


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


def own_forward(mk, name, ops, c, chunk=0, dt=None, **kw):
    return DG.run(mk, name, ops, c, chunk, dt=dt, **kw)


def run(mk, name, ops, c, fwd, G, chunk, dt=None, **kw):
    rp, col = dev_graph(name) if dt is None else dt
    q, cv, ci = ops
    out, m, z = fwd
    return mk.dot_attention_heads_backward(rp, col, q, cv, ci, out, m, z, G, c["scale"],
                                           chunk=chunk, **kw)


def check(y, ref, bound, what):
    assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape, (y.shape, ref.shape)
    r = N.within(y, ref, bound, what)
    RATIOS[what] = r
    print(f"{what}: err/bound {r:.3f}")
    return r


def check_all(c, H, res, b, feat, what):
    """Both gradients inside their bounds, no element excluded; exact zeros where nothing is
    added: a row without edges, a column of grad_q no neighbour selects, an unread column of the
    table, a selector >= D."""
    g = c["g"]
    g_q, g_cbsr = res
    check(g_q, b.g_q[:H], b.g_q_bound[:H], f"{what} grad_q")
    check(g_cbsr, feat[0], feat[1], f"{what} grad_cbsr")
    assert not g_q[:, T(np.diff(g.rp) == 0, DEV)].any()
    assert not g_q[:, T(c["n"] == 0, DEV)].any()
    if g.unread is not None:
        assert not g_cbsr[g.unread].any()
    if bool(np.isfinite(feat[0]).all()):
        assert not g_cbsr[T(c["ci"] >= c["D"], DEV)].any()


# ------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("k,D", SHAPES, ids=[f"k{k}-D{D}" for k, D in SHAPES])
@pytest.mark.parametrize("name", ["S", "Dn", "R"])
def test_parity(mk, cuda, name, k, D, scale):
    """Both gradients inside the derived bounds for H in 1, 2, 3, 5, 8 at the auto item size and
    at 64 tokens, with the reference's forward results and with the kernel's own.  Every
    datb_walk_kernel and datb_gq_kernel instantiation (see the module text)."""
    c = make_case(name, k, D, scale)
    G = cotangent(c)
    refs = Refs(c, G)
    for H in HEADS:
        ops = dev_case(c, H)
        Gd = T(np.ascontiguousarray(G[:H]), DEV)
        fwd = {"ref": ref_forward(c, H), "own": own_forward(mk, name, ops, c)}
        for regime in ("ref", "own"):
            for chunk in (0, 64):
                check_all(c, H, run(mk, name, ops, c, fwd[regime], Gd, chunk), refs.b[regime],
                          refs.feat(regime, H),
                          f"{name} k{k} D{D} s{scale} H{H} {regime} chunk {chunk}")


# ------------------------------------------------------------------------------- cut rows
@pytest.mark.parametrize("H", [3, 8])
@pytest.mark.parametrize("name", ["corner", "transpose"])
def test_cut_rows(mk, cuda, name, H):
    """Rows of 32 / 33 and 512 / 513 edges, the hub of 1700, empty rows first, in a run and last,
    at the auto item size and every entry of EG.CHUNKS (1 token to more than the graph): walk A's
    item ends, B's hub slabs and their sum, the cut columns of the CSC sum.  "transpose":
    num_rows != num_cols."""
    c, G, refs = shared(name)
    assert name != "transpose" or c["g"].R != c["g"].C
    ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    fwd = own_forward(mk, name, ops, c)
    for chunk in CHUNKS:
        res = run(mk, name, ops, c, fwd, Gd, chunk)
        assert all(bool(torch.isfinite(t).all()) for t in res)
        check_all(c, H, res, refs.b["own"], refs.feat("own", H), f"{name} H{H} chunk {chunk}")


@pytest.mark.parametrize("H", [3, 8])
def test_cut_rows_wide_logits(mk, cuda, H):
    """The hub row's queries are scaled up so its logits spread over more than 160 (the case of
    test_dot_attention_gpu.py): the coefficients come from the row's statistics, so no piece
    needs rescaling; everything finite and inside the bounds."""
    g = the_graph("corner")
    base = case("corner")
    q = base["q"].copy()
    q[:, g.hub] *= 8.0
    c = make_case("corner", 16, 256, 1.0, q=q, ci=base["ci"])
    lo, hi = g.rp[g.hub], g.rp[g.hub + 1]
    l = c["a"].l[0, lo:hi]
    assert l.max() - l.min() > 160
    G = cotangent(c)
    refs = Refs(c, G, H, ("own",))
    ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    fwd = own_forward(mk, "corner", ops, c)
    for chunk in (0, 64, 67, 512, 513):
        res = run(mk, "corner", ops, c, fwd, Gd, chunk)
        assert all(bool(torch.isfinite(t).all()) for t in res)
        check_all(c, H, res, refs.b["own"], refs.feat("own", H), f"wide logits H{H} chunk {chunk}")
        assert bool(res[0][:, g.hub].abs().max() > 0)


# ------------------------------------------------------------------------------- composition
def rebuilt_bounds(c, H, G, ers):
    """The bounds of the rebuilt sequence's two gradients: the weight bound and the edge
    gradient's through the softmax backward (edge_softmax_ref.backward), that through the
    aggregation onto q with one rounding for the scale, and both feature gradients onto
    topk_values with one rounding for the scale and one for the sum (the chain of
    test_dot_attention_gpu.py's autograd test)."""
    g, a = c["g"], DR.heads_slice(c["a"], H)
    s = float(np.float32(c["scale"]))
    D = c["D"]
    bs = [ER.backward(g.rp, g.col, a.heads[h]._replace(bound=a.w_bound[h]), ers[h].ref,
                      gw_bound=R.bound(ers[h])) for h in range(H)]
    gl = np.stack([b.gl for b in bs])
    gl_bound = np.stack([b.gl_bound for b in bs])
    gq = [DG.agg_ref(g, gl[h], gl_bound[h], c["cv"], c["ci"], D, c["n"]) for h in range(H)]
    gq_val = np.stack([x[0] for x in gq])
    gq_bound = s * np.stack([x[1] for x in gq]) + DR.U * s * np.abs(gq_val)
    v1, b1 = GA.feat_grad_ref(g, a, G[:H], c["ci"], D)
    v2, b2 = GA.feat_grad_ref(g, types.SimpleNamespace(w=gl, w_bound=gl_bound), c["q"][:H],
                              c["ci"], D)
    return gq_bound, b1 + s * b2 + 2 * DR.U * (np.abs(v1) + s * np.abs(v2))


def rebuilt(mk, rp, col, q, cv, ci, m, z, Gd, D, s, chunk=0):
    """Exactly what MaxKDotAttentionHeadsFunction's rebuilt backward runs."""
    H = q.shape[0]
    alpha = mk.dot_edge_alpha_heads(rp, col, q, cv, ci, D, s, m, z, chunk=chunk)
    grad_a = mk.edge_weight_grad_heads(rp, col, cv, ci, Gd, chunk=chunk)
    grad_l = torch.empty_like(grad_a)
    for h in range(H):
        mk.edge_softmax_backward(rp, alpha[h], grad_a[h], out=grad_l[h])
    gq = mk.spgemm_forward_heads(rp, col, grad_l, cv, ci, D, chunk=chunk).mul_(s)
    gt = mk.sspmm_backward_heads(rp, col, alpha, Gd, ci, chunk=chunk)
    gt.add_(mk.sspmm_backward_heads(rp, col, grad_l, q, ci, chunk=chunk), alpha=s)
    return gq, gt


@pytest.mark.parametrize("H", [2, 5])
@pytest.mark.parametrize("name,k,D", [("S", 16, 256), ("Dn", 32, 256), ("R", 7, 9)])
def test_against_the_sequence_it_replaces(mk, cuda, name, k, D, H):
    """dot_edge_alpha_heads -> edge_weight_grad_heads -> H edge_softmax_backward ->
    spgemm_forward_heads -> two sspmm_backward_heads on the same inputs: each result differs
    from the fused call's by at most the sum of both paths' bounds.  KG = 16, 32, 8."""
    c = make_case(name, k, D, 0.125)
    G = cotangent(c)
    refs = Refs(c, G, H, ("own",))
    gq_b, gt_b = rebuilt_bounds(c, H, G, refs.ers)
    rp, col = dev_graph(name)
    q, cv, ci = ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    out, m, z = fwd = own_forward(mk, name, ops, c)
    b, feat = refs.b["own"], refs.feat("own", H)
    for chunk in (0, 64):
        fused = run(mk, name, ops, c, fwd, Gd, chunk)
        seq = rebuilt(mk, rp, col, q, cv, ci, m, z, Gd, D, c["scale"], chunk)
        for x, y, both, what in ((fused[0], seq[0], b.g_q_bound[:H] + gq_b, "grad_q"),
                                 (fused[1], seq[1], feat[1] + gt_b, "grad_cbsr")):
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
    c = make_case("S", k, D, 0.25, ci=ci)
    assert (ci >= D).any() and (c["n"] == 0).any()
    G = cotangent(c)
    refs = Refs(c, G, 3)
    ops = dev_case(c, 3)
    Gd = T(np.ascontiguousarray(G[:3]), DEV)
    fwd = {"ref": ref_forward(c, 3), "own": own_forward(mk, "S", ops, c, validate=False)}
    for regime in ("ref", "own"):
        for chunk in (0, 64):
            res = run(mk, "S", ops, c, fwd[regime], Gd, chunk, validate=False)
            check_all(c, 3, res, refs.b[regime], refs.feat(regime, 3),
                      f"selectors k{k} D{D} {regime}")
            kept = dup[ci[dup, 0] < D]
            assert M.same_bytes(res[1][T(kept, DEV), k - 1].contiguous(),
                                res[1][T(kept, DEV), 0].contiguous())


# ------------------------------------------------------------------------------- non-finite
def test_non_finite(mk, cuda):
    """Head 1 of 3 on graph S, by the reference's masks (N.same_class inside check).  A NaN in
    q[1, r, j] at a column a neighbour of the short row r selects reaches head 1's grad_q row r
    wherever it has an addend and grad_cbsr of the columns r reads; heads 0 and 2 keep the bytes
    of their grad_q.  A -Inf logit of another row gives alpha = 0 and gl = 0: grad_q of that row
    stays finite.  A NaN of q at every column a third row does not select, and a NaN of grad_out
    in every column a row does not select, reach nothing: the bytes of the clean run."""
    H, D = 3, 256
    c, G, refs = shared("S")
    g, ci, cv = c["g"], c["ci"], c["cv"]
    deg = np.diff(g.rp)

    def neighbours(r):
        return g.col[g.rp[r]:g.rp[r + 1]]

    def own_slot(r):
        s = ci[neighbours(r)]
        vals, counts = np.unique(s, return_counts=True)
        single = np.isin(s, vals[counts == 1])
        return np.where(single.any(1), single.argmax(1), -1)

    short = [int(r) for r in np.flatnonzero((deg >= 2) & (deg <= 30))
             if r != g.hub and (own_slot(int(r)) >= 0).all()]
    short.sort(key=lambda r: deg[r])
    nan_row, ninf_row, clean_row = short[:3]
    q = c["q"][:H].copy()
    c0 = neighbours(nan_row)[0]
    q[1, nan_row, ci[c0, 1]] = np.nan
    c2 = neighbours(ninf_row)[1]
    l2 = own_slot(ninf_row)[1]
    q[1, ninf_row, ci[c2, l2]] = -np.copysign(np.inf, cv[c2, l2])
    unused = np.setdiff1d(np.arange(D), ci[neighbours(clean_row)].ravel())
    q[1, clean_row, unused] = np.nan
    n = c["n"]
    a = DR.attention(g.rp, g.col, q, c["scale"], cv, ci, D, n)
    p = dict(c, a=a, q=q)
    b = BR.backward(g, a, q, c["scale"], cv, ci, G[:H], D, a.out_bound, n, ers=refs.ers[:H])
    feat = BR.cbsr(b, H)
    assert np.isnan(b.g_q[1, nan_row][n[nan_row] > 0]).all()
    assert np.isnan(feat[0][neighbours(nan_row)]).all()
    assert np.isfinite(b.g_q[[0, 2]]).all() and np.isfinite(b.g_q[1]).mean() > 0.9
    e2 = g.rp[ninf_row] + 1
    assert a.w[1, e2] == 0 and b.gl[1, e2] == 0 and np.isfinite(b.g_q[1, ninf_row]).all()
    assert np.array_equal(b.g_q[1, clean_row], refs.b["own"].g_q[1, clean_row])
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    G2 = G[:H].copy()
    G2[:, n == 0] = np.nan
    assert np.isnan(G2).any()
    for chunk in (0, 64):
        ops = dev_case(c, H)
        fwd = own_forward(mk, "S", ops, c, chunk)
        clean = run(mk, "S", ops, c, fwd, Gd, chunk)
        ops_p = dev_case(c, H, q)
        res = run(mk, "S", ops_p, c, own_forward(mk, "S", ops_p, c, chunk), Gd, chunk)
        check_all(p, H, res, b, feat, f"non-finite chunk {chunk}")
        for h in (0, 2):
            assert M.same_bytes(clean[0][h].contiguous(), res[0][h].contiguous()), (chunk, h)
        assert M.same_bytes(clean[0][1, clean_row].contiguous(), res[0][1, clean_row].contiguous())
        nan_g = run(mk, "S", ops, c, fwd, T(G2, DEV), chunk)
        for x, y in zip(clean, nan_g):
            assert M.same_bytes(x, y), chunk


@pytest.mark.parametrize("H,h", [(3, 1), (8, 6), (5, 0)])
def test_head_isolation(mk, cuda, H, h):
    """The other heads' queries (and with them their out, row_max and row_sum) and their
    grad_out replaced by other numbers: head h's grad_q keeps its bytes.  HP = 4 and 8."""
    c, G, _ = shared("corner")
    rng = np.random.default_rng(2600 + H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    for chunk in (0, 64, 7):
        ops = dev_case(c, H)
        base = run(mk, "corner", ops, c, own_forward(mk, "corner", ops, c, chunk), Gd, chunk)
        x = rng.standard_normal(c["q"][:H].shape).astype(np.float32)
        x[h] = c["q"][h]
        G2 = rng.standard_normal(G[:H].shape).astype(np.float32)
        G2[h] = G[h]
        ops2 = dev_case(c, H, x)
        other = run(mk, "corner", ops2, c, own_forward(mk, "corner", ops2, c, chunk), T(G2, DEV),
                    chunk)
        assert M.same_bytes(base[0][h].contiguous(), other[0][h].contiguous()), chunk
        assert not M.same_bytes(base[1], other[1])  # grad_cbsr sums the heads


# ------------------------------------------------------------------------------- degenerate
@pytest.mark.parametrize("H", [1, 3, 8])
def test_no_edges(mk, cuda, H):
    """num_e == 0: zeros in both gradients."""
    rows, cols, D, k = 40, 17, 64, 8
    rp = torch.zeros(rows + 1, dtype=torch.int32, device=cuda)
    col = torch.empty(0, dtype=torch.int32, device=cuda)
    q = torch.randn(H, rows, D, device=cuda)
    cv = torch.randn(cols, k, device=cuda)
    ci = torch.zeros(cols, k, dtype=torch.uint8, device=cuda)
    out, m, z = mk.dot_attention_heads(rp, col, q, cv, ci, D, 0.5)
    G = torch.randn(H, rows, D, device=cuda)
    junk = [torch.full((n,), float("nan"), device=cuda) for n in (H * rows * D, cols * k)]
    del junk
    res = mk.dot_attention_heads_backward(rp, col, q, cv, ci, out, m, z, G, 0.5)
    assert [tuple(t.shape) for t in res] == [(H, rows, D), (cols, k)]
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
    fwd = own_forward(mk, name, ops, c)
    for chunk in (0, 7, 64):
        n_ws = mk._lib().maxk_dot_attention_heads_backward_workspace_size(
            g.R, g.C, g.col.size, 256, 16, H, chunk)
        runs = []
        for fill in (0x00, 0xFF):
            junk = [torch.full((n,), fill, dtype=torch.uint8, device=cuda)
                    for n in (n_ws, n_ws // 2, 4 * H * g.R * 256, 4 * g.C * 16, 4096)]
            del junk
            runs.append(run(mk, name, ops, c, fwd, Gd, chunk))
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
    fwd = own_forward(mk, "corner", dev_case(c, H), c)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    for chunk in (0, 64):
        def factory(primer):
            dt = (T(g.rp, DEV), T(g.col, DEV))
            plan = mk.transpose_plan(dt[1], g.C, cache=False)
            ops = dev_case(c, H)
            rest = tuple(t.clone() for t in fwd) + (Gd.clone(),)
            if primer:
                gen = torch.Generator(device=DEV).manual_seed(5)
                ops = tuple(torch.rand(t.shape, generator=gen, device=DEV) for t in ops[:2]) \
                    + (ops[2],)
                rest = tuple(torch.rand(t.shape, generator=gen, device=DEV) + 0.5 for t in rest)
            return (dt, plan) + ops + rest

        def op(dt, plan, q, cv, ci, out, m, z, G_):
            return mk.dot_attention_heads_backward(dt[0], dt[1], q, cv, ci, out, m, z, G_,
                                                   c["scale"], chunk=chunk, plan=plan)

        res = M.run_regimes(op, factory, arena)
        n_ws = mk._lib().maxk_dot_attention_heads_backward_workspace_size(g.R, g.C, E, D, k, H,
                                                                          chunk)
        assert sorted(x.nbytes for x in arena.allocs) == sorted(
            [4 * H * g.R * D, 4 * g.C * k, n_ws])
        for regime in ("stale", "ones"):
            for x, y in zip(res["zero"], res[regime]):
                assert M.same_bytes(x, y), regime
        check_all(c, H, res["ones"], refs.b["own"], refs.feat("own", H),
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
    fwd = own_forward(mk, "corner", ops, c, dt=dt)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    torch.cuda.synchronize()
    shrunk = Shrunk(mk._L, "maxk_dot_attention_heads_backward_workspace_size")
    monkeypatch.setattr(mk, "_L", shrunk)
    with arena.active("ones"):
        with pytest.raises(RuntimeError, match="workspace too small"):
            run(mk, "corner", ops, c, fwd, Gd, 0, dt=dt, plan=plan)
        made = len(arena.allocs)
    assert shrunk.sizes and all(n > 1 for n in shrunk.sizes), shrunk.sizes
    assert made >= 3  # the outputs and the short workspace came from the arena
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
    q, cv, ci = ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    s = c["scale"]
    for chunk in (0, 64):
        fwd = own_forward(mk, "corner", ops, c, chunk)
        eager = run(mk, "corner", ops, c, fwd, Gd, chunk)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            G2 = torch.zeros_like(Gd)
            for _ in range(20):  # queued on the side stream before the call
                G2 = G2 + Gd / 20
            G2.copy_(Gd)
            res = run(mk, "corner", ops, c, fwd, G2, chunk)
        side.synchronize()
        for x, y in zip(eager, res):
            assert M.same_bytes(x, y)
        hg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(hg, stream=side):
            f2 = mk.dot_attention_heads(rp, col, q, cv, ci, 256, s, chunk=chunk, validate=False)
            got = mk.dot_attention_heads_backward(rp, col, q, cv, ci, *f2, Gd, s, chunk=chunk,
                                                  validate=False, plan=plan)
        for _ in range(2):
            for t in (*f2, *got):
                t.fill_(float("nan"))
            hg.replay()
            torch.cuda.synchronize()
            for x, y in zip((*fwd, *eager), (*f2, *got)):
                assert M.same_bytes(x, y)


# ------------------------------------------------------------------------------- autograd
def test_autograd_fused_backward(mk, cuda, monkeypatch):
    """maxk_dot_attention_heads(backward="fused") against backward="rebuilt" and the references,
    H = 3 on graph S: the fused function saves `out` (and only then), its backward is one
    dot_attention_heads_backward call that allocates the two gradients and a workspace of the
    queried size and no tensor of H * E elements, where the rebuilt one allocates alpha and
    grad_a.  It falls back to the rebuilt backward when a gradient is not needed, when the table
    is too large for the entry and when MAXK_BWD_MODE forces a mode."""
    import maxk_layers as ML
    monkeypatch.delenv("MAXK_BWD_MODE", raising=False)
    monkeypatch.delenv("MAXK_DOT_ATTN_BWD", raising=False)
    D, k, H = 64, 16, 3
    c, G, refs = shared("S", k, D)
    g = c["g"]
    E = g.col.size
    s = c["scale"]
    rp, col = dev_graph("S")
    graph_ = ML.CSRGraph(rp, col)
    mk.transpose_plan(col, g.C)  # cached: not an allocation of the backward
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    calls = []
    for fn in ("dot_attention_heads_backward", "dot_edge_alpha_heads", "edge_weight_grad_heads"):
        real = getattr(mk, fn)
        monkeypatch.setattr(mk, fn, lambda *a, _r=real, _n=fn, **kw: calls.append(_n) or
                            _r(*a, **kw))
    real_empty = torch.empty
    res, saved, allocs = {}, {}, {}

    def run_path(path, need=(True, True), **kw):
        q, tv, ci = dev_case(c, H)
        for t, n in zip((q, tv), need):
            t.requires_grad_(n)
        sizes = []
        with torch.autograd.graph.saved_tensors_hooks(
                lambda t: sizes.append(tuple(t.shape)) or t, lambda t: t):
            y = graph_.dot_attend_heads(tv, ci, D, q, s, **kw)
        made = []

        def empty(*a, **k_):
            t = real_empty(*a, **k_)
            made.append((t.dtype, t.numel()))
            return t
        del calls[:]
        monkeypatch.setattr(torch, "empty", empty)
        y.backward(Gd)
        monkeypatch.setattr(torch, "empty", real_empty)
        res[path] = (y.detach(), q.grad, tv.grad)
        saved[path], allocs[path] = sizes, made
        return list(calls)

    assert run_path("fused", backward="fused") == ["dot_attention_heads_backward"]
    assert "dot_attention_heads_backward" not in run_path("rebuilt")
    assert saved["fused"].count((H, g.R, D)) == 2 and saved["rebuilt"].count((H, g.R, D)) == 1
    assert len(saved["fused"]) == len(saved["rebuilt"]) + 1
    assert all(len(sh) != 2 or sh[1] != E for sh in saved["fused"])  # nothing [H, E]
    n_ws = mk._lib().maxk_dot_attention_heads_backward_workspace_size(g.R, g.C, E, D, k, H, 0)
    f32 = [n for dt, n in allocs["fused"] if dt == torch.float32]
    assert sorted(f32) == sorted([H * g.R * D, g.C * k])
    assert [n for dt, n in allocs["fused"] if dt == torch.uint8] == [n_ws]
    assert not any(n == H * E for _, n in allocs["fused"])
    assert sum(n == H * E for dt, n in allocs["rebuilt"] if dt == torch.float32) >= 2
    b, feat = refs.b["own"], refs.feat("own", H)
    gq_b, gt_b = rebuilt_bounds(c, H, G, refs.ers)
    a = DR.heads_slice(c["a"], H)
    y, gq, gt = res["fused"]
    check(y, a.out, a.out_bound, "autograd fused out")
    check(gq, b.g_q[:H], b.g_q_bound[:H], "autograd fused grad_q")
    check(gt, feat[0], feat[1], "autograd fused grad_cbsr")
    y, gq, gt = res["rebuilt"]
    assert M.same_bytes(y, res["fused"][0])
    N.within(gq, b.g_q[:H], gq_b, "autograd rebuilt q.grad")
    N.within(gt, feat[0], gt_b, "autograd rebuilt topk_values.grad")
    # the fallbacks, and the environment's override of the argument
    assert "dot_attention_heads_backward" not in run_path("partial", (True, False),
                                                          backward="fused")
    assert M.same_bytes(res["partial"][1], res["rebuilt"][1])
    max_cols = mk.HEADS_MAX_COLS
    monkeypatch.setattr(mk, "HEADS_MAX_COLS", g.C)
    assert "dot_attention_heads_backward" not in run_path("wide", backward="fused")
    monkeypatch.setattr(mk, "HEADS_MAX_COLS", max_cols)
    monkeypatch.setenv("MAXK_BWD_MODE", "csc")
    assert "dot_attention_heads_backward" not in run_path("forced", backward="fused")
    monkeypatch.delenv("MAXK_BWD_MODE")
    monkeypatch.setenv("MAXK_DOT_ATTN_BWD", "fused")
    assert run_path("env") == ["dot_attention_heads_backward"]
    monkeypatch.setenv("MAXK_DOT_ATTN_BWD", "rebuilt")
    assert "dot_attention_heads_backward" not in run_path("env2", backward="fused")
    for x, y in zip(res["env"], res["fused"]):
        assert M.same_bytes(x, y)
    for x, y in zip(res["wide"], res["rebuilt"]):
        assert M.same_bytes(x, y)


def test_transformer_conv_fused_backward_matches_dense(cuda, monkeypatch):
    """MaxKTransformerConv(attention="fused", attention_backward="fused") at V = 300, in = 64,
    out = 8, H = 4, k = 16 against the same layer in dense float64 torch, as
    test_dot_attention_gpu.py::test_transformer_conv_fused_matches_stored_and_dense: the output,
    every parameter's gradient and both input gradients at rtol = atol = 1e-4; MAXK_DOT_ATTN_BWD
    overrides the argument, and it has no effect where the attention is "stored"."""
    import maxk_cuda_kernels as mk_
    import maxk_layers as ML
    monkeypatch.delenv("MAXK_DOT_ATTN", raising=False)
    monkeypatch.delenv("MAXK_DOT_ATTN_BWD", raising=False)
    monkeypatch.delenv("MAXK_BWD_MODE", raising=False)
    torch.manual_seed(4)
    rng = np.random.default_rng(300)
    V, D, k, O_, H = 300, 64, 16, 8, 4
    rp, col = rand_graph(rng, V, 8, hubs=((7, 220),), empty=3)
    graph_ = ML.CSRGraph(T(rp.astype(np.int32), cuda), T(col.astype(np.int32), cuda))
    conv = ML.MaxKTransformerConv(D, O_, H, attention="fused",
                                  attention_backward="fused").to(cuda)
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
    calls = []
    real = mk_.dot_attention_heads_backward
    monkeypatch.setattr(mk_, "dot_attention_heads_backward",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    for attn, arg, env, fused in (("fused", "fused", None, True), ("fused", "rebuilt", None, False),
                                  ("fused", "rebuilt", "fused", True),
                                  ("fused", "fused", "rebuilt", False),
                                  ("stored", "fused", "fused", False)):
        conv.attention, conv.attention_backward = attn, arg
        if env is None:
            monkeypatch.delenv("MAXK_DOT_ATTN_BWD", raising=False)
        else:
            monkeypatch.setenv("MAXK_DOT_ATTN_BWD", env)
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
