"""GPU: attention dropout inside the fused dot-product attention walks -- the dropout entries of
dot_attention_heads.hip and dot_attention_heads_bwd.hip through the binding
(mk.dot_attention_heads(dropout=, seed=), mk.dot_attention_heads_backward(dropout=, seed=)),
MaxKDotAttentionHeadsFunction and MaxKTransformerConv(fused_attn_drop=True), against
tests/dot_attn_dropout_ref.py (float64, with its derived bounds), against the rebuilt sequence with
the elementwise mask and against dense float64 torch with the same mask multiplied in.

Which kernels.  dropout > 0 launches dath_fwd_kernel<KG, 8, true> with
softmax_fixup_kernel<true>, and datb_walk_kernel<KG, HP, 4, true>; everything else (the pack,
datb_gq_kernel, the slab fix-ups, the CSC sum) is the entries' without dropout.  KG = 8, 16, 32, 64
for k = 3 and 7, 16, 24, 96; HP = 2, 4, 8 for H = 1 and 2, 3, 5 and 8.  In the forward the mask's
evaluation is shared by S = 64 / (EP * 8 * qp) wave steps: S = 1 (k <= 8 at H = 1), 2, 4 and 8
with one and two quads of heads per pass are all reached by test_forward_parity.

The inputs out, row_max and row_sum of the backward are either the float64 reference rounded to
fp32 ("ref": out_err = u |out|) or what the dropped forward returned ("own": its out_bound).
"""
import functools

import numpy as np
import pytest
import torch

import attn_dropout_ref as AD
import dot_attention_bwd_ref as DB
import dot_attention_ref as DA
import dot_attn_dropout_ref as DD
import esm_corner_graph as EG
import memguard as M
import numerics as N
import test_dot_attention_gpu as DG
import test_gat_attention_gpu as GA
from test_dot_attention_bwd_gpu import cotangent
from test_dot_attention_gpu import DEV, HMAX, case, dev_case, dev_graph, make_case, the_graph
from test_memguard_gpu import Shrunk
from test_parity_gpu import T, rand_graph

pytestmark = pytest.mark.gpu

CHUNKS = (0,) + EG.CHUNKS
SEED = 12345
RATIOS: dict = {}


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


# ------------------------------------------------------------------------------- shared data
def drop_case(c, p, seed):
    """The case c (test_dot_attention_gpu.make_case) with the dropped reference at HMAX heads."""
    g = c["g"]
    ad, _, d = DD.attention(g.rp, g.col, c["q"], c["scale"], c["cv"], c["ci"], c["D"], c["n"], p,
                            seed, base=c["a"])
    return dict(c, ad=ad, d=d, p=p, seed=seed)


@functools.lru_cache(maxsize=None)
def dcase(name, k=16, D=256, p=0.5, seed=SEED):
    """The cases several tests share: computed once, never modified."""
    return drop_case(case(name, k, D), p, seed)


class Refs:
    """The backward references of one dropped case and one G at H heads for the regimes of `out`;
    the feature gradient and the rebuilt sequence's bounds per number of heads."""

    def __init__(self, c, G, H=HMAX, regimes=("ref", "own")):
        self.c, self.G, self.H = c, G, H
        self.a, self.ad = DA.heads_slice(c["a"], H), DA.heads_slice(c["ad"], H)
        self.ers = DB.edge_grads(c["g"], c["cv"], c["ci"], G[:H])
        err = {"ref": DD.rounded_out_err(self.ad), "own": self.ad.out_bound}
        self.b = {r: DD.backward(c["g"], self.a, self.ad, c["d"][:H], c["q"][:H], c["scale"],
                                 c["cv"], c["ci"], G[:H], c["D"], err[r], c["n"], ers=self.ers)
                  for r in regimes}

    @functools.lru_cache(maxsize=None)
    def feat(self, regime, H):
        return DB.cbsr(self.b[regime], H)

    @functools.lru_cache(maxsize=None)
    def rebuilt(self, H):
        c = self.c
        g, D = c["g"], c["D"]
        return DD.rebuilt_bounds(
            g, DA.heads_slice(c["a"], H), DA.heads_slice(c["ad"], H), c["d"][:H], c["q"],
            c["scale"], c["ci"], self.G, D, c["n"], self.ers[:H],
            lambda gl, glb: DG.agg_ref(g, gl, glb, c["cv"], c["ci"], D, c["n"]),
            lambda w, X: GA.feat_grad_ref(g, w, X, c["ci"], D))


@functools.lru_cache(maxsize=None)
def shared(name, k=16, D=256, p=0.5, seed=SEED):
    c = dcase(name, k, D, p, seed)
    G = cotangent(c)
    return c, G, Refs(c, G)


def fwd(mk, name, c, ops, chunk=0, dt=None, **kw):
    rp, col = dev_graph(name) if dt is None else dt
    q, cv, ci = ops
    return mk.dot_attention_heads(rp, col, q, cv, ci, c["D"], c["scale"], chunk=chunk,
                                  dropout=c["p"], seed=c["seed"], **kw)


def bwd(mk, name, c, ops, f, G, chunk=0, dt=None, **kw):
    rp, col = dev_graph(name) if dt is None else dt
    q, cv, ci = ops
    return mk.dot_attention_heads_backward(rp, col, q, cv, ci, *f, G, c["scale"], chunk=chunk,
                                           dropout=c["p"], seed=c["seed"], **kw)


def rebuilt_bwd(mk, name, c, ops, f, G, chunk=0):
    """Exactly what MaxKDotAttentionHeadsFunction's rebuilt backward runs under dropout."""
    rp, col = dev_graph(name)
    q, cv, ci = ops
    H, D, s = q.shape[0], c["D"], c["scale"]
    alpha = mk.dot_edge_alpha_heads(rp, col, q, cv, ci, D, s, f[1], f[2], chunk=chunk)
    grad_a = mk.edge_weight_grad_heads(rp, col, cv, ci, G, chunk=chunk)
    mk.edge_dropout_heads(grad_a, c["p"], c["seed"], out=grad_a)
    grad_l = torch.empty_like(grad_a)
    for h in range(H):
        mk.edge_softmax_backward(rp, alpha[h], grad_a[h], out=grad_l[h])
    gq = mk.spgemm_forward_heads(rp, col, grad_l, cv, ci, D, chunk=chunk).mul_(s)
    mk.edge_dropout_heads(alpha, c["p"], c["seed"], out=alpha)
    gt = mk.sspmm_backward_heads(rp, col, alpha, G, ci, chunk=chunk)
    gt.add_(mk.sspmm_backward_heads(rp, col, grad_l, q, ci, chunk=chunk), alpha=s)
    return gq, gt


def ref_forward(c, H):
    """out, row_max, row_sum of the dropped float64 reference, rounded to fp32."""
    ad = c["ad"]
    with np.errstate(over="ignore", invalid="ignore"):
        return tuple(T(np.ascontiguousarray(x[:H]).astype(np.float32), DEV)
                     for x in (ad.out, ad.m, ad.z))


def check(y, ref, bound, what):
    assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape, (y.shape, ref.shape)
    r = N.within(y, ref, bound, what)
    RATIOS[what] = max(r, RATIOS.get(what, 0.0))
    print(f"{what}: err/bound {r:.3f}")
    return r


def check_fwd(c, H, res, what):
    """out inside the dropped bound, the statistics inside the undropped softmax's; exact zeros
    for empty rows and unselected columns."""
    g, ad = c["g"], DA.heads_slice(c["ad"], H)
    out, m, z = res
    check(out, ad.out, ad.out_bound, f"{what} out")
    check(m, ad.m, ad.m_bound, f"{what} row_max")
    check(z, ad.z, ad.z_bound, f"{what} row_sum")
    empty = T(np.diff(g.rp) == 0, DEV)
    assert not out[:, empty].any() and not m[:, empty].any() and not z[:, empty].any()
    assert not out[:, T(c["n"] == 0, DEV)].any()


def check_bwd(c, H, res, b, feat, what):
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


# ------------------------------------------------------------------------------- forward
SHAPES = [(3, 64), (16, 256), (24, 256), (96, 256), (7, 9)]


@pytest.mark.parametrize("k,D", SHAPES, ids=[f"k{k}-D{D}" for k, D in SHAPES])
@pytest.mark.parametrize("name", ["S", "Dn", "R", "corner"])
def test_forward_parity(mk, cuda, name, k, D):
    """out inside the dropped reference's bound at H in 1, 3, 8 and every item size of the sweep;
    row_max and row_sum bitwise those of the call without dropout at the same item size; out
    differs from the undropped one; dropout = 0 bitwise the old entry in all three outputs."""
    c = drop_case(case(name, k, D), 0.5, SEED)
    rp, col = dev_graph(name)
    for H in (1, 3, 8):
        ops = dev_case(c, H)
        for chunk in CHUNKS:
            res = fwd(mk, name, c, ops, chunk)
            check_fwd(c, H, res, f"{name} k{k} D{D} H{H}")
            plain = mk.dot_attention_heads(rp, col, *ops, D, c["scale"], chunk=chunk)
            assert M.same_bytes(res[1], plain[1]) and M.same_bytes(res[2], plain[2]), chunk
            assert not M.same_bytes(res[0], plain[0])
            zero = mk.dot_attention_heads(rp, col, *ops, D, c["scale"], chunk=chunk, dropout=0.0,
                                          seed=SEED)
            for x, y in zip(zero, plain):
                assert M.same_bytes(x, y), chunk


@pytest.mark.parametrize("p", [0.1, 0.9])
def test_forward_rates(mk, cuda, p):
    """The other two rates on the corner graph, H = 5 (two passes of heads at k = 16)."""
    c = dcase("corner", 16, 256, p)
    ops = dev_case(c, 5)
    for chunk in (0, 64, 7):
        check_fwd(c, 5, fwd(mk, "corner", c, ops, chunk), f"corner p{p} H5")


def test_mask_does_not_depend_on_the_partition(mk, cuda):
    """Two item sizes on the corner graph cut the rows differently: the exactly-zero elements of
    out are the same set in both and the reference's, and both meet the bound.  H = 8."""
    c = dcase("corner", 16, 256, 0.9)
    ops = dev_case(c, 8)
    a, b = (fwd(mk, "corner", c, ops, chunk)[0] for chunk in (7, 513))
    check(a, c["ad"].out, c["ad"].out_bound, "partition chunk 7 out")
    check(b, c["ad"].out, c["ad"].out_bound, "partition chunk 513 out")
    assert bool(((a == 0) == (b == 0)).all())
    assert bool((a == 0).any()) and bool((a != 0).any())
    assert np.array_equal(a.cpu().numpy() == 0, c["ad"].out == 0)


FULL_SEED = 3  # found on the CPU with the reference: see the assertions below


def test_a_fully_dropped_row(mk, cuda):
    """p = 0.9 on graph S, H = 3: under FULL_SEED the reference finds rows of degree >= 2 all of
    whose edges are dropped in some head.  Their out is exact zeros, their row_sum is positive,
    and the backward is inside its bounds."""
    H = 3
    c, G, refs = shared("S", 16, 256, 0.9, FULL_SEED)
    g = c["g"]
    deg = np.diff(g.rp)
    kept = np.stack([np.add.reduceat(c["d"][h] > 0, g.rp[:-1][deg > 0]) for h in range(H)])
    full = np.zeros((H, g.R), bool)
    full[:, deg > 0] = kept == 0
    full &= (deg >= 2)[None]
    assert full.any(), "no fully dropped row of degree >= 2 under this seed"
    assert np.isfinite(c["ad"].out[:H]).all() and (c["ad"].out[:H][full] == 0).all()
    ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    fd = T(full, DEV)
    for chunk in (0, 64, 2):
        f = fwd(mk, "S", c, ops, chunk)
        check_fwd(c, H, f, f"fully dropped chunk {chunk}")
        assert not f[0][fd].any()
        assert bool((f[2][fd] > 0).all())  # the statistics are the undropped softmax's
        res = bwd(mk, "S", c, ops, f, Gd, chunk)
        check_bwd(c, H, res, refs.b["own"], refs.feat("own", H), f"fully dropped chunk {chunk}")


# ------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("H", [2, 5, 8])
@pytest.mark.parametrize("name,k,D", [("S", 16, 256), ("R", 7, 9), ("corner", 16, 256),
                                      ("corner", 24, 256), ("S", 96, 256)])
def test_backwards(mk, cuda, name, k, D, H):
    """The fused backward inside the reference's bounds with the reference's forward results and
    with the kernel's own; the rebuilt sequence with edge_dropout_heads inside its own bounds;
    grad_cbsr of the two within the summed bounds; dropout = 0 bitwise the old entry."""
    c, G, refs = shared(name, k, D)
    ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    gq_b, gt_b = refs.rebuilt(H)
    for chunk in (0, 64, 7):
        f = {"ref": ref_forward(c, H), "own": fwd(mk, name, c, ops, chunk)}
        for regime in ("ref", "own"):
            fused = bwd(mk, name, c, ops, f[regime], Gd, chunk)
            check_bwd(c, H, fused, refs.b[regime], refs.feat(regime, H),
                      f"fused {name} k{k} H{H} {regime}")
        b, feat = refs.b["own"], refs.feat("own", H)
        reb = rebuilt_bwd(mk, name, c, ops, f["own"], Gd, chunk)
        check(reb[0], b.g_q[:H], gq_b, f"rebuilt {name} k{k} H{H} grad_q")
        check(reb[1], feat[0], gt_b, f"rebuilt {name} k{k} H{H} grad_cbsr")
        err = (fused[1].double() - reb[1].double()).abs().cpu().numpy()
        assert (err <= feat[1] + gt_b).all()
    rp, col = dev_graph(name)
    plain_f = mk.dot_attention_heads(rp, col, *ops, D, c["scale"])
    plain = mk.dot_attention_heads_backward(rp, col, *ops, *plain_f, Gd, c["scale"])
    zero = mk.dot_attention_heads_backward(rp, col, *ops, *plain_f, Gd, c["scale"], dropout=0.0,
                                           seed=SEED)
    for x, y in zip(plain, zero):
        assert M.same_bytes(x, y)


@pytest.mark.parametrize("p", [0.1, 0.9])
def test_backward_rates(mk, cuda, p):
    c, G, refs = shared("corner", 16, 256, p)
    H = 3
    ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    for chunk in (0, 64):
        f = fwd(mk, "corner", c, ops, chunk)
        check_bwd(c, H, bwd(mk, "corner", c, ops, f, Gd, chunk), refs.b["own"],
                  refs.feat("own", H), f"fused corner p{p}")


# ------------------------------------------------------------------------------- selectors
def test_skipped_and_repeated_selectors(mk, cuda):
    """k = 5, D = 24 with selectors >= D (skipped; their gradient slots an exact 0) and repeated
    inside a vertex, dropout on, both directions.  KG = 8, HP = 4."""
    k, D, H = 5, 24, 3
    g = the_graph("S")
    rng = np.random.default_rng(2500 + k)
    ci = N.selectors(rng, g.C, 256, k)
    dup = rng.choice(g.C, g.C // 4, replace=False)
    ci[dup, k - 1] = ci[dup, 0]
    c = drop_case(make_case("S", k, D, 0.25, ci=ci), 0.5, SEED)
    assert (ci >= D).any() and (c["n"] == 0).any()
    G = cotangent(c)
    refs = Refs(c, G, H, ("own",))
    ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    for chunk in (0, 64):
        f = fwd(mk, "S", c, ops, chunk, validate=False)
        check_fwd(c, H, f, f"selectors k{k} D{D}")
        res = bwd(mk, "S", c, ops, f, Gd, chunk, validate=False)
        check_bwd(c, H, res, refs.b["own"], refs.feat("own", H), f"selectors k{k} D{D}")
        assert not res[1][T(ci >= D, DEV)].any()
        kept = dup[ci[dup, 0] < D]
        assert M.same_bytes(res[1][T(kept, DEV), k - 1].contiguous(),
                            res[1][T(kept, DEV), 0].contiguous())


# ------------------------------------------------------------------------------- non-finite
def test_non_finite(mk, cuda):
    """Head 1 of 3 on graph S, by the reference's masks (N.same_class inside check): a NaN in
    q[1, r, j] at a column a neighbour of the short row r selects, forward and backward; and an
    Inf in the value of an edge that head 1 drops and head 0 keeps.  Unlike the GAT's scores, a
    value here enters its own edge's logit (Inf * q is +-Inf), so the head that keeps the edge
    cannot see a clean Inf: numpy's IEEE evaluation of the reference gives NaN at that element
    for the head that drops it (dropping does not shield) and for the head that keeps it (an
    Inf logit poisons the row's softmax, a -Inf one gives 0 * Inf), and the kernel must give the
    reference's classes everywhere."""
    H, D = 3, 256
    base = dcase("S")
    g, ci, d = base["g"], base["ci"], base["d"]
    deg = np.diff(g.rp)
    rows = np.repeat(np.arange(g.R), deg)
    readers = N._readers(g)
    hubs = np.flatnonzero(deg > 100)
    nan_row = next(int(r) for r in np.flatnonzero((deg >= 2) & (deg <= 30)) if r != g.hub)
    c0 = g.col[g.rp[nan_row]]
    q = base["q"].copy()
    q[1, nan_row, ci[c0, 1]] = np.nan
    e_inf = next(int(e) for e in range(g.col.size)
                 if d[1, e] == 0 and d[0, e] > 0 and rows[e] != nan_row and rows[e] not in hubs
                 and not np.isin(readers[g.col[e]], hubs).any()
                 and nan_row not in readers[g.col[e]])
    for with_inf in (False, True):
        cv = base["cv"].copy()
        if with_inf:
            cv[g.col[e_inf], 0] = np.inf
        a = DA.attention(g.rp, g.col, q, base["scale"], cv, ci, D, base["n"])
        c = drop_case(dict(base, q=q, cv=cv, a=a), 0.5, SEED)
        ad = c["ad"]
        r, j = rows[e_inf], ci[g.col[e_inf], 0]
        if with_inf:
            assert np.isnan(ad.out[[0, 1], r, j]).all() and not np.isfinite(a.l[:2, e_inf]).any()
        assert np.isnan(ad.out[1, nan_row][c["n"][nan_row] > 0]).all()
        assert np.isfinite(ad.out[[0, 2]]).mean() > 0.9
        ops = dev_case(c, H)
        for chunk in (0, 64):
            f = fwd(mk, "S", c, ops, chunk)
            check_fwd(c, H, f, f"non-finite inf {with_inf}")
            if not with_inf:
                G = cotangent(c)
                refs = Refs(c, G, H, ("own",))
                b = refs.b["own"]
                assert np.isnan(b.g_q[1, nan_row][c["n"][nan_row] > 0]).all()
                assert np.isfinite(b.g_q[[0, 2]]).all()
                res = bwd(mk, "S", c, ops, f, T(np.ascontiguousarray(G[:H]), DEV), chunk)
                check_bwd(c, H, res, b, refs.feat("own", H), "non-finite")


@pytest.mark.parametrize("H,h", [(3, 1), (8, 6)])
def test_head_isolation(mk, cuda, H, h):
    """The other heads' queries replaced: head h's slices of out, the statistics and grad_q keep
    their bytes, dropout on."""
    c, G, _ = shared("corner")
    rng = np.random.default_rng(2600 + H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    for chunk in (0, 64, 7):
        ops = dev_case(c, H)
        f = fwd(mk, "corner", c, ops, chunk)
        base = bwd(mk, "corner", c, ops, f, Gd, chunk)
        x = rng.standard_normal(c["q"][:H].shape).astype(np.float32)
        x[h] = c["q"][h]
        ops2 = dev_case(c, H, x)
        f2 = fwd(mk, "corner", c, ops2, chunk)
        other = bwd(mk, "corner", c, ops2, f2, Gd, chunk)
        for a, b in zip((*f, base[0]), (*f2, other[0])):
            assert M.same_bytes(a[h].contiguous(), b[h].contiguous()), chunk
        assert not M.same_bytes(f[0], f2[0]) and not M.same_bytes(base[1], other[1])


# ------------------------------------------------------------------------------- memory
@pytest.fixture(scope="module")
def arena(cuda):
    return M.Arena(48 << 20, cuda)


@pytest.mark.parametrize("k,D,H", [(16, 256, 3), (3, 64, 8)])
def test_memory_contract(mk, arena, cuda, k, D, H):
    """Both entries with outputs and workspace from the poisoned, guarded arena (the workspace
    exactly the queried size): outputs fully written and the same bytes in every fill regime,
    guards untouched, inputs unchanged."""
    c, G, refs = shared("corner", k, D)
    g = c["g"]
    E = g.col.size
    p, seed, s = c["p"], c["seed"], c["scale"]
    Gd = T(np.ascontiguousarray(G[:H]), DEV)

    def same(res):
        for regime in ("stale", "ones"):
            for x, y in zip(res["zero"], res[regime]):
                assert M.same_bytes(x, y), regime

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
            return mk.dot_attention_heads(dt[0], dt[1], q, cv, ci, D, s, chunk=chunk, dropout=p,
                                          seed=seed)

        res = M.run_regimes(op, factory, arena)
        n_ws = mk._lib().maxk_dot_attention_heads_dropout_workspace_size(g.R, g.C, E, D, k, H,
                                                                         chunk)
        assert sorted(x.nbytes for x in arena.allocs) == sorted(
            [4 * H * g.R * D, 4 * H * g.R, 4 * H * g.R, n_ws])
        same(res)
        check_fwd(c, H, res["ones"], f"memguard k{k} D{D} H{H}")
        f = tuple(t.clone() for t in res["ones"])

        def factory_b(primer):
            dt = (T(g.rp, DEV), T(g.col, DEV))
            plan = mk.transpose_plan(dt[1], g.C, cache=False)
            ops = dev_case(c, H)
            rest = tuple(t.clone() for t in f) + (Gd.clone(),)
            if primer:
                gen = torch.Generator(device=DEV).manual_seed(5)
                ops = tuple(torch.rand(t.shape, generator=gen, device=DEV) for t in ops[:2]) \
                    + (ops[2],)
                rest = tuple(torch.rand(t.shape, generator=gen, device=DEV) + 0.5 for t in rest)
            return (dt, plan) + ops + rest

        def op_b(dt, plan, q, cv, ci, out, m, z, G_):
            return mk.dot_attention_heads_backward(dt[0], dt[1], q, cv, ci, out, m, z, G_, s,
                                                   chunk=chunk, plan=plan, dropout=p, seed=seed)

        res = M.run_regimes(op_b, factory_b, arena)
        n_ws = mk._lib().maxk_dot_attention_heads_dropout_backward_workspace_size(
            g.R, g.C, E, D, k, H, chunk)
        assert sorted(x.nbytes for x in arena.allocs) == sorted(
            [4 * H * g.R * D, 4 * g.C * k, n_ws])
        same(res)
        check_bwd(c, H, res["ones"], refs.b["own"], refs.feat("own", H),
                  f"memguard k{k} D{D} H{H}")


@pytest.mark.parametrize("entry", ["forward", "backward"])
def test_undersized_workspace_is_rejected(mk, arena, monkeypatch, entry):
    """A workspace one byte short of the size query: "workspace too small" from the host-side
    check, before any launch -- the outputs (0xFF-filled) are unchanged, the guards intact."""
    H = 5
    c, G, _ = shared("corner")
    g = c["g"]
    dt = (T(g.rp, DEV), T(g.col, DEV))
    plan = mk.transpose_plan(dt[1], g.C, cache=False)
    ops = dev_case(c, H)
    f = fwd(mk, "corner", c, ops, dt=dt)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    torch.cuda.synchronize()
    shrunk = Shrunk(mk._L, {"forward": "maxk_dot_attention_heads_dropout_workspace_size",
                            "backward": "maxk_dot_attention_heads_dropout_backward_workspace_size"
                            }[entry])
    monkeypatch.setattr(mk, "_L", shrunk)
    with arena.active("ones"):
        with pytest.raises(RuntimeError, match="workspace too small"):
            if entry == "forward":
                fwd(mk, "corner", c, ops, dt=dt)
            else:
                bwd(mk, "corner", c, ops, f, Gd, dt=dt, plan=plan)
        made = len(arena.allocs)
    assert shrunk.sizes and all(n > 1 for n in shrunk.sizes), shrunk.sizes
    assert made >= 3  # the outputs and the short workspace came from the arena
    arena.check()
    assert arena.untouched()


# ------------------------------------------------------------------------------- streams
def test_repeatable_on_the_current_stream_and_captured(mk, cuda):
    """Bitwise repeatable with the allocator's free blocks filled with 0x00 and 0xFF; ordered on
    a side stream made current; one hipGraph capture of the forward followed by the backward
    replayed twice equals the eager result bitwise: the seed travels by value, a replay applies
    the same mask.  H = 5."""
    H = 5
    c, G, _ = shared("corner")
    g = c["g"]
    rp, col = dev_graph("corner")
    plan = mk.transpose_plan(col, g.C)
    ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    for chunk in (0, 64):
        runs = []
        for fill in (0x00, 0xFF):
            junk = [torch.full((n,), fill, dtype=torch.uint8, device=cuda)
                    for n in (64 << 20, 4 * H * g.R * 256, 4096)]
            del junk
            f = fwd(mk, "corner", c, ops, chunk)
            runs.append((*f, *bwd(mk, "corner", c, ops, f, Gd, chunk)))
        for x, y in zip(*runs):
            assert M.same_bytes(x, y)
        eager = runs[0]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            G2 = torch.zeros_like(Gd)
            for _ in range(20):  # queued on the side stream before the calls
                G2 = G2 + Gd / 20
            G2.copy_(Gd)
            f = fwd(mk, "corner", c, ops, chunk)
            res = (*f, *bwd(mk, "corner", c, ops, f, G2, chunk))
        side.synchronize()
        for x, y in zip(eager, res):
            assert M.same_bytes(x, y)
        hg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(hg, stream=side):
            f2 = fwd(mk, "corner", c, ops, chunk, validate=False)
            got = bwd(mk, "corner", c, ops, f2, Gd, chunk, validate=False, plan=plan)
        for _ in range(2):
            for t in (*f2, *got):
                t.fill_(float("nan"))
            hg.replay()
            torch.cuda.synchronize()
            for x, y in zip(eager, (*f2, *got)):
                assert M.same_bytes(x, y)


# ------------------------------------------------------------------------------- autograd
def test_autograd_three_modes(mk, cuda, monkeypatch):
    """H = 3 on graph S, D = 64, k = 16, dropout 0.5 under a fixed seed, a random cotangent:
    stored + the elementwise mask, fused + rebuilt and fused + fused each inside the reference's
    bounds.  The fused function saves nothing of H * E elements where the stored path does, and
    under dropout exactly the tensors it saves without (only the two numbers are added: no mask);
    with the fused backward it saves exactly `out` [H, V, D] more.  (On this graph q [H, V, D],
    an input the function has always saved, is itself larger than H * E, so the check is on the
    saved set, not on a size limit.)  The 7- and 8-argument apply forms are bitwise
    mk.dot_attention_heads."""
    import maxk_layers as ML
    import maxk_spgemm_function as MF
    for v in ("MAXK_BWD_MODE", "MAXK_DOT_ATTN_BWD"):
        monkeypatch.delenv(v, raising=False)
    D, k, H = 64, 16, 3
    c, G, refs = shared("S", k, D)
    g = c["g"]
    E = g.col.size
    p, seed, s = c["p"], c["seed"], c["scale"]
    rp, col = dev_graph("S")
    graph_ = ML.CSRGraph(rp, col)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    ad = DA.heads_slice(c["ad"], H)
    b, feat = refs.b["own"], refs.feat("own", H)
    gq_b, gt_b = refs.rebuilt(H)
    saved = {}
    for mode in ("stored", "rebuilt", "fused"):
        q, tv, ci = dev_case(c, H)
        for t in (q, tv):
            t.requires_grad_(True)
        sizes = []
        with torch.autograd.graph.saved_tensors_hooks(
                lambda t: sizes.append((t.dtype, t.numel())) or t, lambda t: t):
            if mode == "stored":
                logits = MF.maxk_dot_scores_heads(rp, col, q, tv, ci, s)
                alpha = torch.stack([ML.edge_softmax(graph_, logits[h]) for h in range(H)])
                y = graph_.aggregate_heads(tv, ci, D, MF.maxk_edge_dropout_heads(alpha, p, seed))
            else:
                y = graph_.dot_attend_heads(tv, ci, D, q, s, mode, dropout=p, seed=seed)
        y.backward(Gd)
        saved[mode] = sizes
        if mode == "stored":
            assert (torch.float32, H * E) in sizes
            # the stored composition: the bounds of the rebuilt sequence (the same passes)
            check(y.detach(), ad.out, ad.out_bound, "autograd stored out")
            check(q.grad, b.g_q[:H], gq_b, "autograd stored grad_q")
            check(tv.grad, feat[0], gt_b, "autograd stored grad_cbsr")
            continue
        assert sizes and not any(dt == torch.float32 and n in (E, H * E) for dt, n in sizes)
        plain_sizes = []
        with torch.autograd.graph.saved_tensors_hooks(
                lambda t: plain_sizes.append((t.dtype, t.numel())) or t, lambda t: t):
            graph_.dot_attend_heads(tv, ci, D, q, s, mode)
        assert sorted(sizes, key=str) == sorted(plain_sizes, key=str), (sizes, plain_sizes)
        if mode == "fused":  # the fused backward keeps `out` [H, V, D] as well, and nothing else
            assert sorted(sizes, key=str) == sorted(
                saved["rebuilt"] + [(torch.float32, H * g.R * D)], key=str), sizes
        check(y.detach(), ad.out, ad.out_bound, f"autograd {mode} out")
        check(q.grad, b.g_q[:H], b.g_q_bound[:H] if mode == "fused" else gq_b,
              f"autograd {mode} grad_q")
        check(tv.grad, feat[0], feat[1] if mode == "fused" else gt_b,
              f"autograd {mode} grad_cbsr")
    q, tv, ci = dev_case(c, H)
    y7 = MF.MaxKDotAttentionHeadsFunction.apply(rp, col, q, tv, ci, D, s)[0]
    y8 = MF.MaxKDotAttentionHeadsFunction.apply(rp, col, q, tv, ci, D, s, "fused")[0]
    plain = mk.dot_attention_heads(rp, col, q, tv, ci, D, s)[0]
    assert M.same_bytes(y7, plain) and M.same_bytes(y8, plain)


# ------------------------------------------------------------------------------- the layer
def test_transformer_conv_fused_attn_drop(cuda, monkeypatch):
    """MaxKTransformerConv(64, 8, 4, attn_drop=0.5, fused_attn_drop=True) at V = 300 with one hub
    and empty rows (the problem of test_transformer_conv_fused_matches_stored_and_dense), a fixed
    attn_seed, in training mode: the three combinations of attention / attention_backward against
    the dense float64 layer that multiplies the reference's mask into its masked softmax -- the
    output, every parameter's gradient and both input gradients at rtol = atol = 1e-4.  The same
    attn_seed gives the same bytes; two training forwards without attn_seed differ; after the
    same torch.manual_seed they are bitwise equal; after eval() the layer is bitwise the layer
    without dropout."""
    import maxk_layers as ML
    for v in ("MAXK_DOT_ATTN", "MAXK_DOT_ATTN_BWD", "MAXK_BWD_MODE"):
        monkeypatch.delenv(v, raising=False)
    torch.manual_seed(4)
    rng = np.random.default_rng(300)
    V, D, k, O_, H, p, seed = 300, 64, 16, 8, 4, 0.5, 987654321
    rp, col = rand_graph(rng, V, 8, hubs=((7, 220),), empty=3)
    graph_ = ML.CSRGraph(T(rp.astype(np.int32), cuda), T(col.astype(np.int32), cuda))
    conv = ML.MaxKTransformerConv(D, O_, H, attn_drop=p, fused_attn_drop=True).to(cuda)
    plain = ML.MaxKTransformerConv(D, O_, H).to(cuda)
    with torch.no_grad():
        conv.bias.normal_()
    plain.load_state_dict(conv.state_dict())
    x = torch.randn(V, D, device=cuda)
    xs, vals, idx = ML.maxk(x, k)
    xs = xs.detach().requires_grad_(True)
    vals = vals.detach().requires_grad_(True)
    gout = torch.randn(V, H, O_, device=cuda)
    names = ["fc_q.weight", "fc_k.weight", "fc_v.weight", "bias"]
    P = dict(conv.named_parameters())

    rows = torch.repeat_interleave(torch.arange(V, device=cuda),
                                   T(np.diff(rp).astype(np.int64), cuda))
    cols = T(col.astype(np.int64), cuda)
    A = torch.zeros(V, V, dtype=torch.float64, device=cuda)
    A[rows, cols] = 1.0
    Dm = torch.zeros(H, V, V, dtype=torch.float64, device=cuda)
    Dm[:, rows, cols] = T(AD.mask(H, col.size, p, seed), cuda)
    Q = {n: P[n].detach().double().requires_grad_(True) for n in names}
    xs2 = xs.detach().double().requires_grad_(True)
    vals2 = vals.detach().double().requires_grad_(True)
    xv = torch.zeros(V, D, dtype=torch.float64, device=cuda).scatter(1, idx.long(), vals2)
    masked = (A == 0) & (A.sum(1, keepdim=True) > 0)
    heads = []
    for h in range(H):
        Wq, Wk, Wv = (Q[n][h * O_:(h + 1) * O_] for n in names[:3])
        e = (xs2 @ Wq.t()) @ (xv @ Wk.t()).t() / O_ ** 0.5
        al = torch.softmax(e.masked_fill(masked, float("-inf")), 1) * A * Dm[h]
        heads.append(al @ (xv @ Wv.t()) + Q["bias"][h])
    ref = torch.stack(heads, 1)
    want = torch.autograd.grad(ref, [Q[n] for n in names] + [xs2, vals2], gout.double())
    empty = T(np.diff(rp) == 0, cuda)
    assert conv.training
    for attention, backward in (("stored", "rebuilt"), ("fused", "rebuilt"), ("fused", "fused")):
        conv.attention = plain.attention = attention
        conv.attention_backward = plain.attention_backward = backward
        conv.train()
        out = conv(graph_, xs, vals, idx, attn_seed=seed)
        got = torch.autograd.grad(out, [P[n] for n in names] + [xs, vals], gout)
        torch.testing.assert_close(out, ref.float(), rtol=1e-4, atol=1e-4)
        for n, a, b in zip(names + ["x_sparse", "topk_values"], got, want):
            torch.testing.assert_close(a, b.float(), rtol=1e-4, atol=1e-4,
                                       msg=lambda m: f"{attention} {backward} {n}: {m}")
        assert not out[empty].sub(conv.bias).abs().max() > 0  # empty rows: the bias alone
        assert M.same_bytes(out, conv(graph_, xs, vals, idx, attn_seed=seed).detach())
        a, b = (conv(graph_, xs, vals, idx).detach() for _ in range(2))
        assert not M.same_bytes(a, b)
        torch.manual_seed(9)
        a = conv(graph_, xs, vals, idx).detach()
        torch.manual_seed(9)
        assert M.same_bytes(a, conv(graph_, xs, vals, idx).detach())
        conv.eval()
        assert M.same_bytes(conv(graph_, xs, vals, idx).detach(),
                            plain(graph_, xs, vals, idx).detach())


def test_ratios_are_reported():
    """Last in the file: the largest err/bound ratios seen, for the record."""
    for what, r in sorted(RATIOS.items(), key=lambda kv: -kv[1])[:16]:
        print(f"{r:.3f}  {what}")
    assert all(r <= 1.0 for r in RATIOS.values())
