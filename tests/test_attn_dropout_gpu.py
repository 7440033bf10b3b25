"""GPU: attention dropout under the stored-nowhere Philox mask -- mk.edge_dropout_heads
(attn_dropout.hip), mk.gat_attention_heads(dropout=, seed=) (gath_fwd_kernel<.., true>,
softmax_fixup_kernel<true> of heads_walk.h), mk.gat_attention_heads_backward(dropout=, seed=)
(gath_bwd_kernel<.., true>), the autograd functions and the two GAT layers -- against
tests/attn_dropout_ref.py (numpy Philox, float64, derived bounds).

Which kernels.  HP = 2, 4, 8 for H = 1 / 2, 3, 5 / 8; KG = 8 for k = 3, 5, 7, 16 for k = 16,
64 for k = 96.  test_forward_parity runs k in 3, 16, 96, 7 at H in 1, 3, 8; test_backwards runs
k = 16 at H in 2, 5, 8 and k = 7; the selector tests k = 5.

The largest err / bound seen on an MI355X is in test_ratios_are_reported's output and in
profiles/r17/attn_dropout/README.md.
"""
import functools

import numpy as np
import pytest
import torch

import attn_dropout_ref as DR
import esm_corner_graph as EG
import gat_attention_bwd_ref as BR
import gat_attention_ref as AR
import memguard as M
import numerics as N
from test_gat_attention_bwd_gpu import cotangent
from test_gat_attention_gpu import (DEV, SLOPE, case, dev_case, dev_graph, feat_grad_ref,
                                    the_graph)
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
    """The case c (test_gat_attention_gpu.make_case) with the dropped reference at HMAX heads."""
    g = c["g"]
    ad, _, d = DR.attention(g.rp, g.col, c["s_dst"], c["s_src"], SLOPE, c["cv"], c["ci"], c["D"],
                            c["n"], p, seed, base=c["a"])
    return dict(c, ad=ad, d=d, p=p, seed=seed)


@functools.lru_cache(maxsize=None)
def dcase(name, k=16, D=256, p=0.5, seed=SEED):
    """The cases several tests share: computed once, never modified."""
    return drop_case(case(name, k, D), p, seed)


class Refs:
    """The backward references of one dropped case and one G at HMAX heads, the kernel's own
    forward as `out`; the feature gradient per number of heads."""

    def __init__(self, c, G):
        self.c, self.G = c, G
        self.ers = BR.edge_grads(c["g"], c["cv"], c["ci"], G)
        self.b = DR.backward(c["g"], c["a"], c["ad"], c["d"], c["cv"], c["ci"], G, SLOPE, c["D"],
                             c["ad"].out_bound, ers=self.ers)

    @functools.lru_cache(maxsize=None)
    def feat(self, H):
        c = self.c
        with np.errstate(invalid="ignore", over="ignore"):
            return feat_grad_ref(c["g"], AR.heads_slice(c["ad"], H), self.G[:H], c["ci"], c["D"])

    @functools.lru_cache(maxsize=None)
    def rebuilt(self, H):
        c = self.c
        return DR.rebuilt_backward(c["g"], AR.heads_slice(c["a"], H), c["d"][:H], self.ers[:H],
                                   SLOPE)


@functools.lru_cache(maxsize=None)
def shared(name, k=16, D=256, p=0.5, seed=SEED):
    c = dcase(name, k, D, p, seed)
    G = cotangent(c)
    return c, G, Refs(c, G)


def fwd(mk, name, c, ops, chunk=0, dt=None, **kw):
    rp, col = dev_graph(name) if dt is None else dt
    sd, ss, cv, ci = ops
    return mk.gat_attention_heads(rp, col, sd, ss, cv, ci, c["D"], SLOPE, chunk=chunk,
                                  dropout=c["p"], seed=c["seed"], **kw)


def bwd(mk, name, c, ops, f, G, chunk=0, dt=None, **kw):
    rp, col = dev_graph(name) if dt is None else dt
    sd, ss, cv, ci = ops
    return mk.gat_attention_heads_backward(rp, col, sd, ss, cv, ci, *f, G, SLOPE, chunk=chunk,
                                           dropout=c["p"], seed=c["seed"], **kw)


def rebuilt_bwd(mk, name, c, ops, f, G, chunk=0):
    """gat_edge_alpha_heads, then the mask, then the stored passes."""
    rp, col = dev_graph(name)
    sd, ss, cv, ci = ops
    alpha = mk.gat_edge_alpha_heads(rp, col, sd, ss, f[1], f[2], SLOPE)
    gw = mk.edge_weight_grad_heads(rp, col, cv, ci, G, chunk=chunk)
    mk.edge_dropout_heads(gw, c["p"], c["seed"], out=gw)
    g_dst, g_src = mk.gat_edge_softmax_heads_backward(rp, col, sd, ss, alpha, gw, SLOPE,
                                                      chunk=chunk)
    mk.edge_dropout_heads(alpha, c["p"], c["seed"], out=alpha)
    return g_dst, g_src, mk.sspmm_backward_heads(rp, col, alpha, G, ci, chunk=chunk)


def check(y, ref, bound, what):
    assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape, (y.shape, ref.shape)
    r = N.within(y, ref, bound, what)
    RATIOS[what] = max(r, RATIOS.get(what, 0.0))
    print(f"{what}: err/bound {r:.3f}")
    return r


def check_fwd(c, H, res, what):
    """out inside the dropped bound, the statistics inside the undropped softmax's; exact zeros
    where nothing is added."""
    g, ad = c["g"], AR.heads_slice(c["ad"], H)
    out, m, z = res
    check(out, ad.out, ad.out_bound, f"{what} out")
    check(m, ad.m, ad.m_bound, f"{what} row_max")
    check(z, ad.z, ad.z_bound, f"{what} row_sum")
    empty = T(np.diff(g.rp) == 0, DEV)
    assert not out[:, empty].any() and not m[:, empty].any() and not z[:, empty].any()
    assert not out[:, T(c["n"] == 0, DEV)].any()


def check_bwd(c, H, res, b, feat, what):
    g = c["g"]
    g_dst, g_src, g_cbsr = res
    check(g_dst, b.g_dst[:H], b.g_dst_bound[:H], f"{what} grad_s_dst")
    check(g_src, b.g_src[:H], b.g_src_bound[:H], f"{what} grad_s_src")
    check(g_cbsr, feat[0], feat[1], f"{what} grad_cbsr")
    assert not g_dst[:, T(np.diff(g.rp) == 0, DEV)].any()
    if g.unread is not None:
        assert not g_src[:, g.unread].any() and not g_cbsr[g.unread].any()


# ------------------------------------------------------------------------------- the mask
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("H", [1, 3, 5, 8])
def test_mask(mk, cuda, H, p):
    """edge_dropout_heads on ones equals ref.mask exactly -- the same kept set, the kept values
    exactly scale -- at E = 1, 63 * 64 + 1 and graph S's; in place gives the same."""
    for E in (1, 63 * 64 + 1, the_graph("S").col.size):
        want = DR.mask(H, E, p, SEED).astype(np.float32)
        w = torch.ones(H, E, device=cuda)
        out = mk.edge_dropout_heads(w, p, SEED)
        assert out is not w and bool((w == 1).all())
        assert np.array_equal(out.cpu().numpy(), want), (H, E, p)
        assert set(np.unique(want)) <= {0.0, float(DR.scale(p))}
        assert mk.edge_dropout_heads(w, p, SEED, out=w) is w
        assert M.same_bytes(w, out)
    assert not np.array_equal(mk.edge_dropout_heads(torch.ones(H, 4033, device=cuda), p,
                                                    SEED + 1).cpu().numpy(),
                              DR.mask(H, 4033, p, SEED).astype(np.float32))


def test_mask_multiplies(mk, cuda):
    """out = w * d as IEEE has it: the kept weights the correctly rounded product, a dropped NaN
    or Inf NaN, a seed past 32 bits."""
    H, E, p, seed = 5, 1000, 0.5, (7 << 40) + 3
    w = np.random.default_rng(3).standard_normal((H, E)).astype(np.float32)
    w[:, 5] = np.nan
    w[:, 6] = np.inf
    d = DR.mask(H, E, p, seed).astype(np.float32)
    assert (d[:, 5] == 0).any() and (d[:, 6] == 0).any() and (d[:, 6] > 0).any()
    with np.errstate(invalid="ignore"):
        want = w * d
    got = mk.edge_dropout_heads(T(w, cuda), p, seed).cpu().numpy()
    assert np.array_equal(got, want, equal_nan=True)


# ------------------------------------------------------------------------------- forward
SHAPES = [(3, 64), (16, 256), (96, 256), (7, 9)]


@pytest.mark.parametrize("k,D", SHAPES, ids=[f"k{k}-D{D}" for k, D in SHAPES])
@pytest.mark.parametrize("name", ["S", "Dn", "R", "corner"])
def test_forward_parity(mk, cuda, name, k, D):
    """out inside the dropped reference's bound at H in 1, 3, 8 and every item size of the sweep;
    row_max and row_sum bitwise those of the call without dropout at the same item size; p = 0
    bitwise equal in all three outputs."""
    c = drop_case(case(name, k, D), 0.5, SEED)
    rp, col = dev_graph(name)
    for H in (1, 3, 8):
        ops = dev_case(c, H)
        for chunk in CHUNKS:
            res = fwd(mk, name, c, ops, chunk)
            check_fwd(c, H, res, f"{name} k{k} D{D} H{H}")
            plain = mk.gat_attention_heads(rp, col, *ops, D, SLOPE, chunk=chunk)
            assert M.same_bytes(res[1], plain[1]) and M.same_bytes(res[2], plain[2]), chunk
            assert not M.same_bytes(res[0], plain[0])
            zero = mk.gat_attention_heads(rp, col, *ops, D, SLOPE, chunk=chunk, dropout=0.0,
                                          seed=SEED)
            for x, y in zip(zero, plain):
                assert M.same_bytes(x, y), chunk


@pytest.mark.parametrize("p", [0.1, 0.9])
def test_forward_rates(mk, cuda, p):
    """The other two rates on the corner graph, H = 5."""
    c = dcase("corner", 16, 256, p)
    ops = dev_case(c, 5)
    for chunk in (0, 64, 7):
        check_fwd(c, 5, fwd(mk, "corner", c, ops, chunk), f"corner p{p} H5")


def test_mask_does_not_depend_on_the_partition(mk, cuda):
    """Two item sizes on the corner graph cut the rows differently: the exactly-zero and the
    non-zero output elements are the same set, and both meet the bound."""
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
    whose edges are dropped in some head.  Their out is exact zeros, and their grad_s_dst is
    within the bound of the reference's exact 0."""
    H = 3
    c, G, refs = shared("S", 16, 256, 0.9, FULL_SEED)
    g = c["g"]
    deg = np.diff(g.rp)
    kept = np.stack([np.add.reduceat(c["d"][h] > 0, g.rp[:-1][deg > 0]) for h in range(H)])
    full = np.zeros((H, g.R), bool)
    full[:, deg > 0] = kept == 0
    full &= (deg >= 2)[None]
    assert full.any(), "no fully dropped row of degree >= 2 under this seed"
    assert np.isfinite(c["ad"].out[:H]).all()
    assert (c["ad"].out[:H][full] == 0).all() and (refs.b.g_dst[:H][full] == 0).all()
    ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    fd = T(full, DEV)
    for chunk in (0, 64, 2):
        f = fwd(mk, "S", c, ops, chunk)
        assert not f[0][fd].any()
        assert bool((f[2][fd] > 0).all())  # the statistics are the undropped softmax's
        res = bwd(mk, "S", c, ops, f, Gd, chunk)
        check_bwd(c, H, res, refs.b, refs.feat(H), f"fully dropped chunk {chunk}")
        err = res[0][fd].abs().double().cpu().numpy()
        assert (err <= refs.b.g_dst_bound[:H][full]).all()


# ------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("H", [2, 5, 8])
@pytest.mark.parametrize("name,k,D", [("S", 16, 256), ("R", 7, 9), ("corner", 16, 256)])
def test_backwards(mk, cuda, name, k, D, H):
    """The fused backward and the rebuilt one (gat_edge_alpha_heads, the mask, the stored passes)
    inside the reference's bounds; grad_cbsr of the two within the summed bounds; p = 0 bitwise
    the call without dropout."""
    c, G, refs = shared(name, k, D)
    ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    b, feat, st = refs.b, refs.feat(H), refs.rebuilt(H)
    for chunk in (0, 64, 7):
        f = fwd(mk, name, c, ops, chunk)
        fused = bwd(mk, name, c, ops, f, Gd, chunk)
        check_bwd(c, H, fused, b, feat, f"fused {name} H{H}")
        reb = rebuilt_bwd(mk, name, c, ops, f, Gd, chunk)
        check(reb[0], st.g_dst, st.g_dst_bound, f"rebuilt {name} H{H} grad_s_dst")
        check(reb[1], st.g_src, st.g_src_bound, f"rebuilt {name} H{H} grad_s_src")
        check(reb[2], feat[0], feat[1], f"rebuilt {name} H{H} grad_cbsr")
        err = (fused[2].double() - reb[2].double()).abs().cpu().numpy()
        assert (err <= 2 * feat[1]).all()
    rp, col = dev_graph(name)
    plain_f = mk.gat_attention_heads(rp, col, *ops, D, SLOPE)
    plain = mk.gat_attention_heads_backward(rp, col, *ops, *plain_f, Gd, SLOPE)
    zero = mk.gat_attention_heads_backward(rp, col, *ops, *plain_f, Gd, SLOPE, dropout=0.0,
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
        check_bwd(c, H, bwd(mk, "corner", c, ops, f, Gd, chunk), refs.b, refs.feat(H),
                  f"fused corner p{p}")


# ------------------------------------------------------------------------------- selectors
def test_skipped_and_repeated_selectors(mk, cuda):
    """k = 5, D = 24 with selectors >= D (skipped; their gradient slots an exact 0) and repeated
    inside a vertex, dropout on, both directions.  KG = 8, HP = 4."""
    from test_gat_attention_gpu import make_case
    k, D, H = 5, 24, 3
    g = the_graph("S")
    rng = np.random.default_rng(2500 + k)
    ci = N.selectors(rng, g.C, 256, k)
    dup = rng.choice(g.C, g.C // 4, replace=False)
    ci[dup, k - 1] = ci[dup, 0]
    c = drop_case(make_case("S", k, D, ci=ci), 0.5, SEED)
    assert (ci >= D).any() and (c["n"] == 0).any()
    G = cotangent(c)
    refs = Refs(c, G)
    ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    for chunk in (0, 64):
        f = fwd(mk, "S", c, ops, chunk, validate=False)
        check_fwd(c, H, f, f"selectors k{k} D{D}")
        res = bwd(mk, "S", c, ops, f, Gd, chunk, validate=False)
        check_bwd(c, H, res, refs.b, refs.feat(H), f"selectors k{k} D{D}")
        assert not res[2][T(ci >= D, DEV)].any()
        kept = dup[ci[dup, 0] < D]
        assert M.same_bytes(res[2][T(kept, DEV), k - 1].contiguous(),
                            res[2][T(kept, DEV), 0].contiguous())


# ------------------------------------------------------------------------------- non-finite
def test_non_finite(mk, cuda):
    """Head 1 of 3 on graph S: a NaN in s_src[1, c] and, at another column, an Inf in the value
    of an edge that head 1 drops.  The forward gives what numpy's IEEE evaluation of the
    reference gives (0 * Inf is NaN: dropping does not shield; the heads that keep the edge see
    the Inf); with the NaN score alone, the backward the same."""
    H = 3
    base = dcase("S")
    g, d = base["g"], base["d"]
    readers = N._readers(g)
    deg = np.diff(g.rp)
    hubs = np.flatnonzero(deg > 100)
    nan_col = next(int(v) for v in range(g.C)
                   if readers[v].size >= 2 and not np.isin(readers[v], hubs).any())
    rows = np.repeat(np.arange(g.R), deg)
    e_inf = next(int(e) for e in range(g.col.size)
                 if d[1, e] == 0 and d[0, e] > 0 and g.col[e] != nan_col
                 and rows[e] not in hubs and not np.isin(readers[g.col[e]], hubs).any()
                 and not np.isin(readers[g.col[e]], readers[nan_col]).any())
    s_src = base["s_src"].copy()
    s_src[1, nan_col] = np.nan
    for with_inf in (False, True):
        cv = base["cv"].copy()
        if with_inf:
            cv[g.col[e_inf], 0] = np.inf
        a = AR.attention(g.rp, g.col, base["s_dst"], s_src, SLOPE, cv, base["ci"], 256, base["n"])
        c = drop_case(dict(base, s_src=s_src, cv=cv, a=a), 0.5, SEED)
        ad = c["ad"]
        r, j = rows[e_inf], base["ci"][g.col[e_inf], 0]
        if with_inf:
            assert np.isnan(ad.out[1, r, j]) and np.isposinf(ad.out[0, r, j])
        assert np.isnan(ad.out[1, readers[nan_col]]).any()
        assert np.isfinite(ad.out[[0, 2]]).mean() > 0.9
        ops = dev_case(c, H)
        for chunk in (0, 64):
            f = fwd(mk, "S", c, ops, chunk)
            check_fwd(c, H, f, f"non-finite inf {with_inf}")
            if not with_inf:
                G = cotangent(c)
                refs = Refs(c, G)
                assert np.isnan(refs.b.g_dst[1, readers[nan_col]]).all()
                res = bwd(mk, "S", c, ops, f, T(np.ascontiguousarray(G[:H]), DEV), chunk)
                check_bwd(c, H, res, refs.b, refs.feat(H), "non-finite")


@pytest.mark.parametrize("H,h", [(3, 1), (8, 6)])
def test_head_isolation(mk, cuda, H, h):
    """The other heads' scores replaced: head h's slices of out, the statistics, grad_s_dst and
    grad_s_src keep their bytes, dropout on."""
    c, G, _ = shared("corner")
    rng = np.random.default_rng(2600 + H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    for chunk in (0, 64, 7):
        ops = dev_case(c, H)
        f = fwd(mk, "corner", c, ops, chunk)
        base = bwd(mk, "corner", c, ops, f, Gd, chunk)
        arrs = []
        for name in ("s_dst", "s_src"):
            x = rng.standard_normal(c[name][:H].shape).astype(np.float32)
            x[h] = c[name][h]
            arrs.append(x)
        ops2 = dev_case(c, H, *arrs)
        f2 = fwd(mk, "corner", c, ops2, chunk)
        other = bwd(mk, "corner", c, ops2, f2, Gd, chunk)
        for x, y in zip((*f, *base[:2]), (*f2, *other[:2])):
            assert M.same_bytes(x[h].contiguous(), y[h].contiguous()), chunk
        assert not M.same_bytes(f[0], f2[0])


# ------------------------------------------------------------------------------- memory
@pytest.fixture(scope="module")
def arena(cuda):
    return M.Arena(48 << 20, cuda)


@pytest.mark.parametrize("k,D,H", [(16, 256, 3), (3, 64, 8)])
def test_memory_contract(mk, arena, cuda, k, D, H):
    """The three entries with outputs and workspace from the poisoned, guarded arena (the
    workspace exactly the queried size): outputs fully written and the same bytes in every fill
    regime, guards untouched, inputs unchanged."""
    c, G, refs = shared("corner", k, D)
    g = c["g"]
    E = g.col.size
    p, seed = c["p"], c["seed"]
    Gd = T(np.ascontiguousarray(G[:H]), DEV)

    def same(res):
        for regime in ("stale", "ones"):
            for x, y in zip(res["zero"], res[regime]):
                assert M.same_bytes(x, y), regime

    w = torch.ones(H, E, device=DEV)
    res = M.run_regimes(lambda w_: (mk.edge_dropout_heads(w_, p, seed),),
                        lambda primer: (torch.rand_like(w) if primer else w.clone(),), arena)
    assert sorted(x.nbytes for x in arena.allocs) == [4 * H * E]
    same(res)
    assert np.array_equal(res["ones"][0].cpu().numpy(), c["d"][:H].astype(np.float32))

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
            return mk.gat_attention_heads(dt[0], dt[1], sd, ss, cv, ci, D, SLOPE, chunk=chunk,
                                          dropout=p, seed=seed)

        res = M.run_regimes(op, factory, arena)
        n_ws = mk._lib().maxk_gat_attention_heads_dropout_workspace_size(g.R, g.C, E, D, k, H,
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
                ops = tuple(torch.rand(t.shape, generator=gen, device=DEV) for t in ops[:3]) \
                    + (ops[3],)
                rest = tuple(torch.rand(t.shape, generator=gen, device=DEV) + 0.5 for t in rest)
            return (dt, plan) + ops + rest

        def op_b(dt, plan, sd, ss, cv, ci, out, m, z, G_):
            return mk.gat_attention_heads_backward(dt[0], dt[1], sd, ss, cv, ci, out, m, z, G_,
                                                   SLOPE, chunk=chunk, plan=plan, dropout=p,
                                                   seed=seed)

        res = M.run_regimes(op_b, factory_b, arena)
        n_ws = mk._lib().maxk_gat_attention_heads_dropout_backward_workspace_size(
            g.R, g.C, E, D, k, H, chunk)
        assert sorted(x.nbytes for x in arena.allocs) == sorted(
            [4 * H * g.R, 4 * H * g.C, 4 * g.C * k, n_ws])
        same(res)
        check_bwd(c, H, res["ones"], refs.b, refs.feat(H), f"memguard k{k} D{D} H{H}")


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
    shrunk = Shrunk(mk._L, {"forward": "maxk_gat_attention_heads_dropout_workspace_size",
                            "backward": "maxk_gat_attention_heads_dropout_backward_workspace_size"
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
    assert made >= 4
    arena.check()
    assert arena.untouched()


# ------------------------------------------------------------------------------- streams
def test_repeatable_on_the_current_stream_and_captured(mk, cuda):
    """Bitwise repeatable with the allocator's free blocks filled with 0x00 and 0xFF; ordered on
    a side stream made current; one hipGraph capture of the forward, the backward and the
    elementwise mask replayed twice equals the eager result bitwise: the seed travels by value,
    a replay applies the same mask.  H = 5."""
    H = 5
    c, G, _ = shared("corner")
    g = c["g"]
    rp, col = dev_graph("corner")
    plan = mk.transpose_plan(col, g.C)
    ops = dev_case(c, H)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    ones = torch.ones(H, g.col.size, device=DEV)
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
        eager_d = mk.edge_dropout_heads(ones, c["p"], c["seed"])
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
            dd = mk.edge_dropout_heads(ones, c["p"], c["seed"])
        for _ in range(2):
            for t in (*f2, *got, dd):
                t.fill_(float("nan"))
            hg.replay()
            torch.cuda.synchronize()
            for x, y in zip((*eager, eager_d), (*f2, *got, dd)):
                assert M.same_bytes(x, y)


# ------------------------------------------------------------------------------- autograd
def test_autograd_three_modes(mk, cuda, monkeypatch):
    """H = 3 on graph S, dropout 0.5 under a fixed seed, a random cotangent: stored + the
    elementwise mask, fused + rebuilt and fused + fused each inside the reference's bounds; the
    fused function saves no tensor of H * E or more elements where the stored path saves two --
    with the fused backward it saves `out` [H, V, D] besides, as without dropout, and nothing
    of the mask either way."""
    import maxk_layers as ML
    import maxk_spgemm_function as MF
    monkeypatch.delenv("MAXK_BWD_MODE", raising=False)
    monkeypatch.delenv("MAXK_HEADS_ATTN_BWD", raising=False)
    D, k, H = 64, 16, 3
    c, G, refs = shared("S", k, D)
    g = c["g"]
    E = g.col.size
    p, seed = c["p"], c["seed"]
    rp, col = dev_graph("S")
    graph_ = ML.CSRGraph(rp, col)
    Gd = T(np.ascontiguousarray(G[:H]), DEV)
    ad = AR.heads_slice(c["ad"], H)
    st, feat = refs.rebuilt(H), refs.feat(H)
    saved = {}
    for mode in ("stored", "rebuilt", "fused"):
        sd, ss, tv, ci = dev_case(c, H)
        for t in (sd, ss, tv):
            t.requires_grad_(True)
        sizes = []
        with torch.autograd.graph.saved_tensors_hooks(
                lambda t: sizes.append(t.numel()) or t, lambda t: t):
            if mode == "stored":
                alpha = ML.gat_edge_softmax_heads(graph_, sd, ss, SLOPE)
                y = graph_.aggregate_heads(tv, ci, D, MF.maxk_edge_dropout_heads(alpha, p, seed))
            else:
                y = graph_.attend_heads(tv, ci, D, sd, ss, SLOPE, mode, dropout=p, seed=seed)
        y.backward(Gd)
        saved[mode] = sizes
        if mode == "stored":
            assert max(sizes) >= H * E
        elif mode == "rebuilt":
            assert sizes and max(sizes) < H * E, sizes
        else:  # the fused backward keeps `out` [H, V, D] as well, and nothing else
            assert sorted(sizes) == sorted(saved["rebuilt"] + [H * g.R * D]), sizes
        check(y.detach(), ad.out, ad.out_bound, f"autograd {mode} out")
        b = refs.b if mode == "fused" else st
        check(sd.grad, b.g_dst[:H], b.g_dst_bound[:H], f"autograd {mode} s_dst.grad")
        check(ss.grad, b.g_src[:H], b.g_src_bound[:H], f"autograd {mode} s_src.grad")
        check(tv.grad, feat[0], feat[1], f"autograd {mode} topk_values.grad")
    # the existing call forms are untouched: 8 and 9 arguments, no dropout
    sd, ss, tv, ci = dev_case(c, H)
    y8 = MF.MaxKGATAttentionHeadsFunction.apply(rp, col, sd, ss, tv, ci, D, SLOPE)[0]
    y9 = MF.MaxKGATAttentionHeadsFunction.apply(rp, col, sd, ss, tv, ci, D, SLOPE, "fused")[0]
    plain = mk.gat_attention_heads(rp, col, sd, ss, tv, ci, D, SLOPE)[0]
    assert M.same_bytes(y8, plain) and M.same_bytes(y9, plain)


# ------------------------------------------------------------------------------- layers
def dense_gat(P, names, xs, vals, idx, A, Dm, H, O_, gout):
    """The multi-head GAT layer in dense float64 torch, Dm [H, V, V] multiplied into the masked
    softmax; returns (out, the gradients of the parameters, x_sparse and topk_values)."""
    V, D = xs.shape
    Q = {n: P[n].detach().double().requires_grad_(True) for n in names}
    xs2 = xs.detach().double().requires_grad_(True)
    vals2 = vals.detach().double().requires_grad_(True)
    xv = torch.zeros(V, D, dtype=torch.float64, device=xs.device).scatter(1, idx.long(), vals2)
    masked = (A == 0) & (A.sum(1, keepdim=True) > 0)
    W = Q["fc.weight"].view(H, O_, D)
    a_dst, a_src, bias = (Q[n].view(H, O_) for n in ("attn_dst", "attn_src", "bias"))
    heads = []
    for h in range(H):
        h_s = xs2 @ W[h].t()
        e = torch.nn.functional.leaky_relu(
            (h_s @ a_dst[h])[:, None] + (h_s @ a_src[h])[None, :], 0.2)
        alpha = torch.softmax(e.masked_fill(masked, float("-inf")), 1) * A * Dm[h]
        heads.append(alpha @ (xv @ W[h].t()) + bias[h])
    ref = torch.stack(heads, 1)
    return ref, torch.autograd.grad(ref, [Q[n] for n in names] + [xs2, vals2], gout.double())


def layer_problem(cuda, H):
    import maxk_layers as ML
    rng = np.random.default_rng(300)
    V, D, k = 300, 64, 16
    rp, col = rand_graph(rng, V, 8, hubs=((7, 220),), empty=3)
    graph_ = ML.CSRGraph(T(rp.astype(np.int32), cuda), T(col.astype(np.int32), cuda))
    x = torch.randn(V, D, device=cuda)
    xs, vals, idx = ML.maxk(x, k)
    xs = xs.detach().requires_grad_(True)
    vals = vals.detach().requires_grad_(True)
    rows = torch.repeat_interleave(torch.arange(V, device=cuda),
                                   T(np.diff(rp).astype(np.int64), cuda))
    cols = T(col.astype(np.int64), cuda)
    A = torch.zeros(V, V, dtype=torch.float64, device=cuda)
    A[rows, cols] = 1.0

    def dense_mask(p, seed):
        Dm = torch.zeros(H, V, V, dtype=torch.float64, device=cuda)
        Dm[:, rows, cols] = T(DR.mask(H, col.size, p, seed), cuda)
        return Dm
    return graph_, xs, vals, idx, A, dense_mask, T(np.diff(rp) == 0, cuda)


def test_multi_head_gat_conv_attn_drop(cuda, monkeypatch):
    """MaxKMultiHeadGATConv(64, 8, 4, attn_drop=0.5) at V = 300 with one hub and empty rows, a
    fixed attn_seed, in training mode: the three attention modes against the dense float64 layer
    that multiplies ref.mask into its masked softmax -- the output, every parameter's gradient
    and both input gradients at rtol = atol = 1e-4.  After eval() the layer is bitwise the layer
    with attn_drop = 0; two training forwards without attn_seed differ; after the same
    torch.manual_seed they are bitwise equal."""
    import maxk_layers as ML
    for v in ("MAXK_HEADS_ATTN", "MAXK_HEADS_ATTN_BWD", "MAXK_BWD_MODE"):
        monkeypatch.delenv(v, raising=False)
    torch.manual_seed(4)
    O_, H, p, seed = 8, 4, 0.5, 987654321
    graph_, xs, vals, idx, A, dense_mask, empty = layer_problem(cuda, H)
    V, D = xs.shape
    conv = ML.MaxKMultiHeadGATConv(D, O_, H, negative_slope=0.2, attn_drop=p).to(cuda)
    plain = ML.MaxKMultiHeadGATConv(D, O_, H, negative_slope=0.2).to(cuda)
    with torch.no_grad():
        conv.bias.normal_()
    plain.load_state_dict(conv.state_dict())
    gout = torch.randn(V, H, O_, device=cuda)
    names = ["fc.weight", "attn_src", "attn_dst", "bias"]
    P = dict(conv.named_parameters())
    ref, want = dense_gat(P, names, xs, vals, idx, A, dense_mask(p, seed), H, O_, gout)
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


def test_gat_conv_attn_drop(cuda, monkeypatch):
    """MaxKGATConv(attn_drop=0.5): the same checks at one head."""
    import maxk_layers as ML
    monkeypatch.delenv("MAXK_BWD_MODE", raising=False)
    torch.manual_seed(5)
    O_, p, seed = 8, 0.5, 24680
    graph_, xs, vals, idx, A, dense_mask, empty = layer_problem(cuda, 1)
    V, D = xs.shape
    conv = ML.MaxKGATConv(D, O_, negative_slope=0.2, attn_drop=p).to(cuda)
    plain = ML.MaxKGATConv(D, O_, negative_slope=0.2).to(cuda)
    with torch.no_grad():
        conv.bias.normal_()
    plain.load_state_dict(conv.state_dict())
    gout = torch.randn(V, O_, device=cuda)
    names = ["fc.weight", "attn_src", "attn_dst", "bias"]
    P = dict(conv.named_parameters())
    ref, want = dense_gat(P, names, xs, vals, idx, A, dense_mask(p, seed), 1, O_, gout[:, None])
    out = conv(graph_, xs, vals, idx, attn_seed=seed)
    got = torch.autograd.grad(out, [P[n] for n in names] + [xs, vals], gout)
    torch.testing.assert_close(out, ref[:, 0].float(), rtol=1e-4, atol=1e-4)
    for n, a, b in zip(names + ["x_sparse", "topk_values"], got, want):
        torch.testing.assert_close(a, b.float(), rtol=1e-4, atol=1e-4, msg=lambda m: f"{n}: {m}")
    assert not out[empty].sub(conv.bias).abs().max() > 0
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
