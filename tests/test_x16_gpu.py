"""GPU: the 16-bit-selector path for 1 <= D <= 1024 (x16_topk.hip, x16_fwd.hip, x16_bwd.hip)
through the binding, the autograd function and a layer, against tests/x16_ref.py: the encode and
its adjoint bitwise, the forward and the backward inside tests/numerics.py's bound."""
import functools

import numpy as np
import pytest
import torch

import memguard as M
import numerics as N
import test_gat_attention_gpu as GA
import topk_rows as TR
import x16_ref as XR
from test_parity_gpu import T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ENCODE = [(5, 257, 1), (131, 384, 10), (67, 1024, 256), (64, 513, 32), (257, 256, 16), (5, 7, 7)]
SHAPES = [(257, 3), (384, 16), (384, 32), (512, 96), (1024, 32), (1024, 256), (100, 10)]
GRAPHS = ["S", "Dn", "R"]
IDS = [f"D{D}-k{k}" for D, k in SHAPES]

the_graph, dev_graph = GA.the_graph, GA.dev_graph


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


def i16(a):
    return T(np.asarray(a).astype(np.int16), DEV)


@functools.lru_cache(maxsize=None)
def case(name, D, k, regime):
    """A CBSR of distinct selectors, a grad_out, both float64 references and their bounds:
    computed once, never modified."""
    g = the_graph(name)
    rng = np.random.default_rng(4100 + 7 * D + k)
    ci = XR.topk(rng.standard_normal((g.C, D), dtype=np.float32), k)[1]
    cv, G = N.values(rng, (g.C, k), regime), N.values(rng, (g.R, D), regime)
    return dict(g=g, name=name, D=D, ci=ci, cv=cv, G=G, fwd=XR.fwd(g, cv, ci, D),
                fb=XR.bound_fwd(g, cv, ci, D), bwd=XR.bwd(g, G, ci), bb=XR.bound_bwd(g, G, ci))


def run_fwd(mk, c, chunk, cv=None, ci=None):
    g = c["g"]
    rp, col = dev_graph(c["name"])
    return mk.spgemm_forward_x16(rp, col, T(g.ev, DEV), T(c["cv"] if cv is None else cv, DEV),
                                 i16(c["ci"] if ci is None else ci), c["D"], row_div=T(g.div, DEV),
                                 chunk=chunk, validate=False)


def run_bwd(mk, c, chunk, G=None, ci=None):
    g = c["g"]
    rp, col = dev_graph(c["name"])
    return mk.sspmm_backward_x16(rp, col, T(g.ev, DEV), T(c["G"] if G is None else G, DEV),
                                 i16(c["ci"] if ci is None else ci), row_div=T(g.div, DEV),
                                 chunk=chunk, validate=False)


def exact_zero(a, n):
    return not a[T(n == 0, DEV)].view(torch.int32).any()


# ------------------------------------------------------------------------------- encode
def planted_rows(V, D, k, rng):
    """Gaussian rows, then: ties straddling columns 255/256 and 511/512, NaN, +-inf, all equal."""
    x = rng.standard_normal((V, D), dtype=np.float32)
    x[0, max(0, min(D, 256) - k):min(D, 256 + k)] = 9.0
    x[1 % V, max(0, min(D, 512) - 3):min(D, 515)] = 7.0
    x[2 % V, ::3] = np.nan
    x[3 % V, 1::5], x[3 % V, 2::5] = np.inf, -np.inf
    x[4 % V] = -1.5
    return x


@pytest.mark.parametrize("V,D,k", ENCODE, ids=[f"V{v}-D{d}-k{k}" for v, d, k in ENCODE])
def test_encode_bit_exact(mk, cuda, V, D, k):
    x = planted_rows(V, D, k, np.random.default_rng(4000 + D))
    val, idx = XR.topk(x, k)
    xt = T(x, cuda)
    dense, v2, i2 = mk.topk_cbsr_dense_x16(xt, k)
    for v, i in (mk.topk_cbsr_x16(xt, k), (v2, i2)):
        assert i.dtype == torch.int16 and M.same_bytes(v, T(val, cuda))
        assert np.array_equal(i.cpu().numpy().astype(np.int64), idx)
    want = torch.zeros(V, D, device=cuda).scatter_(1, T(idx, cuda), T(val, cuda))
    assert M.same_bytes(dense, want)
    if D <= 256:
        v8, i8 = mk.topk_cbsr(xt, k)
        assert M.same_bytes(v8, v2) and torch.equal(i8.long(), i2.long())
    assert mk.topk_error_rows(cuda) == 0


@pytest.mark.parametrize("D", [7, 100, 256, 257, 384, 512, 513, 1023, 1024])
def test_encode_hard_rows(mk, cuda, D):
    """The corpus of tests/topk_rows.py (keys one apart, clusters that need further radix
    passes, +-0, NaN, +-Inf, few distinct values, ties across columns 64 j / 256 / 512 and at
    the last column) through x16_topk_kernel at every k of TR.x16_ks: values, int16 columns and
    the dense row bitwise against x16_ref.topk; up to D = 256 topk_cbsr gives the same bytes;
    one k also from a column slice of a wider tensor (ld_x > D)."""
    x = TR.rows(D, np.random.default_rng(5000 + D))
    xt = T(x, cuda)
    wide = torch.full((len(x), D + 8), 11.0, device=cuda)
    wide[:, 3:3 + D] = xt
    order = XR.topk(x, min(D, 256))[1]  # a prefix of one ranking serves every k
    ks = TR.x16_ks(D)
    mk.topk_error_rows(cuda)
    for k in ks:
        idx = order[:, :k]
        val, it = T(np.take_along_axis(x, idx, 1), cuda), T(idx, cuda)
        want = torch.zeros(len(x), D, device=cuda).scatter_(1, it, val)
        dense, v2, i2 = mk.topk_cbsr_dense_x16(xt, k)
        runs = [mk.topk_cbsr_x16(xt, k), (v2, i2)]
        if k == ks[len(ks) // 2]:
            runs.append(mk.topk_cbsr_x16(wide[:, 3:3 + D], k))
        for v, i in runs:
            assert i.dtype == torch.int16 and M.same_bytes(v, val), (D, k)
            assert torch.equal(i.long(), it), (D, k)
        assert M.same_bytes(dense, want), (D, k)
        if D <= 256:
            v8, i8 = mk.topk_cbsr(xt, k)
            assert M.same_bytes(v8, val) and torch.equal(i8.long(), it), (D, k)
    assert mk.topk_error_rows(cuda) == 0


@pytest.mark.parametrize("V,D,k", [(131, 384, 10), (67, 1024, 256)])
def test_topk_backward(mk, cuda, V, D, k):
    rng = np.random.default_rng(4050 + D)
    idx = XR.topk(rng.standard_normal((V, D), dtype=np.float32), k)[1]
    gv, gd = (T(rng.standard_normal(s, dtype=np.float32), cuda) for s in ((V, k), (V, D)))
    it = T(idx, cuda)
    for a, b in ((gv, None), (None, gd), (gv, gd)):
        src = (0 if a is None else a) + (0 if b is None else b.gather(1, it))
        want = torch.zeros(V, D, device=cuda).scatter_(1, it, src)
        assert M.same_bytes(mk.topk_backward_x16(a, b, i16(idx), D), want)


# ------------------------------------------------------------------------------- aggregation
@pytest.mark.parametrize("D,k", SHAPES, ids=IDS)
@pytest.mark.parametrize("name", GRAPHS)
def test_forward_within_bound(mk, cuda, name, D, k):
    """At the auto item size and at 64 tokens (both hub rows cut into slabs)."""
    for regime in ("unit", "mixed"):
        c = case(name, D, k, regime)
        for chunk in (0, 64):
            out = run_fwd(mk, c, chunk)
            r = N.within(out, c["fwd"], c["fb"][0], f"fwd {name} D{D} k{k} {regime} chunk {chunk}")
            print(f"fwd {name} D{D} k{k} {regime} chunk {chunk}: err/bound {r:.3f}")
            assert exact_zero(out, c["fb"][1])


@pytest.mark.parametrize("D,k", SHAPES, ids=IDS)
@pytest.mark.parametrize("name", GRAPHS)
def test_backward_within_bound(mk, cuda, name, D, k):
    """Both item sizes; a second call gives the same bytes; no in-edges: exactly 0."""
    for regime in ("unit", "mixed"):
        c = case(name, D, k, regime)
        assert (c["bb"][1][c["g"].unread] == 0).all()
        for chunk in (0, 64):
            out = run_bwd(mk, c, chunk)
            r = N.within(out, c["bwd"], c["bb"][0], f"bwd {name} D{D} k{k} {regime} chunk {chunk}")
            print(f"bwd {name} D{D} k{k} {regime} chunk {chunk}: err/bound {r:.3f}")
            assert exact_zero(out, c["bb"][1]) and M.same_bytes(out, run_bwd(mk, c, chunk))


def test_empty_graph(mk, cuda):
    rp = torch.zeros(41, dtype=torch.int32, device=cuda)
    col, ev = torch.empty(0, dtype=torch.int32, device=cuda), torch.empty(0, device=cuda)
    cv, ci = torch.randn(17, 8, device=cuda), torch.zeros(17, 8, dtype=torch.int16, device=cuda)
    out = mk.spgemm_forward_x16(rp, col, ev, cv, ci, 384)
    assert tuple(out.shape) == (40, 384) and not out.view(torch.int32).any()
    g = mk.sspmm_backward_x16(rp, col, ev, torch.randn(40, 384, device=cuda), ci)
    assert tuple(g.shape) == (17, 8) and not g.view(torch.int32).any()


def test_marker_collision(mk, cuda):
    """Every CBSR row selects the pairs (s, s + 256), s = 0..3; row 0 also repeats a selector
    and names column D.  Both columns of a pair receive their own sums: a record that marks a
    trash slot with bit 0x100 of the selector sends s + 256 to trash."""
    D, k = 384, 8
    base = case("S", D, k, "unit")
    g = base["g"]
    ci = np.tile(np.array([0, 256, 1, 257, 2, 258, 3, 259]), (g.C, 1))
    ci[0] = [0, 256, 1, 257, 2, 258, 256, D]
    c = dict(base, ci=ci)
    fb, bb = XR.bound_fwd(g, c["cv"], ci, D), XR.bound_bwd(g, c["G"], ci)
    assert (fb[1][:, 256:260] > 0).any() and (bb[1][0, 7] == 0)
    for chunk in (0, 64):
        N.within(run_fwd(mk, c, chunk), XR.fwd(g, c["cv"], ci, D), fb[0], f"marker fwd {chunk}")
        got = run_bwd(mk, c, chunk)
        N.within(got, XR.bwd(g, c["G"], ci), bb[0], f"marker bwd {chunk}")
        assert exact_zero(got, bb[1])


@pytest.mark.parametrize("name,D,k", [("S", 384, 16), ("S", 1024, 256), ("R", 257, 3)],
                         ids=["S-D384-k16", "S-D1024-k256", "R-D257-k3"])
def test_non_finite(mk, cuda, name, D, k):
    """numerics.poison's Inf / NaN plan (it works unchanged on selectors above 256 columns)
    through x16_pack_kernel's folding, x16_fwd_kernel and x16_bwd_kernel, at both item sizes.
    poison plants its selector >= D only below D = 256, so one more vertex of the hub row gets
    selector D in one slot and 0xffff (-1 as int16) in another, NaN the value of both: neither
    contributes forward, both read exactly 0 backward.  The NaN / +Inf / -Inf masks equal the
    float64 reference's, the finite rest is inside the bound over the finite terms."""
    c = case(name, D, k, "unit")
    g = c["g"]
    cv, ci, G, where = N.poison(g, c["cv"], c["ci"], c["G"], D)
    hubcols = g.col[g.rp[g.hub]:g.rp[g.hub + 1]]
    v = int(next(x for x in hubcols if x not in where["verts"] and x != g.unread))
    ci[v, k - 2], ci[v, k - 1] = D, 0xFFFF
    cv[v, k - 2:] = np.nan
    fwd, (fb, fn) = XR.fwd(g, cv, ci, D), XR.bound_fwd(g, cv, ci, D)
    bwd, (bb, bn) = XR.bwd(g, G, ci), XR.bound_bwd(g, G, ci)
    print(f"non-finite share: fwd {N.reference_is_meaningful(fwd):.3%}, "
          f"bwd {N.reference_is_meaningful(bwd):.3%}")
    assert np.isfinite(fb).all() and np.isfinite(bb).all()
    assert (bwd[v, k - 2:] == 0).all() and (bn[v, k - 2:] == 0).all()
    for chunk in (0, 64):
        out = run_fwd(mk, c, chunk, cv=cv, ci=ci)
        N.within(out, fwd, fb, f"non-finite fwd {name} D{D} k{k} chunk {chunk}")
        assert exact_zero(out, fn)
        got = run_bwd(mk, c, chunk, G=G, ci=ci)
        N.within(got, bwd, bb, f"non-finite bwd {name} D{D} k{k} chunk {chunk}")
        assert exact_zero(got, bn)


# ------------------------------------------------------------------------------- memory
def test_memory_contract(mk, cuda):
    """Outputs and workspaces from the poisoned, guarded arena: guards intact, every output
    element written (the same bytes in every fill regime), inputs unchanged."""
    arena = M.Arena(48 << 20, cuda)
    c = case("S", 384, 16, "unit")
    g = c["g"]

    def factory(primer):
        rp, col = T(g.rp, DEV), T(g.col, DEV)
        ops = [T(x, DEV) for x in (g.ev, c["cv"], c["G"], g.div)]
        if primer:
            ops[1], ops[2] = torch.rand_like(ops[1]), torch.rand_like(ops[2])
        return rp, col, mk.transpose_plan(col, g.C, cache=False), i16(c["ci"]), ops

    def op(rp, col, plan, ci, ops):
        ev, cv, G, div = ops
        return (mk.spgemm_forward_x16(rp, col, ev, cv, ci, 384, row_div=div, validate=False),
                mk.sspmm_backward_x16(rp, col, ev, G, ci, row_div=div, validate=False, plan=plan))

    res = M.run_regimes(op, factory, arena)
    size = [getattr(mk._lib(), f"maxk_{n}_x16_workspace_size")(g.R, g.C, g.col.size, 384, 16, 0)
            for n in ("spgemm_forward", "sspmm_backward")]
    assert sorted(x.nbytes for x in arena.allocs) == sorted([4 * g.R * 384, 4 * g.C * 16] + size)
    for regime in ("stale", "ones"):
        for x, y in zip(res["zero"], res[regime]):
            assert M.same_bytes(x, y), regime
    N.within(res["ones"][0], c["fwd"], c["fb"][0], "memguard fwd")
    N.within(res["ones"][1], c["bwd"], c["bb"][0], "memguard bwd")


# ------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("shape", ["v4", "v1"])
def test_autograd(mk, cuda, shape):
    """maxk_spgemm v4 with int16 selectors and v1 at D = 384: out and the input's gradient
    against the float64 reference; an edge-weight gradient raises."""
    import maxk_spgemm_function as MF
    D, k = 384, 16
    c = case("S", D, k, "unit")
    g = c["g"]
    rp, col = dev_graph("S")
    ev, div, G = T(g.ev, cuda), T(g.div, cuda), T(c["G"], cuda)
    if shape == "v4":
        a3 = T(c["cv"], cuda).requires_grad_(True)
        out = MF.maxk_spgemm(col, ev, a3, i16(c["ci"]), None, 0, rp, div, dim_origin=D)
        cv, ci, bad = c["cv"], c["ci"], (a3.detach(), i16(c["ci"]), None, 0, rp, div, D)
    else:
        x = N.values(np.random.default_rng(4200), (g.C, D), "unit")
        cv, ci = XR.topk(x, k)
        a3 = T(x, cuda).requires_grad_(True)
        out = MF.maxk_spgemm(col, ev, a3, k, graph_indptr=rp, in_degrees=div)
        bad = (a3.detach(), k, None, 0, rp, div)
    out.backward(G)
    N.within(out, XR.fwd(g, cv, ci, D), XR.bound_fwd(g, cv, ci, D)[0], f"{shape} out")
    gs, gb = XR.bwd(g, c["G"], ci), XR.bound_bwd(g, c["G"], ci)[0]
    if shape == "v1":  # the CBSR gradient scattered to the input's columns
        gs, gb = XR.scatter(gs, ci, D), XR.scatter(gb, ci, D)
    N.within(a3.grad, gs, gb, f"{shape} grad")
    with pytest.raises(RuntimeError, match="edge-weight gradient is not available on the x16"):
        MF.maxk_spgemm(col, ev.clone().requires_grad_(True), *bad)


def test_sage_step_matches_dense(cuda):
    """One optimisation step's loss and parameter gradients of MaxKSAGE(hid_size=384, k=32) at
    V = 300 against the same model on dense float64 torch ops (index_add_ aggregation of the
    masked dense features under the mask the model selected).  rtol = atol = 1e-4, the
    tolerance test_layers_gpu.py holds the D <= 256 layers to: a chain of 2 layers of GEMMs
    with K <= 384 and sums of ~12 terms of O(1) values, whose fp32 error is ~1e-6 relative."""
    import maxk_layers as ML
    rng = np.random.default_rng(4300)
    V, F, H, k, n_cls = 300, 48, 384, 32, 5
    deg = rng.poisson(12, V)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = rng.integers(0, V, rp[-1]).astype(np.int32)
    graph = ML.CSRGraph(T(rp, cuda), T(col, cuda))
    torch.manual_seed(43)
    model = ML.MaxKSAGE(F, H, 2, n_cls, maxk=k, feat_drop=0.0).to(cuda)
    x, y = torch.randn(V, F, device=cuda), T(rng.integers(0, n_cls, V), cuda)
    masks = []  # each layer's topk_indices, as the model selected them
    for layer in model.layers:
        layer.register_forward_hook(lambda m, args, out: masks.append(args[3].long()))
    loss = ML.cross_entropy(model(graph, x), y)
    loss.backward()
    P = {n: p.detach().double().requires_grad_(True) for n, p in model.named_parameters()}
    rows = T(np.repeat(np.arange(V), deg), cuda)
    dv = torch.clamp(T(deg, cuda).double(), min=1)[:, None]
    h = x.double() @ P["lin_in.weight"].t() + P["lin_in.bias"]
    for i in range(2):
        assert masks[i].dtype == torch.int64 and tuple(masks[i].shape) == (V, k)
        hs = h * torch.zeros_like(h).scatter_(1, masks[i], 1.0)
        agg = torch.zeros_like(h).index_add_(0, rows, hs[T(col, cuda).long()]) / dv
        h = hs @ P[f"layers.{i}.fc_self.weight"].t() + P[f"layers.{i}.fc_self.bias"] \
            + agg @ P[f"layers.{i}.fc_neigh.weight"].t()
    ref = torch.nn.functional.cross_entropy(h @ P["lin_out.weight"].t() + P["lin_out.bias"], y)
    ref.backward()
    torch.testing.assert_close(loss.double(), ref, rtol=1e-4, atol=1e-4)
    for n, p in model.named_parameters():
        torch.testing.assert_close(p.grad.double(), P[n].grad, rtol=1e-4, atol=1e-4,
                                   msg=lambda m: f"{n}: {m}")
