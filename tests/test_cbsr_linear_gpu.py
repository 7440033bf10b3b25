"""GPU: the linear layer on CBSR features (cbsr_linear.hip) through mk.cbsr_linear_forward,
mk.cbsr_linear_backward_values, mk.cbsr_linear_backward_weight, the autograd function
maxk_cbsr_linear and MaxKSAGEConv(sparse_self=True), against tests/cbsr_linear_ref.py inside
tests/numerics.py's bound |hip - ref| <= (n + 8) * 2^-24 * S_abs, n the element's own term
count; an element with n = 0 is exactly 0.

Shapes: k = D, k % 4 != 0, O across a tile edge (129, 300), O = 1, a 64-column tile (47) and two
tiles (256, 300: the value gradient's tile sum); chunk_rows 16 cuts every V > 16 into several
items, so the weight gradient sums several partial tiles.  Planted: a repeated selector (row 0,
and every row that selected the unselected column), selectors >= D in slot 0 of every fifth row
where D < 256 and k > 1 (no row loses all its slots), a weight column no row selects.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import cbsr_linear_ref as R
import memguard as M
import numerics as N

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHAPES = [(1, 5, 1, 1), (67, 100, 10, 47), (130, 256, 32, 256), (257, 256, 64, 129),
          (300, 64, 64, 300), (513, 256, 3, 128)]
CHUNKS = (0, 16)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


@functools.lru_cache(maxsize=None)
def case(V, D, k, O, poison=False):
    """Inputs, fp64 references and bounds of one shape, built once."""
    rng = np.random.default_rng(V * 1000 + O)
    idx = N.selectors(rng, V, D, k).astype(np.uint8)
    unsel = 2 % D
    idx[idx == unsel] = (unsel + 1) % D      # no row selects `unsel`; its readers now repeat
    if k > 1:
        idx[0, -1] = idx[0, 0]
    if D < 256 and k > 1:  # rows 1, 6, ...: row 0 keeps its repeat, no row loses every slot
        idx[1::5, 0] = np.minimum(D + rng.integers(0, 9, idx[1::5, 0].shape), 255)
    c = dict(idx=idx, unsel=unsel if D > 1 else None)
    for name, shape in (("val", (V, k)), ("W", (O, D)), ("b", (O,)), ("pre", (V, O)),
                        ("g", (V, O))):
        c[name] = N.values(rng, shape, "unit")
    if poison:
        d0 = int(idx[V // 2, k // 2])
        c["W"][3, d0], c["W"][5, d0], c["val"][7, 2] = np.nan, np.inf, np.nan
    one = lambda a: np.ones_like(a)  # noqa: E731
    fa = N._finite_abs
    for tag, b, pre in (("", None, None), ("b", c["b"], None), ("a", None, c["pre"]),
                        ("ba", c["b"], c["pre"])):
        c["y" + tag] = R.forward(c["val"], idx, c["W"], b, pre)
        n = R.forward(one(c["val"]), idx, one(c["W"]), b if b is None else one(b),
                      pre if pre is None else one(pre))
        s = R.forward(fa(c["val"]), idx, fa(c["W"]), b if b is None else fa(b),
                      pre if pre is None else fa(pre))
        c["by" + tag] = N._bound(n, s, 0.0)
    c["gv"] = R.grad_values(c["g"], idx, c["W"])
    c["bgv"] = N._bound(R.grad_values(one(c["g"]), idx, one(c["W"])),
                        R.grad_values(fa(c["g"]), idx, fa(c["W"])), 0.0)
    c["gw"] = R.grad_weight(c["g"], c["val"], idx, D)
    c["bgw"] = N._bound(R.grad_weight(one(c["g"]), one(c["val"]), idx, D),
                        R.grad_weight(fa(c["g"]), fa(c["val"]), idx, D), 0.0)
    return c


def run_all(mk, c, chunk, what):
    """The three kernels (the forward in its four forms) against the case's references."""
    val, idx, W, g = T(c["val"]), T(c["idx"]), T(c["W"]), T(c["g"])
    for tag in ("", "b", "a", "ba"):
        out = T(c["pre"]).clone() if "a" in tag else None
        y = mk.cbsr_linear_forward(val, idx, W, T(c["b"]) if "b" in tag else None, out=out,
                                   chunk_rows=chunk)
        assert out is None or y is out
        N.within(y, c["y" + tag], c["by" + tag], f"{what} forward {tag!r}")
    gv = mk.cbsr_linear_backward_values(g, idx, W, chunk_rows=chunk)
    N.within(gv, c["gv"], c["bgv"], f"{what} grad_values")
    assert not gv[T(c["idx"] >= W.shape[1])].any()
    gw = mk.cbsr_linear_backward_weight(g, val, idx, W.shape[1], chunk_rows=chunk)
    N.within(gw, c["gw"], c["bgw"], f"{what} grad_weight")
    if c["unsel"] is not None:
        assert not gw[:, c["unsel"]].any() and not c["bgw"][:, c["unsel"]].any()
    return y, gv, gw


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_parity(mk, shape, chunk):
    c = case(*shape)
    first = run_all(mk, c, chunk, f"{shape} chunk {chunk}")
    again = run_all(mk, c, chunk, f"{shape} chunk {chunk}")
    for a, b in zip(first, again):  # bitwise repeatable
        assert M.same_bytes(a, b)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_non_finite(mk, chunk):
    """A NaN and an Inf in one weight column, a NaN value: N.within compares the NaN / Inf masks
    of all three outputs with the restatement's before it bounds the finite rest."""
    c = case(67, 100, 10, 47, poison=True)
    assert np.isnan(c["y"]).any() and np.isnan(c["gv"]).any() and np.isnan(c["gw"]).any()
    assert np.isfinite(c["y"]).any() and np.isfinite(c["gw"][:, c["unsel"]]).all()
    run_all(mk, c, chunk, "poisoned")


def test_empty_and_refused(mk):
    e = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    W, idx0 = T(case(67, 100, 10, 47)["W"]), e(0, 10, dt=torch.uint8)
    assert mk.cbsr_linear_forward(e(0, 10), idx0, W, e(47)).shape == (0, 47)
    assert mk.cbsr_linear_backward_values(e(0, 47), idx0, W).shape == (0, 10)
    gw = mk.cbsr_linear_backward_weight(e(0, 47), e(0, 10), idx0, 100)
    assert gw.shape == (47, 100) and not gw.any()
    idx = e(4, 8, dt=torch.uint8)
    for w, msg in ((e(3, 300), "dim_origin must be in"), (e(3, 5), "dim_k must be in"),
                   (e(0, 16), "out_feats must be in")):
        with pytest.raises(RuntimeError, match=msg):
            mk.cbsr_linear_forward(e(4, 8), idx, w)
        with pytest.raises(RuntimeError, match=msg):
            mk.cbsr_linear_backward_values(e(4, w.shape[0]), idx, w)
        with pytest.raises(RuntimeError, match=msg):
            mk.cbsr_linear_backward_weight(e(4, w.shape[0]), e(4, 8), idx, w.shape[1])


def test_memory_contract(mk, cuda):
    """Outputs and workspaces poisoned and guarded (tests/memguard.py): nothing is stored next to
    them, no input changes, and the results do not depend on what the memory held."""
    shape = (257, 256, 64, 129)
    c, arena = case(*shape), M.Arena(24 << 20, cuda)

    def factory(primer):
        rng = np.random.default_rng(5)
        s = {n: N.values(rng, c[n].shape, "unit") for n in ("val", "W", "g")} if primer else c
        return tuple(T(a) for a in (s["val"], c["idx"], s["W"], s["g"], c["b"]))

    def op(val, idx, W, g, b):
        return (mk.cbsr_linear_forward(val, idx, W, b, chunk_rows=16),
                mk.cbsr_linear_backward_values(g, idx, W, chunk_rows=16),
                mk.cbsr_linear_backward_weight(g, val, idx, 256, chunk_rows=16))
    res = M.run_regimes(op, factory, arena)
    for regime, (y, gv, gw) in res.items():
        N.within(y, c["yb"], c["byb"], regime)
        N.within(gv, c["gv"], c["bgv"], regime)
        N.within(gw, c["gw"], c["bgw"], regime)
        assert all(M.same_bytes(a, b) for a, b in zip(res["zero"], (y, gv, gw))), regime


@pytest.mark.parametrize("drop", [0.0, 0.5])
def test_sage_wiring(mk, drop, monkeypatch):
    """MaxKSAGEConv(sparse_self=True) is, bitwise, linear(agg, fc_neigh) with maxk_cbsr_linear
    accumulated onto it; sparse_self=False is the dense pair of products as before."""
    import maxk_layers as ML
    from test_parity_gpu import rand_graph
    V, D, k, O = 130, 64, 8, 48
    rp, col = rand_graph(np.random.default_rng(3), V, 6)
    graph = ML.CSRGraph(T(rp.astype(np.int32)), T(col.astype(np.int32)))
    torch.manual_seed(1)
    layers = [ML.MaxKSAGEConv(D, O, feat_drop=drop, sparse_self=s).to(DEV) for s in (True, False)]
    x0, gout = torch.randn(V, D, device=DEV), torch.randn(V, O, device=DEV)

    def run(layer, how):
        layer, x = copy.deepcopy(layer), x0.clone().requires_grad_(True)
        torch.manual_seed(7)
        xs, tv, ti = ML.maxk(x, k)
        if how == "layer":
            y = layer(graph, xs, tv, ti)
        else:
            h, tv = ML._dropped_values(xs, tv, ti, layer.feat_drop)
            agg = graph.aggregate(tv, ti, D, row_div=graph.clamped("in_degrees"))
            y = (ML.maxk_cbsr_linear(tv, ti, layer.fc_self.weight, layer.fc_self.bias,
                                     out=ML.linear(agg, layer.fc_neigh)) if how == "sparse"
                 else ML.linear(h, layer.fc_self, agg, layer.fc_neigh))
        y.backward(gout)
        return [y, x.grad, layer.fc_self.weight.grad, layer.fc_self.bias.grad,
                layer.fc_neigh.weight.grad]
    for layer, how in zip(layers, ("sparse", "dense")):
        for a, b in zip(run(layer, "layer"), run(layer, how)):
            assert M.same_bytes(a, b), how
    if drop == 0.0:
        # the autograd function against the dense layer, element by element inside twice the
        # numerics bound (either side is a rounded fp32 sum of the same n terms), S_abs from the
        # same products on absolute values in fp64; the neighbour path is shared by both
        la, f64 = layers[1], lambda t: t.detach().double().abs()  # noqa: E731
        sp = copy.deepcopy(la)  # the same weights, the other path
        sp.sparse_self = True
        (ys, gxs, gws, gbs, gns), (yd, gxd, gwd, gbd, gnd) = run(sp, "layer"), run(la, "layer")
        with torch.no_grad():
            xs, tv, ti = ML.maxk(x0, k)
            agg = graph.aggregate(tv, ti, D, row_div=graph.clamped("in_degrees"))
        g, ws, wn = f64(gout), f64(la.fc_self.weight), f64(la.fc_neigh.weight)
        gself = g @ ws
        for a, b, n, s_abs in (
                (ys, yd, 2 * D + 1, f64(xs) @ ws.t() + f64(agg) @ wn.t() + f64(la.fc_self.bias)),
                (gws, gwd, V, g.t() @ f64(xs)), (gbs, gbd, V, g.sum(0)),
                (gns, gnd, V, g.t() @ f64(agg)),
                (gxs, gxd, O + 2, 2 * gself + f64(gxd))):  # |neighbour part| <= |sum| + |self|
            assert ((a.double() - b.double()).abs() <= 2 * (n + N.EXTRA) * N.EPS * s_abs).all()
    assert list(layers[0].state_dict()) == list(layers[1].state_dict())
    with pytest.raises(ValueError, match="reference_compat"):
        ML.MaxKSAGEConv(D, O, reference_compat=True, sparse_self=True)
    monkeypatch.setenv("MAXK_CBSR_LINEAR", "1")  # overrides the argument, not reference_compat
    assert layers[1].sparse_self_on()
    assert not ML.MaxKSAGEConv(D, O, reference_compat=True).sparse_self_on()
