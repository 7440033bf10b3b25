"""GPU: the fused linear + MaxK (linear_maxk.hip) through mk.linear_maxk_forward, the autograd
function maxk_linear and MaxKGCN(fused_linear_maxk=True), against tests/linear_maxk_ref.py.

Shapes (V, I, D, k): the degenerate case; a K tail below one MFMA step with a D tail and V below
a tile; k = D; two-plus tiles at full width; the rows4 limit with I % 4 != 0 (scalar loads); the
wave-per-row selection (k > 48) at D = 256 and at an odd D; several tiles at a narrow D.
"""
import functools

import numpy as np
import pytest
import torch

import linear_maxk_ref as R
import memguard as M
import numerics as N
import topk_rows as TR
import x16_ref as XR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHAPES = [(1, 1, 1, 1), (5, 3, 100, 10), (67, 100, 100, 100), (130, 256, 256, 32),
          (257, 602, 256, 48), (129, 64, 256, 49), (70, 130, 255, 64), (513, 256, 64, 8)]
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
ids = lambda s: "x".join(map(str, s))  # noqa: E731


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


@functools.lru_cache(maxsize=None)
def case(V, I, D, k, kind, bias):
    """Inputs and the fp64 reference of one shape, built once.  kind "int": integer-valued x, W
    in [-4, 4] and b in [-8, 8], every partial sum below 602 * 16 + 8 < 2^24, so each summation
    order gives the same fp32 number; "unit": Gaussian."""
    rng = np.random.default_rng(V * 1000 + I + D + k)
    if kind == "int":
        draw = lambda s, m: rng.integers(-m, m + 1, s).astype(np.float32)  # noqa: E731
        x, W, b = draw((V, I), 4), draw((D, I), 4), draw((D,), 8)
    else:
        x, W, b = (N.values(rng, s, "unit") for s in ((V, I), (D, I), (D,)))
    b = b if bias else None
    h = R.hidden(x, W, b)
    vals, idx = R.topk(h, k)
    s_abs = R.hidden(np.abs(x), np.abs(W), None if b is None else np.abs(b))
    B = N._bound(np.full(h.shape, I + 1.0), s_abs, 0.0).max(axis=1, keepdims=True)
    return dict(x=x, W=W, b=b, h=h, vals=vals, idx=idx, B=B)


def run(mk, c, k, x=None):
    return mk.linear_maxk_forward(T(c["x"]) if x is None else x, T(c["W"]),
                                  None if c["b"] is None else T(c["b"]), k=k)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_exact_on_integers(mk, shape, bias):
    c, (V, I, D, k) = case(*shape, "int", bias), shape
    if V >= 5 and k < D:  # ties across the k-th position: the column-ascending rule decides
        hs = -np.sort(-c["h"], axis=1)
        assert (hs[:, k - 1] == hs[:, k]).any()
    vals, idx = run(mk, c, k)
    assert M.same_bytes(vals, T(c["vals"].astype(np.float32)))
    assert M.same_bytes(idx, T(c["idx"]))
    if shape == (130, 256, 256, 32):  # ld_x > I: a column slice of a wider tensor
        wide = torch.full((V, I + 8), 7.0, device=DEV)
        wide[:, 4:4 + I] = T(c["x"])
        v2, i2 = run(mk, c, k, wide[:, 4:4 + I])
        assert M.same_bytes(v2, vals) and M.same_bytes(i2, idx)
    assert mk.topk_error_rows() == 0


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_gaussian_within_bound(mk, shape, bias):
    """Sorted in descending order, a row's top-k values move by at most the row's largest
    single-entry error B_r = max_d (I + 1 + 8) 2^-24 (|x_r| . |W_d| + |b_d|); no gap between
    the k-th and (k + 1)-th entry is needed."""
    c, (V, I, D, k) = case(*shape, "unit", bias), shape
    vals, idx = (t.cpu().numpy() for t in run(mk, c, k))
    assert (np.abs(vals - c["vals"]) <= c["B"]).all()
    assert (np.abs(vals - np.take_along_axis(c["h"], idx.astype(np.int64), 1)) <= c["B"]).all()
    srt = np.sort(idx.astype(np.int64), axis=1)
    assert (srt < D).all() and (np.diff(srt, axis=1) > 0).all()
    assert mk.topk_error_rows() == 0


@functools.lru_cache(maxsize=None)
def hard_case(D, pad):
    """The finite rows of tests/topk_rows.py as h's rows: W [D, D + pad] is a signed permutation
    scaled by powers of two (W[d, perm[d]] = +-2^e, e in {-1, 0, 1}, the pad columns zero), so
    h[v, d] = +-2^e x[v, perm[d]] is one product plus zeros: exact, the same fp32 number in any
    summation order, and every zero a +0 like the accumulator's.  Rows that a scale takes out of
    fp32 exactly (a subnormal halved, 3e38 doubled) are left out and named."""
    rng = np.random.default_rng(5100 + 2 * D + pad)
    x, names = TR.rows(D, rng, names=True)
    keep = TR.finite_mask(x)
    x = np.concatenate([x, rng.standard_normal((len(x), pad), dtype=np.float32)], axis=1)
    W = np.zeros((D, D + pad), np.float32)
    W[np.arange(D), rng.permutation(D)] = rng.choice([-1.0, 1.0], D) * 2.0 ** rng.integers(-1, 2, D)
    h64 = R.hidden(x[keep], W)
    with np.errstate(over="ignore"):
        h = h64.astype(np.float32)
    exact = (h.astype(np.float64) == h64).all(axis=1)
    skipped = sorted({n.split("/")[0] for n, e in zip(np.array(names)[keep], exact) if not e})
    h = h[exact] + np.float32(0)  # -0 + 0 = +0
    assert len(h) >= 30 and not np.signbit(h[h == 0]).any()
    return dict(x=x[keep][exact], W=W, b=None, h=h, order=XR.topk(h, D)[1], skipped=skipped)


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("D", [7, 64, 100, 128, 255, 256])
def test_hard_rows(mk, D, pad):
    """topk_select.h's copy of the row selection on the corpus the encode's other copies see:
    values and uint8 columns bitwise against x16_ref.topk at every k of TR.fused_ks; pad = 5
    adds the K tail (and the scalar loads where I % 4 != 0)."""
    c = hard_case(D, pad)
    print(f"D {D} I {D + pad}: {len(c['h'])} rows, left out {c['skipped']}")
    assert set(c["skipped"]) <= {"steps_subnormal", "huge3e38"}
    x, W = T(c["x"]), T(c["W"])
    mk.topk_error_rows()
    for k in TR.fused_ks(D):
        idx = c["order"][:, :k]
        vals, got = mk.linear_maxk_forward(x, W, None, k=k)
        assert M.same_bytes(vals, T(np.take_along_axis(c["h"], idx, 1))), (D, pad, k)
        assert M.same_bytes(got, T(idx.astype(np.uint8))), (D, pad, k)
    assert mk.topk_error_rows() == 0


def test_position_independence(mk):
    shape = (130, 256, 256, 32)
    c, perm = case(*shape, "unit", True), np.random.default_rng(9).permutation(shape[0])
    v0, i0 = run(mk, c, 32)
    v1, i1 = run(mk, c, 32)
    assert M.same_bytes(v0, v1) and M.same_bytes(i0, i1)
    vp, ip = run(mk, c, 32, T(c["x"][perm]))
    assert M.same_bytes(vp, v0[T(perm)]) and M.same_bytes(ip, i0[T(perm)])


def test_non_finite(mk):
    V, I, D, k = 67, 100, 100, 100
    c = case(V, I, D, k, "unit", True)
    x, W = c["x"].copy(), c["W"].copy()
    x[11, 37], W[5, 60] = np.nan, np.inf
    h = R.hidden(x, W, c["b"])
    ref_vals, ref_idx = R.topk(h, k)
    vals, idx = mk.linear_maxk_forward(T(x), T(W), T(c["b"]), k=k)
    vals, idx = vals.cpu().numpy(), idx.cpu().numpy()
    assert np.isnan(vals[11]).all() and (idx[11] == np.arange(k)).all()
    assert np.isposinf(ref_vals).any() and np.isneginf(ref_vals).any()
    N.same_class(vals, ref_vals.astype(np.float32))
    assert (idx[np.isinf(vals)] == 5).all()
    assert mk.topk_error_rows() == 0


def test_memory_contract(mk, cuda):
    """Outputs poisoned and guarded (tests/memguard.py); V = 0 launches nothing."""
    shape = (257, 602, 256, 48)
    c, arena = case(*shape, "int", True), M.Arena(8 << 20, cuda)

    def factory(primer):
        s = case(257, 602, 256, 48, "unit", True) if primer else c
        return tuple(T(s[n]) for n in ("x", "W", "b"))
    res = M.run_regimes(lambda x, W, b: mk.linear_maxk_forward(x, W, b, k=48), factory, arena)
    for regime, (vals, idx) in res.items():
        assert M.same_bytes(vals, T(c["vals"].astype(np.float32))), regime
        assert M.same_bytes(idx, T(c["idx"])), regime
    vals, idx = mk.linear_maxk_forward(torch.empty(0, 602, device=DEV), T(c["W"]), k=48)
    assert vals.shape == idx.shape == (0, 48) and idx.dtype == torch.uint8


def test_refused(mk):
    e = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    for x, w, k, msg in ((e(4, 8), e(257, 8), 4, "D <= 256"), (e(4, 8), e(16, 8), 0, "k = 0"),
                         (e(4, 8), e(16, 8), 17, "k = 17"),
                         (e(4, 8, dt=torch.float16), e(16, 8), 4, "float32")):
        with pytest.raises(RuntimeError, match=msg):
            mk.linear_maxk_forward(x, w, k=k)


def test_autograd(mk):
    """maxk_linear against fp64 torch: the dense linear, then a gather at the kernel's own idx,
    so the comparison does not hinge on the selection."""
    import maxk_layers as ML
    V, I, D, k = 67, 100, 100, 10
    c = case(V, I, D, k, "unit", True)
    layer = torch.nn.Linear(I, D).to(DEV)
    with torch.no_grad():
        layer.weight.copy_(T(c["W"]))
        layer.bias.copy_(T(c["b"]))
    x = T(c["x"]).requires_grad_(True)
    g = T(N.values(np.random.default_rng(3), (V, k), "unit"))
    vals, idx = ML.maxk_linear(x, layer, k)
    vals.backward(g)
    x64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (x, layer.weight, layer.bias))
    sel = idx.long()
    ref = (x64 @ w64.t() + b64).gather(1, sel)
    ref.backward(g.double())
    gd = torch.zeros(V, D, dtype=torch.float64, device=DEV).scatter(1, sel, g.double().abs())
    xa, wa = x64.detach().abs(), w64.detach().abs()
    for a, r, n, s_abs in ((vals, ref, I + 1, (xa @ wa.t() + b64.detach().abs()).gather(1, sel)),
                           (x.grad, x64.grad, D, gd @ wa), (layer.weight.grad, w64.grad, V, gd.t() @ xa),
                           (layer.bias.grad, b64.grad, V, gd.sum(0))):
        assert ((a.double() - r).abs() <= (n + N.EXTRA) * N.EPS * s_abs).all()


def test_gcn_layer(mk, monkeypatch):
    """MaxKGCN(fused_linear_maxk=True) in eval mode; lin_in and the first hidden Linear hold
    integers, so the first fused layer equals the two-step one bitwise.  The second layer's h
    differs between the models by two roundings of (I + 1)-term sums; that bound, carried through
    the aggregation and lin_out in fp64 on absolute values, plus the roundings of those two
    products themselves, bounds the logits."""
    import maxk_layers as ML
    from test_parity_gpu import rand_graph
    V, F, H, C, k = 200, 24, 64, 7, 8
    rp, col = rand_graph(np.random.default_rng(3), V, 6)
    graph = ML.CSRGraph(T(rp.astype(np.int32)), T(col.astype(np.int32)))
    torch.manual_seed(1)
    plain = ML.MaxKGCN(F, H, 2, C, maxk=k, feat_drop=0.5).to(DEV).eval()
    with torch.no_grad():
        for p in (*plain.lin_in.parameters(), *plain.linlayers[0].parameters()):
            p.copy_(torch.randint(-2, 3, p.shape, device=DEV).float())
    fused = ML.MaxKGCN(F, H, 2, C, maxk=k, feat_drop=0.5, fused_linear_maxk=True).to(DEV).eval()
    assert list(fused.state_dict()) == list(plain.state_dict())
    fused.load_state_dict(plain.state_dict())
    x = torch.randint(-2, 3, (V, F), device=DEV).float()
    with torch.no_grad():
        h0 = ML.linear(x, plain.lin_in).relu()
        two = mk.topk_cbsr(ML.linear(h0, plain.linlayers[0]), k)
        one = ML.maxk_linear(h0, fused.linlayers[0], k)
        assert all(M.same_bytes(a, b) for a, b in zip(one, two))
        out_f, out_p = fused(graph, x), plain(graph, x)
        h1 = plain.convs[0](graph, None, *two)
        _, vals2, idx2 = ML.maxk(ML.linear(h1, plain.linlayers[1]), k)
        f64 = lambda t: t.double().abs()  # noqa: E731
        lin2, ev = plain.linlayers[1], f64(plain.convs[1]._norm_values(graph))
        A = torch.zeros(V, V, dtype=torch.float64, device=DEV).index_put_(
            (graph.edge_rows().long(), graph.indices.long()), ev, accumulate=True)
        dh = 2 * (H + 1 + N.EXTRA) * N.EPS * (f64(h1) @ f64(lin2.weight).t() + f64(lin2.bias))
        sel = torch.zeros(V, H, dtype=torch.float64, device=DEV)
        agg = A @ (sel.scatter(1, idx2.long(), 1.0) * dh + sel.scatter(1, idx2.long(), f64(vals2))
                   * 2 * (V + N.EXTRA) * N.EPS)
        s_out = (A @ sel.scatter(1, idx2.long(), f64(vals2))) @ f64(plain.lin_out.weight).t() + \
            f64(plain.lin_out.bias)
        bound = agg @ f64(plain.lin_out.weight).t() + 2 * (H + 1 + N.EXTRA) * N.EPS * s_out
    assert ((out_f.double() - out_p.double()).abs() <= bound).all()
    with pytest.raises(ValueError, match="reference_compat"):
        ML.MaxKGCN(F, H, 2, C, reference_compat=True, fused_linear_maxk=True)
    monkeypatch.setenv("MAXK_LINEAR_MAXK", "1")  # overrides the argument, not reference_compat
    assert plain.fused_linear_maxk_on()
    assert not ML.MaxKGCN(F, H, 2, C, reference_compat=True).fused_linear_maxk_on()
