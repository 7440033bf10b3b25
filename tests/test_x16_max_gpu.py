"""GPU: the max aggregation on 16-bit selectors (x16_max.hip) through the binding
(mk.spgemm_max_forward_x16, mk.spgemm_max_backward_x16), maxk_spgemm_max and the SAGE pool / GIN max
layers at more than 256 columns, against tests/max_aggregate_ref.py: out's bits and arg bitwise,
the backward inside the reference's sum bound, and both held to the u8 kernels at D <= 256.

Graphs: "S" (600 rows, hub rows of 590 and 200 edges, 20 empty rows) and the rectangular "R"
(150 x 700) of numerics.named_graph; a forced item of 64 tokens cuts the hub row into ten."""
import functools

import numpy as np
import pytest
import torch

import max_aggregate_ref as MR
import memguard as M
import numerics as N
import test_gat_attention_gpu as GA
import x16_ref as XR
from test_max_aggregate_gpu import check_backward, check_forward, dense_amax, same_out
from test_parity_gpu import T
from test_x16_gpu import i16, mk  # noqa: F401  (mk: the module fixture)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# a column past the u8 range; the 16-B path; D % 4 != 0; a whole wave with idle lanes; a lane
# walking two slots; the widest
SHAPES = [(257, 3), (384, 16), (513, 33), (1024, 96), (1024, 256)]
IDS = [f"D{D}-k{k}" for D, k in SHAPES]

the_graph, dev_graph = GA.the_graph, GA.dev_graph


def make_case(name, D, k, ci=None, cv=None, seed=0):
    """Distinct selectors; values half Gaussian, half quantised to {-1, -0.0, +0.0, 1} (ties
    across edges, zeros of both signs); the reference's out and arg."""
    g = the_graph(name)
    rng = np.random.default_rng(5100 + 7 * D + k + seed)
    if ci is None:
        ci = XR.topk(rng.standard_normal((g.C, D), dtype=np.float32), k)[1]
    if cv is None:
        cv = N.values(rng, (g.C, k), "unit")
        q = rng.random(cv.shape) < 0.5
        cv[q] = np.rint(np.clip(cv[q], -1, 1))
    out, arg = MR.forward(g.rp, g.col, cv, ci, D)
    return dict(g=g, name=name, D=D, k=k, ci=ci, cv=cv, out=out, arg=arg)


case = functools.lru_cache(maxsize=None)(make_case)  # shared cases: computed once, never modified


def fwd(mk, c, chunk=0, **kw):
    rp, col = dev_graph(c["name"])
    return mk.spgemm_max_forward_x16(rp, col, T(c["cv"], DEV), i16(c["ci"]), c["D"], chunk=chunk,
                                     validate=False, **kw)


def bwd(mk, c, arg, G, chunk=0):
    rp, col = dev_graph(c["name"])
    return mk.spgemm_max_backward_x16(rp, col, i16(c["ci"]), arg, T(G, DEV), c["k"], chunk=chunk)


def grad_case(c, seed, grid=False):
    """grad_out with NaN wherever the implicit zero or nothing won (it must reach nothing) and at
    five winners (it reaches that winner's slots alone); the float64 reference and its bound.
    grid: values on a 2^-6 grid, whose fp32 sums are exact in any order."""
    g = c["g"]
    rng = np.random.default_rng(seed)
    G = N.values(rng, (g.R, c["D"]), "unit")
    if grid:
        G = (np.rint(G * 64) / 64).astype(np.float32)
    G[c["arg"] < 0] = np.nan
    won = np.argwhere(c["arg"] >= 0)
    for i in rng.choice(len(won), 5, replace=False):
        G[tuple(won[i])] = np.nan
    return G, MR.backward(g.rp, g.col, c["ci"], c["arg"], G)


# ------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("name,D,k", [("S", D, k) for D, k in SHAPES] + [("R", 384, 16)],
                         ids=IDS + ["R-D384-k16"])
def test_forward_bitwise(mk, cuda, name, D, k):
    c = case(name, D, k)
    assert (c["arg"] < 0).any() and (c["out"] > 0).any()
    for chunk in (0, 64):
        check_forward(c, *fwd(mk, c, chunk), f"{name} D{D} k{k} chunk {chunk}")
    out, arg = fwd(mk, c, 64, want_arg=False)
    assert arg is None and same_out(out, c["out"])


def test_cut_and_workspace_independence(mk, cuda):
    """Items of one token up to one item for the whole graph (200 tokens cut the hub row into
    three), each from allocator blocks filled with 0x00 and with 0xFF: the same bytes."""
    c = case("S", 384, 16)
    g = c["g"]
    for chunk in (1, 7, 64, 200, 10 ** 6):
        n_ws = mk._lib().maxk_spgemm_max_forward_x16_workspace_size(g.R, g.C, g.col.size, 384, 16,
                                                                    chunk)
        for fill in (0x00, 0xFF):
            junk = [torch.full((n,), fill, dtype=torch.uint8, device=cuda) for n in (n_ws, 4096)]
            del junk
            check_forward(c, *fwd(mk, c, chunk), f"chunk {chunk} fill {fill}")


@pytest.mark.parametrize("chunk", [0, 64])
def test_hard_rows(mk, cuda, chunk):
    """Every vertex selects the pairs (s, s + 256) -- a record that marks trash with bit 0x100
    loses s + 256 -- vertex 0 also repeats a selector and names column D.  Values from
    {+-0.0, +-1, +-Inf, NaN, 0.5}; column 3 is negative in every vertex (an explicit negative
    wins) and column 259 negative where kept and not kept by vertex 0 (the implicit zero wins)."""
    D, k = 384, 8
    g = the_graph("S")
    rng = np.random.default_rng(5200)
    ci = np.tile(np.array([0, 256, 1, 257, 2, 258, 3, 259]), (g.C, 1))
    ci[0] = [0, 256, 1, 257, 2, 258, 256, D]
    pool = np.array([0.0, -0.0, 1, -1, np.inf, -np.inf, np.nan, 0.5], np.float32)
    cv = pool[rng.integers(0, pool.size, (g.C, k))]
    cv[:, 6:] = -1 - rng.random((g.C, 2), dtype=np.float32)
    c = make_case("S", D, k, ci=ci, cv=cv)
    out, arg = c["out"], c["arg"]
    reads0 = np.array([(g.col[g.rp[r]:g.rp[r + 1]] == 0).any() for r in range(g.R)])
    assert reads0.any() and (arg[reads0, 259] == -1).all() and (out[~reads0, 259] <= 0).all()
    assert (out[:, 3] < 0).any() and np.isnan(out).any() and np.isposinf(out).any()
    assert (out.view(np.uint32) == 0x80000000).any() and (arg[:, 256:260] >= 0).any()
    check_forward(c, *fwd(mk, c, chunk), f"hard rows chunk {chunk}")


@pytest.mark.parametrize("D,k", [(100, 10), (256, 16)])
def test_same_bytes_as_u8(mk, cuda, D, k):
    """At D <= 256 the x16 entries give the u8 kernels' bytes of out and arg (the restated key
    functions are the originals'), and a backward numerically equal to theirs on a grad_out whose
    sums are exact (the two-phase form adds explicit zeros: the sign of a zero sum may differ)."""
    c = case("S", D, k)
    rp, col = dev_graph("S")
    ci8 = T(c["ci"].astype(np.uint8), DEV)
    G, b = grad_case(c, 5300 + D, grid=True)
    for chunk in (0, 64):
        out, arg = fwd(mk, c, chunk)
        out8, arg8 = mk.spgemm_max_forward(rp, col, T(c["cv"], DEV), ci8, D, chunk=chunk)
        assert M.same_bytes(out, out8) and M.same_bytes(arg, arg8)
        got = bwd(mk, c, arg, G, chunk)
        got8 = mk.spgemm_max_backward(rp, col, ci8, arg8, T(G, DEV), k)
        assert bool(((got == got8) | (got.isnan() & got8.isnan())).all())
        check_backward(c, got, b, f"D{D} k{k} chunk {chunk}")


# ------------------------------------------------------------------------------- backward
@functools.lru_cache(maxsize=None)
def dup_case():
    """A quarter of the vertices repeat a selector; selectors run past D = 384."""
    g = the_graph("S")
    rng = np.random.default_rng(5400)
    ci = XR.topk(rng.standard_normal((g.C, 448), dtype=np.float32), 16)[1]
    dup = rng.choice(g.C, g.C // 4, replace=False)
    ci[dup, 15] = ci[dup, 0]
    assert (ci >= 384).any()
    return make_case("S", 384, 16, ci=ci)


@pytest.mark.parametrize("src", ["ref", "kernel"])
@pytest.mark.parametrize("D,k", SHAPES + [(384, 0)], ids=IDS + ["repeated-and-skipped"])
def test_backward(mk, cuda, D, k, src):
    """grad_cbsr inside the reference's bound from the reference's arg and from the kernel's own;
    exact zeros where nothing is added, NaNs of grad_out at -1 winners reach nothing; two runs
    give the same bytes."""
    c = case("S", D, k) if k else dup_case()
    G, b = grad_case(c, 5500 + D + k)
    assert (b.n == 0).any() and (b.n > 1).any()
    for chunk in (0, 64):
        arg = T(c["arg"], DEV) if src == "ref" else fwd(mk, c, chunk)[1]
        got = bwd(mk, c, arg, G, chunk)
        check_backward(c, got, b, f"backward D{D} k{k} {src} chunk {chunk}")
        assert M.same_bytes(got, bwd(mk, c, arg, G, chunk))


# ------------------------------------------------------------------------------- autograd, layers
def test_autograd(mk, cuda, monkeypatch):
    """maxk_spgemm_max at D = 384 on int16 selectors: out's bits and the gradient of topk_values
    against the reference; under no_grad the kernel is asked for no winners."""
    import maxk_spgemm_function as MF
    c = case("S", 384, 16)
    rp, col = dev_graph("S")
    calls, real = [], mk.spgemm_max_forward_x16
    monkeypatch.setattr(mk, "spgemm_max_forward_x16",
                        lambda *a, **kw: calls.append(kw.get("want_arg")) or real(*a, **kw))
    tv = T(c["cv"], cuda).requires_grad_(True)
    y = MF.maxk_spgemm_max(rp, col, tv, i16(c["ci"]), 384)
    G, b = grad_case(c, 5600)
    y.backward(T(G, cuda))
    assert same_out(y.detach(), c["out"])
    check_backward(c, tv.grad, b, "autograd topk_values.grad")
    with torch.no_grad():
        y2 = MF.maxk_spgemm_max(rp, col, tv, i16(c["ci"]), 384)
    assert calls == [True, False] and M.same_bytes(y2, y.detach())


@pytest.mark.parametrize("layer", ["sage-pool", "gin-max"])
def test_layer_step_matches_dense(cuda, layer):
    """One step of MaxKSAGEConv(384, 384, aggregator_type="pool") and of
    MaxKGINConv(aggregator_type="max") at 384 columns against the dense float64 composition
    (amax over the neighbours of the masked features), in the output and every gradient, at
    rtol = atol = 1e-4: what test_max_aggregate_gpu.py holds the D <= 256 layers to."""
    import maxk_layers as ML
    rng = np.random.default_rng(5700)
    V, D, k = 200, 384, 32
    deg = rng.poisson(8, V)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = rng.integers(0, V, rp[-1]).astype(np.int32)
    graph = ML.CSRGraph(T(rp, cuda), T(col, cuda))
    torch.manual_seed(57)
    xs, vals, idx = ML.maxk(torch.randn(V, D, device=cuda), k)
    x, tv = xs.detach().requires_grad_(True), vals.detach().requires_grad_(True)
    assert idx.dtype == torch.int16
    if layer == "sage-pool":
        conv = ML.MaxKSAGEConv(D, D, aggregator_type="pool").to(cuda)
    else:
        conv = ML.MaxKGINConv(torch.nn.Linear(D, 24), init_eps=0.25, learn_eps=True,
                              aggregator_type="max").to(cuda)
    out = conv(graph, x, tv, idx)
    gout = torch.randn_like(out)
    names = [n for n, _ in conv.named_parameters()]
    ins = [x] if layer == "sage-pool" else [x, tv]
    got = torch.autograd.grad(out, [p for _, p in conv.named_parameters()] + ins, gout)
    Q = {n: p.detach().double().requires_grad_(True) for n, p in conv.named_parameters()}
    x2, tv2 = (t.detach().double().requires_grad_(True) for t in (x, tv))
    if layer == "sage-pool":
        p = x2 @ Q["fc_pool.weight"].t() + Q["fc_pool.bias"]
        pi = ML.maxk(conv.fc_pool(x.detach()), k)[2]
        agg = dense_amax(rp, col, p * torch.zeros_like(p).scatter(1, pi.long(), 1.0))
        ref = x2 @ Q["fc_self.weight"].t() + Q["fc_self.bias"] + agg @ Q["fc_neigh.weight"].t()
        ins2 = [x2]
    else:
        X = torch.zeros(V, D, dtype=torch.float64, device=cuda).scatter(1, idx.long(), tv2)
        h = (1 + Q["eps"]) * x2 + dense_amax(rp, col, X)
        ref = h @ Q["apply_func.weight"].t() + Q["apply_func.bias"]
        ins2 = [x2, tv2]
    want = torch.autograd.grad(ref, [Q[n] for n in names] + ins2, gout.double())
    torch.testing.assert_close(out, ref.float(), rtol=1e-4, atol=1e-4)
    for n, a, b_ in zip(names + ["x", "topk_values"], got, want):
        torch.testing.assert_close(a, b_.float(), rtol=1e-4, atol=1e-4, msg=lambda m: f"{n}: {m}")
