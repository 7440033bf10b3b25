"""GPU: the multi-head 16-bit-selector kernels (x16_heads.hip) through the binding, the autograd
functions and the two attention layers, against float64 numpy built from tests/x16_ref.py: every
element within numerics.py's bound (n + 8) * 2^-24 * sum|terms| of exact, exactly 0 where n = 0.

One rectangular graph, 220 x 310: row 3 is a hub of 200 edges (chunk = 64 cuts it three times),
row 7 is empty, no edge reads column 150, vertex 5 repeats a selector and vertex 6 names column
D; the hub row reads both vertices."""
import functools

import numpy as np
import pytest
import torch

import memguard as M
import numerics as N
import x16_ref as XR
from test_parity_gpu import T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
R, C, UNREAD = 220, 310, 150
CASES = [(7, 7, 3), (260, 10, 2), (508, 16, 3), (512, 32, 8), (384, 33, 2), (1024, 100, 3),
         (1024, 256, 1)]
IDS = [f"D{D}-k{k}-H{H}" for D, k, H in CASES]


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


@functools.lru_cache(maxsize=None)
def graph():
    rng = np.random.default_rng(2800)
    deg = rng.poisson(10, R)
    deg[3], deg[7] = 200, 0
    rp = np.concatenate([[0], np.cumsum(deg)])
    col = rng.integers(0, C, rp[-1])
    col[rp[3]:rp[3] + 2] = (5, 6)
    return N.make_graph(rng, rp, col, C, unread=UNREAD)


def refs(g, w, cv, ci, G, D):
    """The float64 values of the three entries, per head from x16_ref, and their bounds (fb, eb,
    bb): S_abs from the same sums over absolute values, n the addend count -- the feature
    gradient has the addends of every head."""
    H = w.shape[0]
    gh = [g._replace(ev=w[h]) for h in range(H)]
    ga = [g._replace(ev=np.abs(w[h])) for h in range(H)]
    rows = np.repeat(np.arange(g.R), np.diff(g.rp))
    X, Xa, Xn = (XR.scatter(v, ci, D)[g.col] for v in (cv, np.abs(cv), np.ones_like(cv)))
    dv = g.div[rows].astype(np.float64)
    n = XR.bound_bwd(ga[0], G[0], ci)[1]  # one head's count: the same for every head
    return dict(
        fwd=np.stack([XR.fwd(x, cv, ci, D) for x in gh]),
        fb=np.stack([XR.bound_fwd(x, cv, ci, D)[0] for x in ga]),
        edge=np.stack([(X * G[h][rows]).sum(1) / dv for h in range(H)]),
        eb=np.stack([N._bound(Xn.sum(1), (Xa * np.abs(G[h][rows])).sum(1) / dv, 0.0)
                     for h in range(H)]),
        bwd=sum(XR.bwd(x, G[h], ci) for h, x in enumerate(gh)),
        bb=N._bound(H * n, sum(XR.bwd(x, np.abs(G[h]), ci) for h, x in enumerate(ga)), 0.0), n=n)


@functools.lru_cache(maxsize=None)
def case(D, k, H):
    """Inputs, references and bounds of one shape: computed once, never modified."""
    g, rng = graph(), np.random.default_rng(2810 + 7 * D + k)
    ci = XR.topk(rng.standard_normal((C, D), dtype=np.float32), k)[1]
    ci[5, k - 1], ci[6, 0] = ci[5, 0], D
    cv, w = N.values(rng, (C, k), "unit"), N.values(rng, (H, g.col.size), "unit")
    G = N.values(rng, (H, R, D), "unit")
    c = dict(refs(g, w, cv, ci, G, D), g=g, D=D, k=k, H=H, ci=ci, cv=cv, w=w, G=G)
    assert (c["n"][UNREAD] == 0).all() and c["n"][6, 0] == 0 and (c["n"][6, 1:] > 0).any()
    return c


def run(mk, c, chunk, w=None, G=None, plan=None):
    """(out, grad_edge, grad_cbsr) of the three entries on the case's inputs."""
    g = c["g"]
    rp, col, div, ci = T(g.rp, DEV), T(g.col, DEV), T(g.div, DEV), T(c["ci"].astype(np.int16), DEV)
    w, G, cv = (a if torch.is_tensor(a) else T(a, DEV)
                for a in (c["w"] if w is None else w, c["G"] if G is None else G, c["cv"]))
    kw = dict(row_div=div, chunk=chunk, validate=False)
    return (mk.spgemm_forward_heads_x16(rp, col, w, cv, ci, c["D"], **kw),
            mk.edge_weight_grad_heads_x16(rp, col, cv, ci, G, **kw),
            mk.sspmm_backward_heads_x16(rp, col, w, G, ci, plan=plan, **kw))


@pytest.mark.parametrize("chunk", (0, 64))
@pytest.mark.parametrize("D,k,H", CASES, ids=IDS)
def test_oracle(mk, cuda, D, k, H, chunk):
    c = case(D, k, H)
    got = run(mk, c, chunk)
    for a, name, b in zip(got, ("fwd", "edge", "bwd"), ("fb", "eb", "bb")):
        r = N.within(a, c[name], c[b], f"{name} D{D} k{k} H{H} chunk {chunk}")
        print(f"{name} D{D} k{k} H{H} chunk {chunk}: err/bound {r:.3f}")
    assert not got[2][UNREAD].view(torch.int32).any()  # no in-edge: an exactly zero row
    assert got[2][6, 0].view(torch.int32).item() == 0  # the selector >= D
    assert all(M.same_bytes(a, b) for a, b in zip(got, run(mk, c, chunk)))


@pytest.mark.parametrize("chunk", (0, 64))
@pytest.mark.parametrize("D,k,H", CASES, ids=IDS)
def test_head_isolation(mk, cuda, D, k, H, chunk):
    """NaN in every other head's weights (forward) and grad_out (edge gradient) leaves head 0's
    bytes; at H = 1 the backward is sspmm_backward_x16, bit for bit."""
    c = case(D, k, H)
    got = run(mk, c, chunk)
    if H == 1:
        g = c["g"]
        one = mk.sspmm_backward_x16(T(g.rp, DEV), T(g.col, DEV), T(c["w"][0], DEV),
                                    T(c["G"][0], DEV), T(c["ci"].astype(np.int16), DEV),
                                    row_div=T(g.div, DEV), chunk=chunk, validate=False)
        assert M.same_bytes(got[2], one)
        return
    w, G = c["w"].copy(), c["G"].copy()
    w[1:], G[1:] = np.nan, np.nan
    bad = run(mk, c, chunk, w=w, G=G)
    assert M.same_bytes(got[0][0], bad[0][0]) and M.same_bytes(got[1][0], bad[1][0])
    assert torch.isnan(bad[0][1:]).any() and torch.isnan(bad[1][1:]).any()


@pytest.mark.parametrize("fn", ["spgemm_heads", "dot_scores_heads"])
def test_autograd(mk, cuda, fn):
    """maxk_spgemm_heads and maxk_dot_scores_heads with int16 selectors at D = 384: the output
    and both gradients inside the bounds.  The selector D becomes a second repeated one: the
    binding's selector check, where it is switched on, refuses it."""
    import maxk_spgemm_function as MF
    c = case(384, 16, 3)
    g, ci_np = c["g"], c["ci"].copy()
    ci_np[6, 0] = ci_np[6, 1]
    rp, col, ci = T(g.rp, DEV), T(g.col, DEV), T(ci_np.astype(np.int16), DEV)
    tv = T(c["cv"], DEV).requires_grad_(True)
    if fn == "spgemm_heads":
        a = T(c["w"], DEV).requires_grad_(True)
        out = MF.maxk_spgemm_heads(rp, col, a, tv, ci, 384, T(g.div, DEV))
        out.backward(T(c["G"], DEV))
        c = refs(g, c["w"], c["cv"], ci_np, c["G"], 384)
        want = (("fwd", "fb", out), ("edge", "eb", a.grad), ("bwd", "bb", tv.grad))
    else:  # the score is the edge gradient with q for grad_out; its gradients are the other two
        a = T(c["G"], DEV).requires_grad_(True)
        out = MF.maxk_dot_scores_heads(rp, col, a, tv, ci, 1.0)
        out.backward(T(c["w"], DEV))
        c = refs(g._replace(div=np.ones_like(g.div)), c["w"], c["cv"], ci_np, c["G"], 384)
        want = (("edge", "eb", out), ("fwd", "fb", a.grad), ("bwd", "bb", tv.grad))
    for name, b, got in want:
        N.within(got, c[name], c[b], f"{fn} {name}")


@pytest.mark.parametrize("kind", ["gat", "transformer"])
def test_layer_step_matches_dense(cuda, kind):
    """One step of Linear -> MaxK -> layer at in_feats = 384, V = 300, k = 32, three heads: the
    loss and every parameter gradient against the same model in dense float64 torch under the
    mask the model selected, rtol = atol = 1e-4 as tests/test_layers_gpu.py holds the layers to
    (GEMMs of K <= 384 and sums of ~12 O(1) terms: fp32 error ~1e-6 relative)."""
    import maxk_layers as ML
    rng = np.random.default_rng(2850)
    V, F, I, O, H, k = 300, 48, 384, 8, 3, 32
    deg = rng.poisson(12, V)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = T(rng.integers(0, V, rp[-1]).astype(np.int32), cuda)
    graph_ = ML.CSRGraph(T(rp, cuda), col)
    torch.manual_seed(28)
    lin = torch.nn.Linear(F, I).to(cuda)
    make = ML.MaxKMultiHeadGATConv if kind == "gat" else ML.MaxKTransformerConv
    layer = make(I, O, H).to(cuda)
    x, y = torch.randn(V, F, device=cuda), T(rng.integers(0, O, V), cuda)
    xs, tv, ti = ML.maxk(lin(x), k)
    assert ti.dtype == torch.int16
    loss = ML.cross_entropy(layer(graph_, xs, tv, ti).mean(1), y)
    loss.backward()
    with pytest.raises(ValueError, match='attention="stored"'):
        make(I, O, H, attention="fused").to(cuda)(graph_, xs.detach(), tv.detach(), ti)

    P = {pre + n: p.detach().double().requires_grad_(True)
         for m, pre in ((lin, "lin."), (layer, "")) for n, p in m.named_parameters()}
    rows, cl = T(np.repeat(np.arange(V), deg), cuda), col.long()
    h = x.double() @ P["lin.weight"].t() + P["lin.bias"]
    hs = h * torch.zeros_like(h).scatter_(1, ti.long(), 1.0)
    if kind == "gat":
        W = P["fc.weight"].view(H, O, I)
        sd = torch.einsum("vi,hoi,ho->hv", hs, W, P["attn_dst"])
        ss = torch.einsum("vi,hoi,ho->hv", hs, W, P["attn_src"])
        logit = torch.nn.functional.leaky_relu(sd[:, rows] + ss[:, cl], layer.negative_slope)
    else:
        Wq, Wk, W = (P[f"fc_{n}.weight"].view(H, O, I) for n in "qkv")
        q = torch.matmul(torch.matmul(hs, Wq.transpose(1, 2)), Wk)
        logit = layer.scale * (q[:, rows] * hs[cl]).sum(-1)
    p = torch.exp(logit)  # O(1) logits in float64: no shift needed
    alpha = p / torch.zeros(H, V, dtype=p.dtype, device=cuda).index_add_(1, rows, p)[:, rows]
    agg = torch.zeros(H, V, I, dtype=p.dtype, device=cuda).index_add_(
        1, rows, alpha[:, :, None] * hs[cl])
    rst = torch.einsum("hvi,hoi->vho", agg, W) + P["bias"]
    ref = torch.nn.functional.cross_entropy(rst.mean(1), y)
    ref.backward()
    torch.testing.assert_close(loss.double(), ref, rtol=1e-4, atol=1e-4)
    for m, pre in ((lin, "lin."), (layer, "")):
        for n, q_ in m.named_parameters():
            torch.testing.assert_close(q_.grad.double(), P[pre + n].grad, rtol=1e-4, atol=1e-4,
                                       msg=lambda s: f"{pre + n}: {s}")


def test_memory_contract(mk, cuda):
    """(512, 32, 8) at chunk 64 from the poisoned, guarded arena: guards intact, the allocations
    are the outputs and the queried workspaces, the outputs the same bytes in every fill regime."""
    arena = M.Arena(64 << 20, cuda)
    c = case(512, 32, 8)
    g = c["g"]

    def factory(primer):
        col = T(g.col, DEV)
        w, G = T(c["w"], DEV), T(c["G"], DEV)
        if primer:
            w, G = torch.rand_like(w), torch.rand_like(G)
        return w, G, mk.transpose_plan(col, C, cache=False)

    res = M.run_regimes(lambda w, G, plan: run(mk, c, 64, w=w, G=G, plan=plan), factory, arena)
    size = [getattr(mk._lib(), f"maxk_{n}_heads_x16_workspace_size")(R, C, g.col.size, 512, 32, 8,
                                                                     64)
            for n in ("spgemm_forward", "edge_weight_grad", "sspmm_backward")]
    outs = [4 * 8 * R * 512, 4 * 8 * g.col.size, 4 * C * 32]
    assert sorted(x.nbytes for x in arena.allocs) == sorted(outs + size)
    for regime in ("stale", "ones"):
        assert all(M.same_bytes(a, b) for a, b in zip(res["zero"], res[regime])), regime
    for a, name, b in zip(res["ones"], ("fwd", "edge", "bwd"), ("fb", "eb", "bb")):
        N.within(a, c[name], c[b], f"memguard {name}")
