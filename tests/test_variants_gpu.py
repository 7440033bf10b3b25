"""GPU: one small oracle case for every kernel instantiation that a launch site can select and
no other small test launches (tests/variant_cases.py; the map of which test file launches which
instantiation is profiles/r08/variant_reach/, written by tools/variant_reach.py).

Each case's `rule` field is its docstring: the host rule and the file:line it restates.
test_variants_cpu.py checks, without a GPU, that every case's graph still selects the kernels
it names.

Comparison: the per-element bound of tests/numerics.py, (n + 8) * 2^-24 * S_abs, exact zeros
where an element has no addend, and the NaN / +inf / -inf masks (same_class, inside within) --
never the parity tests' absolute 1e-4.  Every case runs N(0,1) ("unit") and mixed-magnitude
values, with row_div and without, on a graph with an empty row, row lengths that are no
multiple of a batch and a hub row that the case's explicit chunk splits over items.  Inf / NaN
inputs (numerics.poison) go through one case per kernel family (variant_cases.POISONED); the
dense route's and the wide tables' families have theirs in test_numerics_gpu.py.

The top-k cases are bit-exact against the oracle's ordering (value descending, ties by
ascending column).
"""
import functools

import numpy as np
import pytest
import torch

import edge_grad_ref as ER
import numerics as N
import oracle as O
import variant_cases as VC
from test_parity_gpu import T

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:backward mode 'bsort'")]

REGIMES = ("unit", "mixed")
GRAPH_CASES = [c.id for c in VC.CASES if c.op != "topk"]
TOPK_CASES = [c.id for c in VC.CASES if c.op == "topk"]


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    return maxk_cuda_kernels


# ------------------------------------------------------------------------------- shared data
@functools.lru_cache(maxsize=None)
def prepared(cid):
    """The case's graph, selectors and addend counts: built once, never modified.  Past 2^24
    columns the oracle runs over the columns the edges read (compacted, `uc`), as in
    test_parity_gpu.py::test_tables_past_2_24_columns."""
    c = VC.BY_ID[cid]
    rp, col = VC.build_csr(c)
    rng = np.random.default_rng(len(cid) + c.k)
    uc = None
    colc, C = col, c.C
    if c.C >= 1 << 24:
        uc = np.unique(col)
        colc, C = np.searchsorted(uc, col).astype(np.int32), uc.size
    g = N.make_graph(rng, rp, colc, C)
    if uc is None:
        g = g._replace(unread=VC.unread_column(c))
    ci = N.selectors(rng, C, c.D, c.k)
    return dict(c=c, g=g, col=col, uc=uc, ci=ci, nf=N.count_fwd(g, ci, c.D),
                nb=N.count_bwd(g, ci, c.D))


def device_side(p, cuda, ci=None, cv=None):
    """Device tensors of the graph and of the CBSR tables the kernels read (past 2^24 columns
    the full-size tables: the rows no edge reads hold selectors 0..k-1 and zero values)."""
    c, g, uc = p["c"], p["g"], p["uc"]
    ci = p["ci"] if ci is None else ci
    d = dict(rp=T(g.rp, cuda), col=T(p["col"], cuda), ev=T(g.ev, cuda), div=T(g.div, cuda))
    if uc is None:
        d["ci"] = T(ci, cuda)
        d["cv"] = None if cv is None else T(cv, cuda)
        return d
    d["ucg"] = torch.from_numpy(uc.astype(np.int64)).to(cuda)
    d["ci"] = torch.arange(c.k, device=cuda, dtype=torch.uint8).repeat(c.C, 1)
    d["ci"][d["ucg"]] = T(ci, cuda)
    if cv is not None:
        d["cv"] = torch.zeros(c.C, c.k, device=cuda)
        d["cv"][d["ucg"]] = T(cv, cuda)
    return d


def read_rows(out, d):
    """Past 2^24 columns: the rows the edges read; every other row exactly zero."""
    if "ucg" not in d:
        return out
    got = out[d["ucg"]].clone()
    out[d["ucg"]] = 0.0
    assert not out.any(), "rows no edge reads are not zero"
    return got


def backward(mk, c, d, G, div, validate=None):
    """The case's backward call (the mode and options its kernels are selected through)."""
    kw = dict(row_div=div, chunk=c.chunk, validate=validate)
    if c.opts.get("esel"):
        kw["edge_sel"] = mk.edge_selectors(d["col"], d["ci"])
    if c.op == "pull":
        plan = None
        if "shift" in c.opts:
            plan = mk.pull_plan(d["rp"], d["col"], d["ev"], c.C, c.k, c.D,
                                slices=c.opts["slices"], shift=c.opts["shift"])
        return mk.sspmm_backward(d["rp"], d["col"], d["ev"], G, d["ci"], mode="pull", plan=plan,
                                 **kw)
    return mk.sspmm_backward(d["rp"], d["col"], d["ev"], G, d["ci"], mode=c.op, **kw)


# ------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("cid", GRAPH_CASES)
def test_variant_against_oracle(mk, cuda, cid):
    p = prepared(cid)
    c, g = p["c"], p["g"]
    rng = np.random.default_rng(c.k * 7 + c.D)
    for regime in REGIMES:
        G = N.values(rng, (c.R, c.D), regime)
        cv = N.values(rng, p["ci"].shape, regime)
        d = device_side(p, cuda, cv=cv if c.op in ("dense", "wide_fwd", "wide_eg") else None)
        Gd = T(G, cuda)
        for use_div in (True, False):
            gg = g if use_div else g._replace(div=None)
            div = d["div"] if use_div else None
            what = f"{cid} {regime} row_div={use_div}: {c.rule}"
            if c.op in ("csc", "bsort", "dense", "pull"):
                gs = read_rows(backward(mk, c, d, Gd, div), d)
                N.within(gs, N.bwd_ref(gg, G, p["ci"]), N.bound_bwd(gg, G, p["ci"], n=p["nb"]),
                         what)
            if c.op in ("dense", "wide_fwd"):
                y = mk.spgemm_forward(d["rp"], d["col"], d["ev"], d["cv"], d["ci"], c.D,
                                      row_div=div, chunk=c.chunk)
                N.within(y, N.fwd_ref(gg, cv, p["ci"], c.D),
                         N.bound_fwd(gg, cv, p["ci"], c.D, n=p["nf"]), what)
            if c.op == "wide_eg":
                y = mk.edge_weight_grad(d["rp"], d["col"], d["cv"], d["ci"], Gd, row_div=div,
                                        chunk=c.chunk)
                er = ER.edge_grad_ref(g.rp, g.col, cv, p["ci"], G, gg.div)
                N.within(y, ER.as_f32(er.ref), ER.bound(er), what)
        del d
    if c.C >= 1 << 24:
        torch.cuda.empty_cache()


@pytest.mark.parametrize("cid", VC.POISONED)
def test_variant_inf_nan(mk, cuda, cid):
    """+inf, -inf and NaNs in grad_output and repeated selectors (numerics.poison) through the
    family's deepest new variant: the class masks equal the oracle's, the finite rest stays
    inside the bound."""
    p = prepared(cid)
    c, g = p["c"], p["g"]
    rng = np.random.default_rng(c.k + 99)
    G = N.values(rng, (c.R, c.D), "unit")
    cv = N.values(rng, p["ci"].shape, "unit")
    _, cip, Gp, _ = N.poison(g, cv, p["ci"], G, c.D)
    go = N.bwd_ref(g, Gp, cip)
    N.reference_is_meaningful(go)
    d = device_side(p, cuda, ci=cip)
    gs = backward(mk, c, d, T(Gp, cuda), d["div"], validate=False)
    N.within(gs, go, N.bound_bwd(g, Gp, cip), f"{cid} poisoned: {c.rule}")


@pytest.mark.parametrize("cid", TOPK_CASES)
def test_topk_variant_bit_exact(mk, cuda, cid):
    c = VC.BY_ID[cid]
    rng = np.random.default_rng(c.k + c.D)
    if c.opts["dtype"] == "u8":
        x = rng.integers(0, 256, (c.R, c.D)).astype(np.uint8)  # many ties at the threshold
        x[3] = 7  # an all-equal row
        order = np.lexsort((np.tile(np.arange(c.D), (c.R, 1)), -x.astype(np.int32)), axis=1)
        order = order[:, :c.k]
        vo, io = np.take_along_axis(x, order, 1), order.astype(np.uint8)
    else:
        x = rng.standard_normal((c.R, c.D)).astype(np.float32)
        x[::2] = np.round(x[::2] * 4) / 4  # ties
        x[3] = 1.5
        vo, io = O.topk(x, c.k)
    v, i = mk.topk_cbsr(T(x, cuda), c.k)
    assert np.array_equal(i.cpu().numpy(), io), c.rule
    assert np.array_equal(v.cpu().numpy(), vo), c.rule
