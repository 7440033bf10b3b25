"""GPU numerics: every forward form and backward mode against the fp64 oracle at the values
where kernels go wrong -- magnitudes far from 1, fp32 subnormals, Inf and NaN -- with the
per-element rounding bound and the class masks of tests/numerics.py instead of the parity
tests' absolute 1e-4.

(a) bound      |hip - oracle| <= (n + 8) * 2^-24 * S_abs per element, at N(0,1), 2^-20, 2^40 and
               mixed +-m * 2^e values; elements without addends exactly 0.
(b) scale      f(2^s x) == 2^s f(x) bitwise for s = -20, +40 wherever the sum order is fixed.
(c) Inf / NaN  class masks equal the oracle's, the finite rest inside the bound.
(d) subnormal  inputs at 2^-130 with the floor (n + 8) * 2^-149; nothing resolvable flushed.
(e) autograd   an Inf and a NaN in grad_output reach x.grad where the oracle says.

Forward forms and where the code takes them (csrc/spgemm_fwd.hip, fwd_layout :927-949 and
forward_impl :1045-1097; S is sparse, average degree < kFwdSparseDegree = 128):
  ustep      S, k = 8 and D = 33, k = 5.  D % 4 != 0 never streams (L.stream needs D % 4 == 0), so
             every row of D = 33 goes through EdgeWalker::run / run_rows, the U-step walker over
             packed records (cbsr_pack_kernel: k % 4 != 0).  At k = 8 a sparse graph runs 16 lanes
             per edge (fwd_lanes_per_edge), which the stream rule accepts: its rows of at most 64
             edges stream, the longer ones and the hub slabs take EdgeWalker::run.
  stream     S, k = 16: stream_rows over packed one-line records (6k = 96 <= 128 B).
  stream-rec S, k = 32 and D = 100, k = 28: records past one line, packed as transport records
             (mk.records_ok asserted): stream_rows / walk_src over RecordSrc.
  deep       Dn, k = 16 (packed) and k = 32 (transport records, mk.records_ok asserted): average
             degree >= 128 sets L.deep, the 2U-step EdgeWalker.
  emit       edge_sel_out=: spgemm_fwd_kernel<KG, U, false, true> whatever the graph.
  dense      D = 64, k = 32 and D = 128, k = 64: maxk_dense_route asserted (dense_route.hip).
  records    mk.cbsr_records + mk.spgemm_forward_records.
  rect       R, 150 x 700.

Sum order, for (b): every forward form is bitwise scale-equivariant.  A product is one fma into
the lane group's own LDS copy (spgemm_fwd.hip: EdgeWalker, walk_src and stream_rows; plain
ds_read / ds_write, no LDS atomics: repeated selectors are folded by the pack, cbsr_pack_kernel,
cbsr_pack4_kernel and cbsr_records_kernel), a group meets its edges in CSR order, flush_row
adds the copies in fixed order and slab_fixup_kernel (common.h) adds a hub row's slabs in
item order; the dense route walks rows into registers and uses the same fixup (dense_route.hip,
dense_forward).  A power-of-two scale
commutes with every one of these roundings.  Of the backward modes csc, csc with edge_sel= and
dense are bitwise repeatable (include/maxk_hip.h) and get (b); pull, bsort and hybrid sum
through order-dependent fp64 LDS atomics and atomic through fp32 global atomics: (a) at both
scales.

Largest err / bound seen on an MI355X, over all regimes of (a) and (d) (the fp32 sequential
emulation of test_numerics_cpu.py reaches 0.35 forward, 0.31 backward):

  forward   ustep 0.40   stream 0.36   stream-rec 0.34   deep 0.30   emit 0.36   dense 0.33
            records 0.34   rect 0.30
  backward  auto 0.28   pull 0.20   csc 0.31   csc-sel 0.28   bsort 0.27   hybrid 0.28
            atomic 0.36   dense 0.29

None is above 0.5.  The pull's fp64 LDS sums show in its ratio (one rounding at the end instead
of n; the hybrid's 0.28 comes from its csc part, its pulled tiles alone reach 0.19); the atomic
mode's ratio moves with the order of its atomics (0.31 and 0.36 in two runs), and it kept every
fp32 subnormal.
"""
import functools

import numpy as np
import pytest
import torch

import numerics as N
import oracle as O
from test_parity_gpu import T, rand_graph

pytestmark = pytest.mark.gpu
quiet_bsort = pytest.mark.filterwarnings("ignore:backward mode 'bsort'")  # k > 8: slower, correct

DEV = torch.device("cuda:0")
RATIOS: dict = {}


@pytest.fixture(scope="module")
def mk(cuda):
    import maxk_cuda_kernels
    yield maxk_cuda_kernels
    for fam in sorted(RATIOS):  # the docstring's table (pytest -s shows it)
        print(f"\nnumerics err/bound  {fam:<14s} {RATIOS[fam]:.3f}", end="")
    print()


def note(family, r):
    RATIOS[family] = max(RATIOS.get(family, 0.0), r)


# ------------------------------------------------------------------------------- shared data
@functools.lru_cache(maxsize=None)
def graph(name):
    return N.named_graph(name, rand_graph)


@functools.lru_cache(maxsize=None)
def dgraph(name):
    """The graph's device tensors, made once (the per-graph plans are cached on them)."""
    g = graph(name)
    return tuple(T(a, DEV) for a in (g.rp, g.col, g.ev, g.div))


@functools.lru_cache(maxsize=None)
def sel_and_counts(name, D, k):
    g = graph(name)
    ci = N.selectors(np.random.default_rng(D * 1000 + k), g.C, D, k)
    return ci, N.count_fwd(g, ci, D), N.count_bwd(g, ci, D)


@functools.lru_cache(maxsize=None)
def case(name, D, k, regime):
    """Inputs, oracle results and bounds of one (graph, shape, regime): computed once, shared by
    every form and mode, never modified."""
    g = graph(name)
    ci, nf, nb = sel_and_counts(name, D, k)
    rng = np.random.default_rng(D * 100 + k + 7 * len(regime))
    cv = N.values(rng, (g.C, k), regime)
    G = N.values(rng, (g.R, D), regime)
    pre = N.values(rng, (g.R, D), regime)
    unit = N.floor_unit(regime)
    yo = N.fwd_ref(g, cv, ci, D)
    return dict(g=g, ci=ci, cv=cv, G=G, pre=pre, yo=yo, go=N.bwd_ref(g, G, ci),
                by=N.bound_fwd(g, cv, ci, D, unit=unit, n=nf),
                ya=N.add_prefill(yo, pre),
                bya=N.bound_fwd(g, cv, ci, D, prefill=pre, unit=unit, n=nf),
                bg=N.bound_bwd(g, G, ci, unit=unit, n=nb))


# ------------------------------------------------------------------------------- forward forms
#        id                    family        graph D    k   variant
FWD = [("ustep-k8",            "fwd ustep",   "S",  256, 8,  "plain"),
       ("ustep-D33-k5",        "fwd ustep",   "S",  33,  5,  "plain"),
       ("stream-k16",          "fwd stream",  "S",  256, 16, "plain"),
       ("stream-rec-k32",      "fwd stream-rec", "S", 256, 32, "plain"),
       ("stream-rec-D100-k28", "fwd stream-rec", "S", 100, 28, "plain"),
       ("deep-k16",            "fwd deep",    "Dn", 256, 16, "plain"),
       ("deep-rec-k32",        "fwd deep",    "Dn", 256, 32, "plain"),
       ("emit-k16",            "fwd emit",    "S",  256, 16, "emit"),
       ("dense-D64-k32",       "fwd dense",   "S",  64,  32, "plain"),
       ("dense-D128-k64",      "fwd dense",   "S",  128, 64, "plain"),
       ("records-k32",         "fwd records", "S",  256, 32, "records"),
       ("rect-k32",            "fwd rect",    "R",  256, 32, "plain")]
FWD_IDS = [f[0] for f in FWD]
CHUNKS = (0, 40)  # 40 tokens: the hub rows are split into slabs
TRANSPORT = {"stream-rec-k32", "stream-rec-D100-k28", "deep-rec-k32", "records-k32", "rect-k32"}


def check_form(mk, fid, name, D, k):
    """The case really takes the form its id names, where the library exposes a predicate."""
    g = graph(name)
    E = g.col.size
    dense = bool(mk._lib().maxk_dense_route(D, k))
    assert dense == fid.startswith("dense"), fid
    if fid in TRANSPORT:
        assert mk.records_ok(g.R, g.C, E, D, k), fid
    elif not dense:
        assert not mk.records_ok(g.R, g.C, E, D, k), fid
    assert (E >= 128 * g.R) == (name == "Dn")


def run_fwd(mk, name, variant, cv, ci, D, chunk, out=None, accumulate=False, validate=None,
            gt=None, es_out=None):
    """gt: the graph's device tensors in place of the cached dgraph(name); es_out: the caller's
    buffer for the emit variant's edge selectors."""
    rp, col, ev, div = dgraph(name) if gt is None else gt
    k = ci.shape[1]
    if variant == "records":
        rec = mk.cbsr_records(cv, ci, D)
        return mk.spgemm_forward_records(rp, col, ev, rec, k, D, row_div=div, chunk=chunk,
                                         out=out, accumulate=accumulate, validate=validate)
    es = None
    if variant == "emit":
        es = es_out
        if es is None:
            es = torch.full((col.numel(), k), 0xAB, dtype=torch.uint8, device=DEV)
    y = mk.spgemm_forward(rp, col, ev, cv, ci, D, row_div=div, chunk=chunk, out=out,
                          accumulate=accumulate, validate=validate, edge_sel_out=es)
    if es is not None:
        assert torch.equal(es, ci[col.long()])
    return y


@pytest.mark.parametrize("regime", N.REGIMES)
@pytest.mark.parametrize("fid,family,name,D,k,variant", FWD, ids=FWD_IDS)
def test_forward_bound(mk, cuda, fid, family, name, D, k, variant, regime):
    """(a) and (d): every forward form, whole and with the hub rows in slabs, written and
    accumulated onto a prefill of the regime's own magnitude (one more addend)."""
    check_form(mk, fid, name, D, k)
    c = case(name, D, k, regime)
    cv, ci = T(c["cv"], cuda), T(c["ci"], cuda)
    for chunk in CHUNKS:
        y = run_fwd(mk, name, variant, cv, ci, D, chunk)
        note(family, N.within(y, c["yo"], c["by"], f"{fid} chunk {chunk}"))
        acc = T(c["pre"], cuda)
        run_fwd(mk, name, variant, cv, ci, D, chunk, out=acc, accumulate=True)
        note(family, N.within(acc, c["ya"], c["bya"], f"{fid} chunk {chunk} accumulate"))
        if regime == "subnormal":
            N.nonzero_where_resolved(y, c["yo"], c["by"])


@pytest.mark.parametrize("s", [-20, 40])
@pytest.mark.parametrize("fid,family,name,D,k,variant", FWD, ids=FWD_IDS)
def test_forward_scale_equivariant(mk, cuda, fid, family, name, D, k, variant, s):
    """(b): f(2^s x) == 2^s f(x) bit for bit in every forward form (fixed sum order, see the
    module docstring), the accumulate prefill scaled alike."""
    c = case(name, D, k, "unit")
    ci = T(c["ci"], cuda)
    f = np.float32(2.0 ** s)
    for chunk in CHUNKS:
        y1 = run_fwd(mk, name, variant, T(c["cv"], cuda), ci, D, chunk).cpu().numpy()
        ys = run_fwd(mk, name, variant, T(c["cv"] * f, cuda), ci, D, chunk).cpu().numpy()
        assert np.array_equal(ys, y1 * f), f"{fid} chunk {chunk}"
        a1, as_ = T(c["pre"], cuda), T(c["pre"] * f, cuda)
        run_fwd(mk, name, variant, T(c["cv"], cuda), ci, D, chunk, out=a1, accumulate=True)
        run_fwd(mk, name, variant, T(c["cv"] * f, cuda), ci, D, chunk, out=as_, accumulate=True)
        assert np.array_equal(as_.cpu().numpy(), a1.cpu().numpy() * f), f"{fid} accumulate"


# ------------------------------------------------------------------------------- backward modes
#        id              family        graph D    k   mode      chunk  extra
BWD = [("auto-k16",      "bwd auto",   "S",  256, 16, "auto",   0,    None),
       ("auto-k32",      "bwd auto",   "S",  256, 32, "auto",   0,    None),
       ("auto-D64-k32",  "bwd auto",   "S",  64,  32, "auto",   0,    None),
       ("pull-k16",      "bwd pull",   "S",  256, 16, "pull",   0,    None),
       ("pull-k32",      "bwd pull",   "S",  256, 32, "pull",   0,    None),
       ("pull-k10",      "bwd pull",   "S",  256, 10, "pull",   0,    None),  # one l per lane
       ("pull-Dn-k16",   "bwd pull",   "Dn", 256, 16, "pull",   0,    None),
       ("csc-c0",        "bwd csc",    "S",  256, 16, "csc",    0,    None),
       ("csc-c13",       "bwd csc",    "S",  256, 16, "csc",    13,   None),
       ("csc-c4096",     "bwd csc",    "S",  256, 16, "csc",    4096, None),  # unstaged phase 2
       ("csc-k32",       "bwd csc",    "S",  256, 32, "csc",    0,    None),
       ("csc-Dn-k16",    "bwd csc",    "Dn", 256, 16, "csc",    0,    None),
       ("csc-sel",       "bwd csc-sel", "S", 256, 16, "csc",    0,    "edge_sel"),
       ("csc-sel-c13",   "bwd csc-sel", "S", 256, 16, "csc",    13,   "edge_sel"),
       ("bsort-k8",      "bwd bsort",  "S",  256, 8,  "bsort",  0,    None),
       ("bsort-k16",     "bwd bsort",  "S",  256, 16, "bsort",  0,    None),
       ("hybrid-d0",     "bwd hybrid", "S",  256, 16, "hybrid", 0,    0.0),   # every tile pulled
       ("hybrid-d0.5",   "bwd hybrid", "S",  256, 16, "hybrid", 0,    0.5),   # a mix
       ("hybrid-d3",     "bwd hybrid", "S",  256, 16, "hybrid", 0,    3.0),   # the hub tiles only
       ("hybrid-none",   "bwd hybrid", "S",  256, 16, "hybrid", 0,    1e9),   # none: all csc
       ("atomic-k16",    "bwd atomic", "S",  256, 16, "atomic", 0,    None),
       ("atomic-k32-c13", "bwd atomic", "S", 256, 32, "atomic", 13,   None),
       ("dense-rows",    "bwd dense",  "S",  64,  32, "dense",  0,    None),
       ("dense-rows-c13", "bwd dense", "S",  64,  32, "dense",  13,   None),
       ("dense-cols",    "bwd dense",  "S",  64,  16, "dense",  0,    None)]
BWD_IDS = [b[0] for b in BWD]
BITWISE = [b for b in BWD if b[5] in ("csc", "dense")]


def run_bwd(mk, name, G, ci, mode, chunk, extra, validate=None, gt=None):
    rp, col, ev, div = dgraph(name) if gt is None else gt
    g = graph(name)
    k, D = ci.shape[1], G.shape[1]
    kw = {}
    if extra == "edge_sel":
        kw["edge_sel"] = mk.edge_selectors(col, ci)
    elif mode == "hybrid":
        plan = kw["plan"] = mk.hybrid_plan(rp, col, ev, g.C, k, D, density=extra, cache=False)
        if extra == 0.0:
            assert plan[7][1].numel() == 0  # no edge left to the csc part
        if extra >= 1e9:
            assert plan[0].numel() == 0     # no tile pulled
    return mk.sspmm_backward(rp, col, ev, G, ci, row_div=div, chunk=chunk, mode=mode,
                             validate=validate, **kw)


@quiet_bsort
@pytest.mark.parametrize("regime", N.REGIMES)
@pytest.mark.parametrize("bid,family,name,D,k,mode,chunk,extra", BWD, ids=BWD_IDS)
def test_backward_bound(mk, cuda, bid, family, name, D, k, mode, chunk, extra, regime):
    """(a) and (d): every backward mode.  The atomic mode shares the bound: the order of its fp32
    atomics changes which rounding happens, not how many."""
    c = case(name, D, k, regime)
    gs = run_bwd(mk, name, T(c["G"], cuda), T(c["ci"], cuda), mode, chunk, extra)
    note(family, N.within(gs, c["go"], c["bg"], bid))
    if regime == "subnormal":
        N.nonzero_where_resolved(gs, c["go"], c["bg"])


@pytest.mark.parametrize("s", [-20, 40])
@pytest.mark.parametrize("bid,family,name,D,k,mode,chunk,extra", BITWISE,
                         ids=[b[0] for b in BITWISE])
def test_backward_scale_equivariant(mk, cuda, bid, family, name, D, k, mode, chunk, extra, s):
    """(b): csc, csc with edge_sel= and both dense forms, the bitwise-repeatable modes."""
    c = case(name, D, k, "unit")
    ci = T(c["ci"], cuda)
    f = np.float32(2.0 ** s)
    g1 = run_bwd(mk, name, T(c["G"], cuda), ci, mode, chunk, extra).cpu().numpy()
    gs = run_bwd(mk, name, T(c["G"] * f, cuda), ci, mode, chunk, extra).cpu().numpy()
    assert np.array_equal(gs, g1 * f), bid


# ------------------------------------------------------------------------------- (c) Inf and NaN
POISON_SHAPES = [("S", 256, 32), ("S", 256, 16), ("S", 64, 32), ("S", 100, 28), ("S", 100, 10),
                 ("Dn", 256, 16)]
POISON_IDS = [f"{n}-D{D}-k{k}" for n, D, k in POISON_SHAPES]


@functools.lru_cache(maxsize=None)
def poisoned(name, D, k):
    g = graph(name)
    c = case(name, D, k, "unit")
    cvp, cip, Gp, where = N.poison(g, c["cv"], c["ci"], c["G"], D)
    yo, go = N.fwd_ref(g, cvp, cip, D), N.bwd_ref(g, Gp, cip)
    N.reference_is_meaningful(yo)  # each class occurs; at most 5 % non-finite
    N.reference_is_meaningful(go)
    pre = N.poison_prefill(np.random.default_rng(D + k), yo)
    return dict(g=g, cv=cvp, ci=cip, G=Gp, where=where, yo=yo, go=go, pre=pre,
                by=N.bound_fwd(g, cvp, cip, D), ya=N.add_prefill(yo, pre),
                bya=N.bound_fwd(g, cvp, cip, D, prefill=pre), bg=N.bound_bwd(g, Gp, cip))


def bits(t):
    return t.contiguous().view(torch.int32)


# the transport-record shapes (k % 4 == 0 in [24, 32], maxk_records_ok) also go through
# mk.cbsr_records + mk.spgemm_forward_records
POISON_FWD = [(n, D, k, v) for n, D, k in POISON_SHAPES for v in ("plain", "emit")] + \
             [("S", 256, 32, "records"), ("S", 100, 28, "records")]


@pytest.mark.parametrize("name,D,k,variant", POISON_FWD,
                         ids=[f"{n}-D{D}-k{k}-{v}" for n, D, k, v in POISON_FWD])
def test_forward_inf_nan(mk, cuda, name, D, k, variant):
    """(c): +inf, -inf and NaNs of three bit patterns (the records' skip marker among them) in
    selected slots, repeated selectors over (+inf, -inf) and (+inf, finite), a NaN behind a
    selector >= D, a NaN vertex no edge reads, and a poisoned accumulate prefill: the class
    masks equal the oracle's and the finite rest stays inside the bound."""
    p = poisoned(name, D, k)
    g = p["g"]
    if variant == "records":
        assert mk.records_ok(g.R, g.C, g.col.size, D, k)
    cv, ci = T(p["cv"], cuda), T(p["ci"], cuda)
    clean = p["cv"].copy()
    clean[g.unread] = 1.0
    for chunk in CHUNKS:
        y = run_fwd(mk, name, variant, cv, ci, D, chunk, validate=False)
        N.within(y, p["yo"], p["by"], f"{variant} chunk {chunk}")
        # the vertex no edge reads: bitwise the run without its NaNs
        y2 = run_fwd(mk, name, variant, T(clean, cuda), ci, D, chunk, validate=False)
        assert torch.equal(bits(y), bits(y2))
        acc = T(p["pre"], cuda)
        run_fwd(mk, name, variant, cv, ci, D, chunk, out=acc, accumulate=True, validate=False)
        N.within(acc, p["ya"], p["bya"], f"{variant} chunk {chunk} accumulate")


POISON_MODES = [("auto", None), ("pull", None), ("csc", None), ("csc", "edge_sel"),
                ("bsort", None), ("hybrid", 0.5), ("atomic", None), ("dense", None)]


POISON_BWD = [(n, D, k, m, e) for n, D, k in POISON_SHAPES for m, e in POISON_MODES
              if k % 4 == 0 or (m in ("auto", "pull", "csc", "atomic") and e is None)]


@quiet_bsort
@pytest.mark.parametrize("name,D,k,mode,extra", POISON_BWD,
                         ids=[f"{n}-D{D}-k{k}-{m}" + ("" if e is None else f"-{e}")
                              for n, D, k, m, e in POISON_BWD])
def test_backward_inf_nan(mk, cuda, name, D, k, mode, extra):
    """(c): +inf in the hub row's G row, -inf and NaNs of every pattern in short rows' G rows
    (each in a column several destinations select), repeated selectors, a destination whose
    selector >= D reads 0 beside a +inf slot, and an all-NaN G row of a source row without
    edges: the class masks equal the oracle's, whichever order the mode sums in."""
    p = poisoned(name, D, k)
    for chunk in (0, 13):
        gs = run_bwd(mk, name, T(p["G"], cuda), T(p["ci"], cuda), mode, chunk, extra,
                     validate=False)
        N.within(gs, p["go"], p["bg"], f"{mode} chunk {chunk}")
    if "past" in p["where"]:
        v, slot = p["where"]["past"]
        row = gs[v].cpu().numpy()
        assert row[slot] == 0.0 and not np.isfinite(row[0])


# ------------------------------------------------------------------------------- (e) autograd
@pytest.mark.parametrize("via", ["v1", "v4"])
def test_autograd_inf_nan_reach_input_grad(cuda, via):
    """(e): a grad_output with one Inf and one NaN through maxk_spgemm (v1) and the
    MaxKSpmmWrapper v4 path: x.grad has the oracle's class masks (its backward, scattered), so
    torch.isfinite(x.grad).all() -- what a loss scaler looks at -- is False."""
    import maxk_spgemm_function as F
    name, D, k = "S", 256, 32
    g = graph(name)
    rp, col, ev, div = dgraph(name)
    rng = np.random.default_rng(99)
    x = rng.standard_normal((g.C, D), dtype=np.float32)
    cv, ci = O.topk(x, k)
    G = rng.standard_normal((g.R, D), dtype=np.float32)
    _, _, Gall, where = N.poison(g, cv, ci, G, D)
    (ri, ji), (rn, jn) = where["G"][0], where["G"][2]  # the hub row's +inf, a short row's NaN
    G[ri, ji], G[rn, jn] = np.inf, np.nan
    go = N.bwd_ref(g, G, ci)
    ref = O.scatter_dense(go, ci, D)
    bound = np.zeros((g.C, D))
    np.put_along_axis(bound, ci.astype(np.int64), N.bound_bwd(g, G, ci), axis=1)
    assert np.isnan(ref).any() and np.isposinf(ref).any()
    xt = T(x, cuda).requires_grad_(True)
    if via == "v1":
        y = F.maxk_spgemm(col, ev, xt, k, graph_indptr=rp, in_degrees=div, out_degrees=div)
    else:
        w = F.MaxKSpmmWrapper("numerics")
        assert w.build_metadata(rp)
        ti = T(ci, cuda, torch.int64)
        y = w.spmm(col, ev, xt.gather(1, ti), ti, rp, div, dim_origin=D)
    y.backward(T(G, cuda))
    N.within(xt.grad, ref, bound, via)
    assert not torch.isfinite(xt.grad).all()
