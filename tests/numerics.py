"""Value-level comparison helpers for the aggregation kernels (plain numpy over the CPU oracle).

The parity tests check shapes with an absolute 1e-4 tolerance on N(0,1) values.  These helpers
check values: a per-element rounding bound that follows the magnitude of each output's own
terms, exact agreement of the NaN / +inf / -inf masks, and input generators for magnitudes far
from 1.

Bound (standard forward-error analysis of an n-term fp32 sum, first order in 2^-24):

    |hip - oracle| <= (n + 8) * 2^-24 * S_abs + floor

n     the number of addends of the output element: the oracle on all-ones weights and values
      (duplicates and edges counted);
S_abs the oracle on |edge_val| and |values| with the same row_div (over the finite terms);
+ 8   the roundings that do not depend on n: the division by row_div on either side of the
      sum, a product's rounding, the pull's weights pre-divided by row_div, the final cast of
      both sides -- not a measured number;
floor 0, or (n + 8) * 2^-149 for fp32-subnormal inputs, where every product is rounded to a
      multiple of 2^-149 whatever its size.

An element with n = 0 (a row without edges, a column nobody selects, a vertex without in-edges)
has bound 0: it must be exactly 0.

Selectors >= D contribute nothing: every oracle call here runs at width 256 and is cut back.
"""
from collections import namedtuple

import numpy as np

import oracle as O

EPS = 2.0 ** -24
EXTRA = 8
FULL = 256
SUBNORMAL_UNIT = 2.0 ** -149

REGIMES = ("unit", "small", "large", "mixed", "subnormal")

#: the records' skip marker, a negative quiet NaN, a signalling NaN with the smallest payload
NAN_PATTERNS = (0x7FBADBAD, 0xFFC00000, 0x7F800001)

Graph = namedtuple("Graph", "rp col ev div R C hub unread")


# ------------------------------------------------------------------------------- inputs
def values(rng, shape, regime):
    """cbsr_val / grad_out / prefill of a regime, fp32."""
    if regime == "unit":
        return rng.standard_normal(shape).astype(np.float32)
    if regime == "small":
        return (rng.standard_normal(shape) * 2.0 ** -20).astype(np.float32)
    if regime == "large":  # partial sums stay below 2^55: no overflow
        return (rng.standard_normal(shape) * 2.0 ** 40).astype(np.float32)
    if regime == "mixed":  # +-m * 2^e: the outputs of one row span twelve orders of magnitude
        m = rng.uniform(1.0, 2.0, shape)
        e = rng.integers(-30, 11, shape)
        return (np.ldexp(m, e) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    if regime == "subnormal":
        return (rng.standard_normal(shape) * 2.0 ** -130).astype(np.float32)
    raise ValueError(regime)


def floor_unit(regime):
    return SUBNORMAL_UNIT if regime == "subnormal" else 0.0


def drop_column(rp, col, c):
    """The CSR without the edges into column c."""
    keep = col != c
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))[keep]
    rp2 = np.zeros_like(rp)
    rp2[1:] = np.cumsum(np.bincount(rows, minlength=rp.size - 1))
    return rp2, np.ascontiguousarray(col[keep])


def make_graph(rng, rp, col, C=None, unread=None):
    """Weights uniform in [0.5, 1.5) and row_div = max(deg, 1): finite and away from 0, so the
    class of every product depends on the values alone.  `unread`: a column whose in-edges are
    deleted (a vertex no edge reads)."""
    if unread is not None:
        rp, col = drop_column(rp, col, unread)
    R = rp.size - 1
    C = R if C is None else C
    ev = rng.uniform(0.5, 1.5, col.size).astype(np.float32)
    deg = np.diff(rp)
    div = np.maximum(deg, 1).astype(np.float32)
    return Graph(rp.astype(np.int32), col.astype(np.int32), ev, div, R, C, int(np.argmax(deg)),
                 unread)


def named_graph(name, rand_graph):
    """The module graphs, the smallest that still reach each code path (rand_graph: the parity
    tests' generator).  S: V = 600, average degree 12, hub rows of 590 and 200 edges, 20 empty
    rows.  Dn: V = 400, average degree 160 (>= 128: the forward's dense-graph rules), a hub row
    of 390.  R: rectangular, 150 x 700, average degree 40.  One column of each has no in-edge."""
    rng = np.random.default_rng({"S": 7001, "Dn": 7002, "R": 7003}[name])
    if name == "S":
        rp, col = rand_graph(rng, 600, 12, hubs=((3, 590), (100, 200)), empty=20)
        return make_graph(rng, rp, col, 600, unread=411)
    if name == "Dn":
        rp, col = rand_graph(rng, 400, 160, hubs=((3, 390),))
        return make_graph(rng, rp, col, 400, unread=211)
    if name == "R":
        rp, col = rand_graph(rng, 150, 40, cols=700)
        return make_graph(rng, rp, col, 700, unread=555)
    raise ValueError(name)


def selectors(rng, C, D, k):
    """k distinct selectors per vertex, in top-k order of a random row."""
    return O.topk(rng.standard_normal((C, D), dtype=np.float32), k)[1]


# ------------------------------------------------------------------------------- oracle
def fwd_ref(g, cv, ci, D):
    return O.spgemm_fwd(g.rp, g.col, g.ev, cv, ci, FULL, row_div=g.div)[:, :D]


def _pad(G):
    if G.shape[1] == FULL:
        return G
    Gp = np.zeros((G.shape[0], FULL), np.float32)
    Gp[:, :G.shape[1]] = G
    return Gp


def bwd_ref(g, G, ci):
    return O.sspmm_bwd(g.rp, g.col, g.ev, _pad(G), ci, row_div=g.div)


def bwd_ref_pull(g, G, ci):
    tp, ts, tv = O.transpose(g.rp, g.col, g.ev, g.C)
    return O.sspmm_bwd_pull(tp, ts, tv, _pad(G), ci, row_div=g.div)


def _finite_abs(a):
    return np.where(np.isfinite(a), np.abs(a), 0).astype(np.float32)


def _bound(n, s_abs, unit):
    n = np.rint(n.astype(np.float64))
    return np.where(n > 0, (n + EXTRA) * (EPS * s_abs.astype(np.float64) + unit), 0.0)


def count_fwd(g, ci, D):
    """Addends per forward output element (no row_div: a count)."""
    one_e = np.ones_like(g.ev)
    return O.spgemm_fwd(g.rp, g.col, one_e, np.ones(ci.shape, np.float32), ci, FULL)[:, :D]


def count_bwd(g, ci, D):
    G = np.zeros((g.R, FULL), np.float32)
    G[:, :D] = 1.0
    return O.sspmm_bwd(g.rp, g.col, np.ones_like(g.ev), G, ci)


def bound_fwd(g, cv, ci, D, prefill=None, unit=0.0, n=None):
    """Per-element bound of the forward; `prefill` (accumulate) is one more addend."""
    n = count_fwd(g, ci, D) if n is None else n
    s = O.spgemm_fwd(g.rp, g.col, g.ev, _finite_abs(cv), ci, FULL, row_div=g.div)[:, :D]
    s = s.astype(np.float64)
    if prefill is not None:
        n = n + 1.0
        s = s + _finite_abs(prefill)
    return _bound(n, s, unit)


def bound_bwd(g, G, ci, unit=0.0, n=None):
    n = count_bwd(g, ci, G.shape[1]) if n is None else n
    s = O.sspmm_bwd(g.rp, g.col, g.ev, _pad(_finite_abs(G)), ci, row_div=g.div)
    return _bound(n, s, unit)


# ------------------------------------------------------------------------------- checks
def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def same_class(a, ref):
    """The NaN, +inf and -inf masks of `a` equal the reference's exactly; returns the mask of
    the elements finite in `ref` (the ones left for the bound)."""
    a, ref = _np(a), _np(ref)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    for name, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        ma, mr = f(a), f(ref)
        if not np.array_equal(ma, mr):
            extra, lost = np.argwhere(ma & ~mr), np.argwhere(mr & ~ma)
            raise AssertionError(
                f"{name} mask differs: {len(extra)} unexpected (first {extra[:3].tolist()}), "
                f"{len(lost)} missing (first {lost[:3].tolist()}) of {int(mr.sum())} expected")
    return np.isfinite(ref)


def ratio(a, ref, bound):
    """max err / bound over the elements finite in ref with a bound > 0; inf where an element
    with bound 0 is not exactly 0 or a finite reference meets a non-finite value."""
    a, ref = _np(a).astype(np.float64), _np(ref).astype(np.float64)
    fin = np.isfinite(ref)
    err = np.where(fin, np.abs(np.where(fin, a, 0.0) - np.where(fin, ref, 0.0)), 0.0)
    err = np.where(fin & ~np.isfinite(a), np.inf, err)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / bound)
    return float(q[fin].max()) if fin.any() else 0.0


def within(a, ref, bound, what=""):
    """same_class, then |a - ref| <= bound on the finite rest; returns the largest err / bound."""
    same_class(a, ref)
    r = ratio(a, ref, bound)
    if not r <= 1.0:
        a64, r64 = _np(a).astype(np.float64), _np(ref).astype(np.float64)
        fin = np.isfinite(r64)
        bad = fin & ~(np.abs(np.where(fin, a64 - r64, 0.0)) <= bound)
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {int(fin.sum())} elements past the bound, worst "
            f"err/bound {r:.3g}; first at {i}: got {a64[i]!r}, oracle {r64[i]!r}, "
            f"bound {bound[i]:.3g}")
    return r


def nonzero_where_resolved(a, ref, bound):
    """Subnormal regime: wherever the oracle's magnitude exceeds the bound (so 0 is past it
    anyway) the output is non-zero -- spelled out, since a flush to zero is the failure this
    regime looks for."""
    a, ref = _np(a), _np(ref)
    big = np.abs(ref.astype(np.float64)) > bound
    assert big.any(), "no output above the floor: the case checks nothing"
    lost = big & (a == 0)
    assert not lost.any(), f"{int(lost.sum())} of {int(big.sum())} resolvable outputs flushed to 0"


def reference_is_meaningful(ref):
    """The two conditions on a poisoned case's expected output: each class occurs, and at most
    5 % is non-finite (the bound still checks the rest)."""
    assert np.isnan(ref).any() and np.isposinf(ref).any() and np.isneginf(ref).any(), \
        (int(np.isnan(ref).sum()), int(np.isposinf(ref).sum()), int(np.isneginf(ref).sum()))
    share = 1.0 - np.isfinite(ref).mean()
    assert share <= 0.05, f"{share:.3%} of the expected output is non-finite"
    return share


# ------------------------------------------------------------------------------- fp32 emulation
def emulate_fwd(g, cv, ci, D):
    """The forward as a straight fp32 sequential sum in CSR order (products rounded, then
    added), divided by row_div at the end."""
    out = np.zeros((g.R, D), np.float32)
    sel = ci.astype(np.int64)
    for r in range(g.R):
        acc = np.zeros(FULL, np.float32)
        for e in range(g.rp[r], g.rp[r + 1]):
            c = g.col[e]
            np.add.at(acc, sel[c], g.ev[e] * cv[c])
        out[r] = (acc / g.div[r])[:D]
    return out


def emulate_bwd(g, G, ci):
    """The backward as a straight fp32 sequential push in CSR order, G / row_div first."""
    out = np.zeros(ci.shape, np.float32)
    sel = ci.astype(np.int64)
    Gp = _pad(G)
    for r in range(g.R):
        gr = Gp[r] / g.div[r]
        for e in range(g.rp[r], g.rp[r + 1]):
            c = g.col[e]
            out[c] += g.ev[e] * gr[sel[c]]
    return out


def truncate_tf32(a):
    """fp32 with the mantissa cut to 10 bits."""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFFE000)).view(
        np.float32)


# ------------------------------------------------------------------------------- Inf / NaN
def _set_bits(a, idx, bits):
    a.view(np.uint32)[idx] = np.uint32(bits)


def _readers(g):
    """Per column, the rows that read it."""
    order = np.argsort(g.col, kind="stable")
    rows = np.repeat(np.arange(g.R), np.diff(g.rp))[order]
    ptr = np.searchsorted(g.col[order], np.arange(g.C + 1))
    return [rows[ptr[c]:ptr[c + 1]] for c in range(g.C)]


def poison(g, cv, ci, G, D):
    """Non-finite inputs at positions chosen from the graph; returns (cv, ci, G, where).

    cbsr_val (forward), each on its own vertex read by the hub row and by at least one other
    row (those with the shortest other reader first): +inf, -inf and a NaN in a selected slot;
    NaNs of NAN_PATTERNS; a repeated selector over +inf and -inf (the column becomes NaN) and
    over +inf and a finite value (+inf); at D < 256 a slot with selector >= D holding NaN
    (contributes nothing).  The vertex no edge reads is all NaN.
    grad_out (backward): +inf in the hub row's G row, -inf and the NaNs in five short rows' G
    rows, each in the column most of that row's destinations select; an empty source row's G
    row is all NaN.  The destination with the selector >= D is one of the hub row's, and the
    hub row's G row holds a second +inf in the column that destination's slot 0 selects: its
    slot 0 is +inf while the slot with the selector >= D reads 0.
    """
    cv, ci, G = cv.copy(), ci.copy(), G.copy()
    k = ci.shape[1]
    deg = np.diff(g.rp)
    readers = _readers(g)
    hubcols = g.col[g.rp[g.hub]:g.rp[g.hub + 1]]
    cand = []
    for c in hubcols:
        others = readers[c][readers[c] != g.hub]
        if others.size and c != g.unread:
            cand.append((int(deg[others].min()), int(c)))
    verts = [c for _, c in sorted(cand)][:9]
    assert len(verts) == 9
    where = {"verts": verts}
    cv[verts[0], 0] = np.inf
    cv[verts[1], 1 % k] = -np.inf
    cv[verts[2], 2 % k] = np.nan
    for v, slot, bits in zip(verts[3:6], (0, 3 % k, k - 1), NAN_PATTERNS):
        _set_bits(cv, (v, slot), bits)
    ci[verts[6], 1] = ci[verts[6], 0]
    cv[verts[6], 0], cv[verts[6], 1] = np.inf, -np.inf
    ci[verts[7], k - 1] = ci[verts[7], 0]
    cv[verts[7], 0] = np.inf
    if D < FULL:
        ci[verts[8], 1] = 200
        cv[verts[8], 1] = np.nan
        where["past"] = (verts[8], 1)
    if g.unread is not None:
        cv[g.unread] = np.nan

    def hot_column(r):  # the column most of row r's destinations select
        sel = ci[g.col[g.rp[r]:g.rp[r + 1]]].ravel()
        cnt = np.bincount(sel[sel < D], minlength=D)
        return int(np.argmax(cnt)), int(cnt.max())
    short = [int(r) for r in np.argsort(deg, kind="stable") if deg[r] >= 3 and r != g.hub][:5]
    assert len(short) == 5
    j, cnt = hot_column(g.hub)
    assert cnt >= 2
    G[g.hub, j] = np.inf
    where["G"] = [(g.hub, j)]
    if D < FULL:  # the destination with the selector >= D reads this +inf in its slot 0
        G[g.hub, ci[verts[8], 0]] = np.inf
        where["G"].append((g.hub, int(ci[verts[8], 0])))
    for r, bits in zip(short, (0xFF800000, 0x7FC00000) + NAN_PATTERNS):
        j, _ = hot_column(r)
        _set_bits(G, (r, j), bits)
        where["G"].append((r, j))
    empty = np.flatnonzero(deg == 0)
    if empty.size:
        G[empty[0]] = np.nan
        where["empty"] = int(empty[0])
    return cv, ci, G, where


def poison_prefill(rng, ref, regime="unit"):
    """An accumulate prefill of the regime's magnitude with a +inf and a -inf where the product
    is finite (they stay) and finite values where the product is NaN (they become NaN)."""
    pre = values(rng, ref.shape, regime)
    fin = np.argwhere(np.isfinite(ref) & (ref != 0))
    assert len(fin) >= 2
    a, b = fin[len(fin) // 3], fin[2 * len(fin) // 3]
    pre[tuple(a)] = np.inf
    pre[tuple(b)] = -np.inf
    return pre


def add_prefill(ref, pre):
    """The accumulate reference: oracle + prefill, summed in double."""
    with np.errstate(invalid="ignore"):
        return (ref.astype(np.float64) + pre.astype(np.float64)).astype(np.float32)
