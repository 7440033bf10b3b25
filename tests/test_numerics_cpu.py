"""The comparison helpers of tests/numerics.py proved without a GPU: a straight fp32 sequential
sum passes the bound in every regime, deliberately wrong results are rejected, and the expected
NaN / Inf classes do not depend on the summation order (push and pull oracles agree).

V = 600 graph (hub rows of 590 and 200 edges, empty rows), D, k = (256, 32) and (64, 32).
"""
import functools

import numpy as np
import pytest

import numerics as N
import oracle as O
from test_parity_gpu import rand_graph

SHAPES = [(256, 32), (64, 32)]


@functools.lru_cache(maxsize=None)
def graph(name="S"):
    return N.named_graph(name, rand_graph)


@functools.lru_cache(maxsize=None)
def case(D, k, regime):
    """Inputs, oracle results and bounds of one shape and regime, computed once."""
    g = graph()
    rng = np.random.default_rng(D * 1000 + k + len(regime))
    ci = N.selectors(rng, g.C, D, k)
    cv = N.values(rng, (g.C, k), regime)
    G = N.values(rng, (g.R, D), regime)
    unit = N.floor_unit(regime)
    return dict(g=g, ci=ci, cv=cv, G=G, yo=N.fwd_ref(g, cv, ci, D), go=N.bwd_ref(g, G, ci),
                by=N.bound_fwd(g, cv, ci, D, unit=unit), bg=N.bound_bwd(g, G, ci, unit=unit))


@pytest.mark.parametrize("regime", N.REGIMES)
@pytest.mark.parametrize("D,k", SHAPES)
def test_fp32_sequential_sum_passes(D, k, regime):
    """A legitimate fp32 kernel -- products rounded, summed in CSR order -- stays inside the
    bound in every regime, with at least a factor 2 to spare outside the subnormal one; the
    elements without addends are exactly 0."""
    c = case(D, k, regime)
    ry = N.within(N.emulate_fwd(c["g"], c["cv"], c["ci"], D), c["yo"], c["by"], "forward")
    rg = N.within(N.emulate_bwd(c["g"], c["G"], c["ci"]), c["go"], c["bg"], "backward")
    print(f"fp32 emulation D={D} k={k} {regime}: err/bound forward {ry:.3f} backward {rg:.3f}")
    if regime != "subnormal":
        assert ry <= 0.5 and rg <= 0.5
    assert (c["by"] == 0).any() and (c["bg"] == 0).any()  # empty rows, the unread vertex
    if regime == "subnormal":
        N.nonzero_where_resolved(N.emulate_fwd(c["g"], c["cv"], c["ci"], D), c["yo"], c["by"])


@pytest.mark.parametrize("regime", ["unit", "small", "large", "mixed"])
@pytest.mark.parametrize("D,k", SHAPES)
def test_tf32_truncation_rejected(D, k, regime):
    """cbsr_val / grad_out cut to a 10-bit mantissa: the exact sums of the truncated values are
    past the bound on most outputs that have addends (the 1e-4 tolerance passes 99.7 %)."""
    c = case(D, k, regime)
    y = N.fwd_ref(c["g"], N.truncate_tf32(c["cv"]), c["ci"], D)
    gs = N.bwd_ref(c["g"], N.truncate_tf32(c["G"]), c["ci"])
    for a, ref, b in ((y, c["yo"], c["by"]), (gs, c["go"], c["bg"])):
        with pytest.raises(AssertionError):
            N.within(a, ref, b)
        live = b > 0
        bad = np.abs(a.astype(np.float64) - ref) > b
        assert bad[live].mean() > 0.5, bad[live].mean()


@pytest.mark.parametrize("D,k", SHAPES)
def test_small_magnitudes_are_resolved(D, k):
    """At 2^-20 every reference output is below 1e-4, where the parity tolerance is absolute:
    an all-zero output and a hub row that lost one edge pass it, and fail the bound."""
    c = case(D, k, "small")
    g = c["g"]
    assert np.abs(c["yo"]).max() < 1e-4 and np.abs(c["go"]).max() < 1e-4
    for ref, b in ((c["yo"], c["by"]), (c["go"], c["bg"])):
        with pytest.raises(AssertionError):
            N.within(np.zeros_like(ref), ref, b)
    ev = g.ev.copy()
    ev[g.rp[g.hub] + 17] = 0.0  # the hub row without one of its edges
    lost = g._replace(ev=ev)
    y = N.fwd_ref(lost, c["cv"], c["ci"], D)
    gs = N.bwd_ref(lost, c["G"], c["ci"])
    assert np.abs(y - c["yo"]).max() < 1e-4 and np.abs(gs - c["go"]).max() < 1e-4
    with pytest.raises(AssertionError):
        N.within(y, c["yo"], c["by"])
    with pytest.raises(AssertionError):
        N.within(gs, c["go"], c["bg"])


@functools.lru_cache(maxsize=None)
def poisoned(name, D, k):
    g = graph(name)
    rng = np.random.default_rng(D * 77 + k)
    ci = N.selectors(rng, g.C, D, k)
    cv = N.values(rng, (g.C, k), "unit")
    G = N.values(rng, (g.R, D), "unit")
    cvp, cip, Gp, where = N.poison(g, cv, ci, G, D)
    return dict(g=g, cv=cv, ci=ci, G=G, cvp=cvp, cip=cip, Gp=Gp, where=where,
                yo=N.fwd_ref(g, cvp, cip, D), go=N.bwd_ref(g, Gp, cip))


POISON_SHAPES = [("S", 256, 32), ("S", 256, 16), ("S", 64, 32), ("S", 100, 28), ("S", 100, 10),
                 ("Dn", 256, 16)]


@pytest.mark.parametrize("name,D,k", POISON_SHAPES)
def test_poisoned_reference(name, D, k):
    """The expected output of the Inf / NaN cases: every class occurs, at most 5 % is non-finite,
    the push and the pull oracle give identical class masks (the classes do not depend on the
    summation order), and each poison lands where the contract says."""
    p = poisoned(name, D, k)
    g, w = p["g"], p["where"]
    sy = N.reference_is_meaningful(p["yo"])
    sg = N.reference_is_meaningful(p["go"])
    print(f"{name} D={D} k={k}: non-finite share forward {sy:.3%} backward {sg:.3%}")
    N.same_class(N.bwd_ref_pull(g, p["Gp"], p["cip"]), p["go"])
    # forward: the NaN patterns, the +inf / -inf pair and the +inf / finite pair in the rows
    # that read them (a short reader of each vertex)
    readers = N._readers(g)
    v = w["verts"]

    def at(vert, slot):
        r = [r for r in readers[vert] if r != g.hub][0]
        return p["yo"][r, p["cip"][vert, slot]]
    assert at(v[0], 0) == np.inf and at(v[1], 1 % k) == -np.inf
    for vert, slot in zip(v[2:6], (2 % k, 0, 3 % k, k - 1)):
        assert np.isnan(at(vert, slot))
    assert np.isnan(at(v[6], 0)) and at(v[7], 0) == np.inf
    # the unread vertex and a selector >= D change nothing: bitwise the clean run elsewhere
    clean_cv = p["cvp"].copy()
    clean_cv[g.unread] = p["cv"][g.unread]
    if "past" in w:
        clean_cv[w["past"]] = 0.0
        assert p["go"][w["past"]] == 0.0  # reads 0 while the hub row's G row holds +inf
        assert not np.isfinite(p["go"][w["past"][0], 0])
    assert np.array_equal(N.fwd_ref(g, clean_cv, p["cip"], D), p["yo"], equal_nan=True)
    if "empty" in w:  # the empty source row's NaN row of G reaches no gradient
        Gc = p["Gp"].copy()
        Gc[w["empty"]] = 0.0
        assert np.array_equal(N.bwd_ref(g, Gc, p["cip"]), p["go"], equal_nan=True)


def test_class_errors_rejected():
    """same_class rejects a NaN replaced by 0, a +inf turned into -inf and a NaN moved one
    column -- each invisible or fatal to a tolerance on differences."""
    p = poisoned("S", 256, 32)
    for ref in (p["yo"], p["go"]):
        b = np.full(ref.shape, np.inf)
        N.within(ref.copy(), ref, b)
        i = tuple(np.argwhere(np.isnan(ref))[0])
        a = ref.copy()
        a[i] = 0.0
        with pytest.raises(AssertionError, match="NaN mask"):
            N.within(a, ref, b)
        a = ref.copy()
        a[tuple(np.argwhere(np.isposinf(ref))[0])] = -np.inf
        with pytest.raises(AssertionError, match=r"\+inf mask"):
            N.within(a, ref, b)
        a = ref.copy()
        j = (i[0], (i[1] + 1) % ref.shape[1])
        assert not np.isnan(ref[j])
        a[i], a[j] = ref[j], np.nan
        with pytest.raises(AssertionError, match="NaN mask"):
            N.within(a, ref, b)
        # a finite reference met by a non-finite value is past any bound
        a = ref.copy()
        a[tuple(np.argwhere(np.isfinite(ref))[0])] = np.inf
        with pytest.raises(AssertionError):
            N.within(a, ref, b)


def test_accumulate_prefill_reference():
    """The poisoned prefill: an Inf in out where the product is finite stays Inf, a finite out
    where the product is NaN becomes NaN."""
    p = poisoned("S", 256, 32)
    pre = N.poison_prefill(np.random.default_rng(5), p["yo"])
    ref = N.add_prefill(p["yo"], pre)
    assert np.array_equal(np.isnan(ref), np.isnan(p["yo"]))
    assert (np.isinf(ref) & np.isfinite(p["yo"])).sum() == 2
    b = N.bound_fwd(p["g"], p["cvp"], p["cip"], 256, prefill=pre)
    assert np.isfinite(b).all()
    N.within(ref, ref, b)
