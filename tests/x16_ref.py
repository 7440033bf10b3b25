"""Plain numpy float64 reference of the 16-bit-selector path (1 <= D <= 1024), and its bound.

The CPU oracle is u8 and fixed at width 256, so it cannot serve here.  topk ranks by the kernels'
order key (NaN largest, then the float order) with ties in ascending column order; fwd and bwd
are the definitions, summed in float64.  bound_* run the same two functions on absolute values
and on all-ones, which give S_abs and the addend count n of tests/numerics.py's bound,
|hip - ref| <= (n + 8) * 2^-24 * S_abs, exactly 0 where n = 0.
"""
import numpy as np

import numerics as N


def order_key(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    key = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(x), 0xFFFFFFFF, key)


def topk(x, k):
    """(fp32 values, int64 columns) of each row's k largest: key descending, column ascending."""
    cols = np.broadcast_to(np.arange(x.shape[1]), x.shape)
    idx = np.lexsort((cols, -order_key(x)), axis=1)[:, :k]
    return np.take_along_axis(x, idx, 1), idx


def scatter(cv, ci, D):
    """[C, D] float64: the CBSR as dense rows; repeated selectors add, selectors >= D drop."""
    X = np.zeros((cv.shape[0], D))
    rows = np.broadcast_to(np.arange(cv.shape[0])[:, None], ci.shape)
    ok = ci < D
    with np.errstate(invalid="ignore"):
        np.add.at(X, (rows[ok], ci[ok]), cv[ok].astype(np.float64))
    return X


def fwd(g, cv, ci, D):
    X = scatter(cv, ci.astype(np.int64), D)
    out = np.zeros((g.R, D))
    with np.errstate(invalid="ignore"):  # Inf - Inf is a NaN the kernels give too
        for r in range(g.R):
            e = slice(g.rp[r], g.rp[r + 1])
            out[r] = g.ev[e].astype(np.float64) @ X[g.col[e]] / g.div[r]
    return out


def bwd(g, G, ci):
    with np.errstate(invalid="ignore"):
        Gd = G / g.div[:, None].astype(np.float64)
    order = np.argsort(g.col, kind="stable")
    rows = np.repeat(np.arange(g.R), np.diff(g.rp))[order]
    ptr = np.searchsorted(g.col[order], np.arange(g.C + 1))
    Y = np.zeros((g.C, G.shape[1]))  # A^T . (G / row_div)
    with np.errstate(invalid="ignore"):
        for c in range(g.C):
            e = slice(ptr[c], ptr[c + 1])
            Y[c] = g.ev[order[e]].astype(np.float64) @ Gd[rows[e]]
    ci = ci.astype(np.int64)
    ok = ci < G.shape[1]
    return np.where(ok, np.take_along_axis(Y, np.where(ok, ci, 0), 1), 0.0)


def _unit(g):
    return g._replace(ev=np.ones_like(g.ev), div=np.ones_like(g.div))


def bound_fwd(g, cv, ci, D):
    """(bound, n) of the forward's elements; S_abs over the finite terms, as in numerics.py."""
    n = fwd(_unit(g), np.ones(cv.shape, np.float32), ci, D)
    return N._bound(n, fwd(g, N._finite_abs(cv), ci, D), 0.0), n


def bound_bwd(g, G, ci):
    n = bwd(_unit(g), np.ones(G.shape, np.float32), ci)
    return N._bound(n, bwd(g, N._finite_abs(G), ci), 0.0), n
