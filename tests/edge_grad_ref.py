"""Expected values of the edge-weight gradient, in plain numpy (a helper, like tests/numerics.py).

    grad_edge[e] = ( sum_l cbsr_val[c, l] * G[r, cbsr_idx[c, l]] ) / row_div[r]
                   r = the CSR row holding e, c = col_idx[e], over the selectors below D

The CPU oracle has no such function, so the dot products are formed here in float64 (Inf and NaN
follow IEEE through numpy's multiply and sum).  Per edge:

ref    the float64 result (cast by the caller where it compares classes);
n      the number of column c's selectors below D (repeated ones counted each);
s_abs  sum |term| / row_div over the finite terms;
bound  numerics' own: (n + 8) * (2^-24 * s_abs + unit), 0 where n = 0 -- the roundings are the
       n products, at most n - 1 inexact additions of the tree (adding a skipped slot's 0 is
       exact) and the division, within the + 8 that numerics allows for what does not grow
       with n.

test_edge_grad_cpu.py pins this helper against torch autograd on a dense float64 restatement.
"""
from collections import namedtuple

import numpy as np

import numerics as N

EdgeRef = namedtuple("EdgeRef", "ref n s_abs")
BLOCK = 4096  # edges per step: E x k float64 temporaries stay small at k = 256


def edge_rows(rp):
    """The CSR row of every edge."""
    return np.repeat(np.arange(rp.size - 1), np.diff(rp))


def edge_grad_ref(rp, col, cv, ci, G, div=None):
    """EdgeRef of a CSR (rp, col), a CBSR (cv, ci), G [R, D] and row_div (None: no division)."""
    D = G.shape[1]
    E = col.size
    rows = edge_rows(rp)
    Gp = np.zeros((G.shape[0], N.FULL), np.float64)
    Gp[:, :D] = G
    sel = ci.astype(np.int64)
    ref = np.zeros(E, np.float64)
    n = np.zeros(E, np.int64)
    s_abs = np.zeros(E, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):  # a signalling NaN warns when widened
        cv64 = cv.astype(np.float64)
        for a in range(0, E, BLOCK):
            r, c = rows[a:a + BLOCK], col[a:a + BLOCK]
            s = sel[c]                                  # [b, k]
            keep = s < D
            t = np.where(keep, cv64[c] * Gp[r[:, None], s], 0.0)
            ref[a:a + BLOCK] = t.sum(1)
            n[a:a + BLOCK] = keep.sum(1)
            s_abs[a:a + BLOCK] = np.where(np.isfinite(t), np.abs(t), 0.0).sum(1)
        if div is not None:
            d = div.astype(np.float64)[rows]
            ref, s_abs = ref / d, s_abs / d
    return EdgeRef(ref, n, s_abs)


def bound(er, unit=0.0):
    """The per-edge bound, built by numerics' own rule."""
    return N._bound(er.n, er.s_abs, unit)


def as_f32(ref):
    """The reference as fp32 (for the class masks: a float64 sum past fp32's range is +-inf)."""
    with np.errstate(over="ignore"):
        return ref.astype(np.float32)
