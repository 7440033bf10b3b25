"""The max aggregation on CBSR features restated in numpy: the yardstick of
test_max_aggregate_gpu.py, itself pinned against dense float64 torch in test_max_aggregate_cpu.py.

With X = scatter(CBSR) [C, D] (zeros where a row keeps nothing):

    out[r, j] = max over the edges e of row r of X[col[e], j]       0 for a row without edges
    arg[r, j] = the CSR edge index of the winner, or -1

Candidates of (r, j): the row's edges whose column keeps j, in CSR order.  A repeated selector
is folded into its first occurrence, which carries the fp32 sum of the values in l order (what
the kernels' record pack stores); a selector >= D is no candidate.  The first candidate with the
largest value wins (strict >, so the lower edge wins a tie; a NaN beats everything and the first
NaN stays).  If an edge of the row does not keep j its implicit +0.0 competes: it wins only when
0 > best strictly, or alone; then arg = -1 and out = +0.0.  out carries the winner's bits.

    grad_cbsr[c, l] = sum over the edges e = (r <- c) of [arg[r, ci[c, l]] == e] * G[r, ci[c, l]]

in float64, with the project's sum bound (numerics.py): (n + 8) * 2^-24 * sum |terms|, n the
number of addends, 0 -- an exact zero -- for an element without one.

Plain loops over rows and edges; only the k slots of one edge are handled as a vector (they name
distinct columns once folded).
"""
from collections import namedtuple

import numpy as np

import numerics as N

Backward = namedtuple("Backward", "grad bound n")


def folded(cv, ci, D):
    """Per column (selectors, values) of its candidates: first occurrences, the repeats added in
    l order in fp32, selectors >= D dropped."""
    out = []
    for c in range(ci.shape[0]):
        sel, val, at = [], [], {}
        for l in range(ci.shape[1]):
            j = int(ci[c, l])
            if j in at:
                val[at[j]] = np.float32(val[at[j]] + cv[c, l])
            else:
                at[j] = len(sel)
                sel.append(j)
                val.append(np.float32(cv[c, l]))
        keep = [i for i, j in enumerate(sel) if j < D]
        out.append((np.array([sel[i] for i in keep], np.int64),
                    np.array([val[i] for i in keep], np.float32)))
    return out


def forward(rp, col, cv, ci, D):
    """(out float32 [R, D], arg int32 [R, D])."""
    R = rp.size - 1
    cand = folded(np.asarray(cv, np.float32), ci, D)
    out = np.zeros((R, D), np.float32)
    arg = np.full((R, D), -1, np.int32)
    for r in range(R):
        best = np.zeros(D, np.float32)
        have = np.zeros(D, bool)
        kept = np.zeros(D, np.int64)
        win = np.full(D, -1, np.int64)
        for e in range(rp[r], rp[r + 1]):
            js, vs = cand[col[e]]
            b = best[js]
            with np.errstate(invalid="ignore"):
                take = ~have[js] | (~np.isnan(b) & (np.isnan(vs) | (vs > b)))
            jt = js[take]
            best[jt] = vs[take]
            win[jt] = e
            have[js] = True
            kept[js] += 1
        deg = rp[r + 1] - rp[r]
        with np.errstate(invalid="ignore"):
            implicit = ~have | ((kept < deg) & (0 > best))  # 0 > NaN is false: the NaN stays
        out[r] = np.where(implicit, np.float32(0.0), best)
        arg[r] = np.where(implicit, -1, win)
    return out, arg


def backward(rp, col, ci, arg, G, C=None):
    """Backward(grad float64 [C, k], bound, n) from the forward's arg and the gradient of out."""
    C = ci.shape[0] if C is None else C
    k = ci.shape[1]
    D = G.shape[1]
    G64 = G.astype(np.float64)
    Gabs = np.where(np.isfinite(G64), np.abs(G64), 0.0)
    grad = np.zeros((C, k))
    s_abs = np.zeros((C, k))
    n = np.zeros((C, k))
    sel = ci.astype(np.int64)
    ok = sel < D
    selc = np.where(ok, sel, 0)
    for r in range(rp.size - 1):
        for e in range(rp[r], rp[r + 1]):
            c = col[e]
            hit = ok[c] & (arg[r, selc[c]] == e)
            ls = np.flatnonzero(hit)
            js = selc[c, ls]
            grad[c, ls] += G64[r, js]
            s_abs[c, ls] += Gabs[r, js]
            n[c, ls] += 1
    return Backward(grad, N._bound(n, s_abs, 0.0), n)


def outcomes(rp, col, cv, ci, D, out, arg):
    """How many (r, j) end as: an explicit positive winner; the implicit zero beating a negative
    best; an explicit negative winner in a row where every edge keeps j."""
    deg = np.diff(rp)
    kept = np.zeros(out.shape, np.int64)
    cand = folded(np.asarray(cv, np.float32), ci, D)
    for r in range(rp.size - 1):
        for e in range(rp[r], rp[r + 1]):
            kept[r, cand[col[e]][0]] += 1
    pos = int(((arg >= 0) & (out > 0)).sum())
    imp = int(((arg < 0) & (kept > 0)).sum())  # candidates, all of them below the implicit zero
    neg = int(((arg >= 0) & (out < 0) & (kept == deg[:, None])).sum())
    return pos, imp, neg
