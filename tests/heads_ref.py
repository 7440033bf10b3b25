"""Expected values of the multi-head aggregation, in plain numpy (a helper, like
tests/numerics.py and tests/edge_grad_ref.py, which it applies per head).

Layout, head-major as the kernels take it: weights w [H, E], outputs and their gradients
[H, R, D], edge gradients [H, E].

    out[h]       = fwd(A with weights w[h]) . scatter(cbsr) / div           numerics.fwd_ref
    grad_edge[h] = edge_grad_ref(..., G[h], div)                              edge_grad_ref
    grad_cbsr    = sum_h bwd(A with weights w[h], G[h])                       numerics.bwd_ref

Bounds are numerics' own rule, (n + 8) * (2^-24 * S_abs + unit), per head for the first two;
the sum over heads has the addends of every head, n = sum_h n_h and S_abs = sum_h S_abs_h.

test_heads_cpu.py pins all three against torch autograd on a dense float64 restatement.
"""
import numpy as np

import edge_grad_ref as R
import numerics as N


def head_graph(g, w_h, div=True):
    """Graph g with head h's weights (and no divisor when div is False)."""
    return g._replace(ev=np.ascontiguousarray(w_h, np.float32), div=g.div if div else None)


def fwd_heads_ref(g, w, cv, ci, D, div=True):
    """[H, R, D] fp32: the oracle's forward per head."""
    return np.stack([N.fwd_ref(head_graph(g, w[h], div), cv, ci, D) for h in range(w.shape[0])])


def bound_fwd_heads(g, w, cv, ci, D, div=True, unit=0.0):
    n = N.count_fwd(g, ci, D)  # the addends do not depend on the weights
    return np.stack([N.bound_fwd(head_graph(g, w[h], div), cv, ci, D, unit=unit, n=n)
                     for h in range(w.shape[0])])


def edge_grad_heads_ref(g, cv, ci, G, div=True):
    """EdgeRef with [H, E] members: edge_grad_ref per head of G [H, R, D]."""
    ers = [R.edge_grad_ref(g.rp, g.col, cv, ci, G[h], g.div if div else None)
           for h in range(G.shape[0])]
    return R.EdgeRef(*(np.stack([getattr(e, f) for e in ers]) for f in R.EdgeRef._fields))


def bound_edge_heads(er, unit=0.0):
    return R.bound(er, unit)


def heads_slice(er, H):
    """The first H heads of an EdgeRef."""
    return R.EdgeRef(*(a[:H] for a in er))


def feat_grad_heads_ref(g, w, G, ci, div=True):
    """[C, k] float64: the feature (CBSR value) gradient, the per-head oracle backwards summed
    in double."""
    return sum(N.bwd_ref(head_graph(g, w[h], div), G[h], ci).astype(np.float64)
               for h in range(w.shape[0]))


def bound_feat_grad_heads(g, w, G, ci, div=True, unit=0.0):
    """n = sum_h n_h (H times the count of one head), S_abs = sum_h S_abs_h."""
    H = w.shape[0]
    n = H * N.count_bwd(g, ci, G.shape[2]).astype(np.float64)
    s = np.zeros(ci.shape, np.float64)
    for h in range(H):
        gh = head_graph(g, w[h], div)
        s += N.O.sspmm_bwd(gh.rp, gh.col, gh.ev, N._pad(N._finite_abs(G[h])), ci,
                           row_div=gh.div).astype(np.float64)
    return N._bound(n, s, unit)
