"""Expected values and bounds of the fused multi-head GAT attention backward
(gat_attention_heads_bwd.hip), in plain numpy float64, built on gat_attention_ref (the forward and
its alpha), edge_softmax_ref (the score sums) and edge_grad_ref (ga).  Edge e lies in CSR row r,
c = col[e]:

    alpha_he = gat_attention_ref's w                 ga_he = sum_l cv[c, l] G[h, r, ci[c, l]]
    t_hr     = sum_j out[h, r, j] G[h, r, j]  over the columns j with an addend
    gz_he    = alpha_he (ga_he - t_hr) (z_he > 0 ? 1 : slope)
    g_dst[h, r] = sum_{e in r} gz_he                 g_src[h, c] = sum_{e: col = c} gz_he
    g_cbsr[c, l] = sum_h sum_{e -> c} alpha_he G[h, r, ci[c, l]]

t is formed from the exact float64 out of the reference; sum_j out_j G_j = sum_e alpha_e ga_e
holds exactly (test_gat_attention_bwd_cpu.py pins it), so this is the edge softmax's backward.
A column without an addend is left out, as the kernel leaves out the columns where its `out`
is 0: a NaN or Inf of G there reaches nothing.  Inf and NaN otherwise follow IEEE through numpy.

Bounds, u = 2^-24.  The kernel computes each factor once, so each carries its own entry's bound:

alpha   d_alpha = edge_softmax_ref's forward bound (f.bound): the coefficient is rebuilt from
        the row statistics exactly as maxk_gat_edge_alpha_heads rebuilds it.
ga      d_ga = edge_grad_ref.bound: the same products and the same butterfly as
        maxk_edge_weight_grad_heads.
t       d_t = (n_t + 8) u sum_j |out_j G_j| + sum_j out_err_j |G_j|, n_t the number of the row's
        columns with an addend: n_t fused products summed by a lane loop and a 64-lane
        butterfly (at most n_t + 6 roundings on any path, inside n_t + 8), plus the error of
        the `out` the kernel is given, carried through G.  out_err is the caller's: u |out| for
        the reference rounded to fp32, gat_attention_ref's out_bound for the kernel's own
        forward.
gz      the product bound.  With x = ga - t: d_x = d_ga + d_t + u |x| (the subtraction);
        gl = alpha x: d_gl = d_alpha |x| + (|alpha| + d_alpha) d_x + u |gl|;
        gz = gl fac: d_gz = fac d_gl + u |gz|.  The sign of the fp32 score sum is the sign of
        the exact one (rounding is monotone and keeps 0), so fac is exact.
scores  edge_softmax_ref._sum_bound: (n + 8) u sum |gz| + sum d_gz, n the row's degree or the
        column's in-degree; an element without addends is exactly 0.
g_cbsr  feat_grad_ref of tests/test_gat_attention_gpu.py: (n + 8) u sum |alpha G| with
        n = H times the in-degree (one product and one fma per further head, then the CSC sum),
        plus d_alpha carried through |G|; 0 where the selector is >= D or the column is unread.

The one place where this differs from the stored path's reference (edge_softmax_ref.backward):
there t is the sum over the row's edges of w gw, so a row of a single edge has gw - t = 0
exactly; here ga and t are the same number summed in two orders, and such a row's gz is within
d_gz of 0, not 0.

These constants are derived, not measured.  tests/test_gat_attention_bwd_cpu.py pins the
formulas against float64 torch autograd of the dense composition."""
from collections import namedtuple

import numpy as np

import edge_grad_ref as R
import edge_softmax_ref as ER
import gat_attention_ref as AR

U = AR.U

Bwd = namedtuple("Bwd", "ga ga_bound t t_bound gz gz_bound g_dst g_dst_bound g_src g_src_bound "
                        "g_cbsr g_cbsr_bound")


def _fabs(a):
    return np.where(np.isfinite(a), np.abs(a), 0.0)


def rounded_out_err(a):
    """out_err of the reference out rounded to fp32."""
    return U * _fabs(a.out)


def edge_grads(g, cv, ci, G):
    """edge_grad_ref of every head's G: the part of backward() that does not depend on the
    scores or on out_err, for callers that ask for several references of one G."""
    return [R.edge_grad_ref(g.rp, g.col, cv, ci, G[h], None) for h in range(G.shape[0])]


def backward(g, a, cv, ci, G, slope, D, out_err, feat_grad_ref=None, ers=None):
    """g: the graph (rp, col, C), a: gat_attention_ref.Attn of H heads, (cv, ci) the CBSR,
    G [H, R, D] fp32 the gradient of out, out_err [H, R, D] the bound of the `out` the kernel is
    given against a.out.  feat_grad_ref: tests/test_gat_attention_gpu.py's (None: g_cbsr and
    its bound are left None).  ers: edge_grads(g, cv, ci, G), when the caller has them."""
    rp, col = g.rp, g.col
    H = len(a.heads)
    ers = edge_grads(g, cv, ci, G[:H]) if ers is None else ers
    rows = ER.edge_rows(rp)
    deg = np.diff(rp).astype(np.float64)
    cnt = np.bincount(col, minlength=g.C).astype(np.float64)
    G64 = np.asarray(G, np.float64)
    res = {k: [] for k in Bwd._fields[:10]}
    for h in range(H):
        f = a.heads[h]
        er = ers[h]
        ga, d_ga = er.ref, R.bound(er)
        has = a.out_bound[h] > 0                        # the columns with an addend
        with np.errstate(invalid="ignore", over="ignore"):
            og = np.where(has, a.out[h] * G64[h], 0.0)
            t = og.sum(1)
            n_t = has.sum(1).astype(np.float64)
            d_t = ((n_t + 8) * U * _fabs(og).sum(1)
                   + np.where(has, out_err[h] * _fabs(G64[h]), 0.0).sum(1))
            x = ga - t[rows]
            d_x = d_ga + d_t[rows] + U * _fabs(x)
            wf = _fabs(f.w)
            gl = f.w * x
            d_gl = f.bound * _fabs(x) + (wf + f.bound) * d_x + U * _fabs(gl)
            fac = np.where(f.z > 0, 1.0, np.float64(slope))
            gz = gl * fac
            d_gz = fac * d_gl + U * _fabs(gz)
            g_dst = ER._row_reduce(np.add, gz, rp, 0.0)
            g_dst_bound = ER._sum_bound(deg, ER._row_reduce(np.add, _fabs(gz), rp, 0.0),
                                        ER._row_reduce(np.add, d_gz, rp, 0.0))
            g_src = np.zeros(g.C, np.float64)
            np.add.at(g_src, col, gz)
            g_src_bound = ER._sum_bound(cnt, np.bincount(col, _fabs(gz), minlength=g.C),
                                        np.bincount(col, d_gz, minlength=g.C))
        for k, v in zip(Bwd._fields[:10], (ga, d_ga, t, d_t, gz, d_gz, g_dst, g_dst_bound, g_src,
                                           g_src_bound)):
            res[k].append(v)
    gc = gcb = None
    if feat_grad_ref is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            gc, gcb = feat_grad_ref(g, a, G, ci, D)
    return Bwd(*(np.stack(res[k]) for k in Bwd._fields[:10]), gc, gcb)
