"""Expected values and bounds of the edge softmax, in plain numpy float64 (a helper, like
tests/edge_grad_ref.py).  Edge e lies in CSR row r, c = col[e]:

    z_e = s_dst[r] + s_src[c]            l_e = z_e > 0 ? z_e : slope * z_e      (GAT form)
    w_e = exp(l_e - m_r) / sum_{j in r} exp(l_j - m_r)       m_r = max_{j in r} l_j
    t_r  = sum_{e in r} w_e gw_e         gl_e = w_e (gw_e - t_r)
    gz_e = gl_e (z_e > 0 ? 1 : slope)    grad_s_dst[r] = sum_{e in r} gz_e
                                         grad_s_src[c] = sum_{e: col[e] = c} gz_e

Inf and NaN follow IEEE through numpy (np.maximum.reduceat propagates NaN, so a row with a NaN
logit is all NaN either way; exp(-inf) = 0; -inf - -inf = NaN).

Bounds, with u = 2^-24, n_r the degree of row r and A_r = max_e |z_e| (plain: max_e |logit_e|)
over the row's finite values:

forward   |w - ref| <= (n_r + 16 + 16 A_r) u ref + (n_r + 16) 2^-149
          -- three roundings of the exponent's argument (the fp32 score sum, the slope product,
          the subtraction of the max), each at most 2 A_r u absolute, act on numerator and
          denominator; exp is good to a few ulp; the sum has n_r terms; one division; the floor
          covers weights that underflow.
gl        (n_r + 8) u |w_e| (|gw_e| + sum_j |w_j gw_j|), evaluated with the reference w, plus
          the forward bound of w carried through: dw_e (|gw_e| + |t_r|) + |w_e| sum_j dw_j |gw_j|.
scores    (n + 8) u sum|terms| on top of the sum of the terms' own bounds, n the number of
          addends; an element without addends is exactly 0 (bound 0).

These constants are derived, not measured.  tests/test_edge_softmax_cpu.py pins the formulas
against torch autograd of the PyTorch composition in float64.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -149

Fwd = namedtuple("Fwd", "w bound z l rows deg A")
Bwd = namedtuple("Bwd", "gl gl_bound gz gz_bound g_dst g_dst_bound g_src g_src_bound")


def edge_rows(rp):
    return np.repeat(np.arange(rp.size - 1), np.diff(rp))


def _row_reduce(f, x, rp, empty):
    """f.reduceat over the CSR rows, `empty` for a row without edges."""
    R = rp.size - 1
    out = np.full(R, empty, np.float64)
    has = np.diff(rp) > 0
    if x.size and has.any():
        starts = rp[:-1][has].astype(np.int64)
        out[has] = f.reduceat(x, starts)
    return out


def _finite_abs(a):
    return np.where(np.isfinite(a), np.abs(a), 0.0)


def gat_logits(rp, col, s_dst, s_src, slope):
    rows = edge_rows(rp)
    with np.errstate(invalid="ignore"):
        z = s_dst.astype(np.float64)[rows] + s_src.astype(np.float64)[col]
        l = np.where(z > 0, z, np.float64(slope) * z)
    return z, l


def forward(rp, l, z=None):
    """Fwd of logits l [E] (float64; z: the GAT pre-activations, for A_r and the backward)."""
    rows = edge_rows(rp)
    deg = np.diff(rp).astype(np.float64)
    l = np.asarray(l, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = _row_reduce(np.maximum, l, rp, 0.0)
        p = np.exp(l - m[rows])
        s = _row_reduce(np.add, p, rp, 1.0)
        w = p / s[rows]
    A = _row_reduce(np.maximum, _finite_abs(l if z is None else z), rp, 0.0)
    n = deg[rows]
    bound = (n + 16 + 16 * A[rows]) * U * np.where(np.isfinite(w), w, 0.0) + (n + 16) * FLOOR
    return Fwd(w, bound, z, l, rows, deg, A)


def gat_forward(rp, col, s_dst, s_src, slope):
    z, l = gat_logits(rp, col, s_dst, s_src, slope)
    return forward(rp, l, z)


def _sum_bound(n, s_abs, term_bounds):
    """(n + 8) u sum|terms| + the terms' own bounds; 0 where n = 0."""
    return np.where(n > 0, (n + 8) * U * s_abs + term_bounds, 0.0)


def backward(rp, col, f, gw, slope=None, num_cols=None, gw_bound=None):
    """Bwd of a Fwd and the gradient of w; slope None: the plain form (gl only).  gw_bound: the
    bound of a gw that is itself computed (the edge-weight gradient's), carried through
    gl = w (gw - t): w_e (dgw_e + sum_j w_j dgw_j)."""
    rows, deg = f.rows, f.deg
    gw = np.asarray(gw, np.float64)
    n = deg[rows]
    with np.errstate(invalid="ignore", over="ignore"):
        wg = f.w * gw
        t = _row_reduce(np.add, wg, rp, 0.0)
        gl = f.w * (gw - t[rows])
        s_wg = _row_reduce(np.add, _finite_abs(wg), rp, 0.0)
        wf = _finite_abs(f.w)
        carried = (f.bound * (np.abs(gw) + np.abs(t[rows]))
                   + wf * _row_reduce(np.add, f.bound * np.abs(gw), rp, 0.0)[rows])
        if gw_bound is not None:
            carried = carried + wf * (gw_bound + _row_reduce(np.add, wf * gw_bound, rp, 0.0)[rows])
        gl_bound = (n + 8) * U * wf * (np.abs(gw) + s_wg[rows]) + carried
    if slope is None:
        return Bwd(gl, gl_bound, None, None, None, None, None, None)
    C = int(num_cols)
    with np.errstate(invalid="ignore"):
        fac = np.where(f.z > 0, 1.0, np.float64(slope))
        gz = gl * fac
        gz_bound = gl_bound * fac + U * _finite_abs(gz)  # the product's own rounding
        g_dst = _row_reduce(np.add, gz, rp, 0.0)
        g_dst_bound = _sum_bound(deg, _row_reduce(np.add, _finite_abs(gz), rp, 0.0),
                                 _row_reduce(np.add, gz_bound, rp, 0.0))
        g_src = np.zeros(C, np.float64)
        np.add.at(g_src, col, gz)
        cnt = np.bincount(col, minlength=C).astype(np.float64)
        g_src_bound = _sum_bound(cnt, np.bincount(col, _finite_abs(gz), minlength=C),
                                 np.bincount(col, gz_bound, minlength=C))
    return Bwd(gl, gl_bound, gz, gz_bound, g_dst, g_dst_bound, g_src, g_src_bound)


def row_sum_bound(f):
    """|sum_{e in r} w_e - 1| is within the sum of the row's forward bounds (the reference sums
    to 1 up to float64 rounding); rows without edges are left out by the caller."""
    return _row_reduce(np.add, f.bound, _rp_of(f), 0.0)


def _rp_of(f):
    rp = np.zeros(f.deg.size + 1, np.int64)
    np.cumsum(f.deg.astype(np.int64), out=rp[1:])
    return rp


def as_f32(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a).astype(np.float32)
