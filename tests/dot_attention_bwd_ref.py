"""Expected values and bounds of the fused backward of the multi-head dot-product attention on CBSR
keys (dot_attention_heads_bwd.hip), in plain numpy float64, built on dot_attention_ref (the forward
and its alpha), edge_grad_ref (ga) and edge_softmax_ref (the row reductions).  Edge e lies in CSR
row r, c = col[e], s = ci[c, l]:

    alpha_he = dot_attention_ref's w                 ga_he = sum_l cv[c, l] G[h, r, s]
    t_hr     = sum_j out[h, r, j] G[h, r, j]  over the columns j with an addend
    gl_he    = alpha_he (ga_he - t_hr)
    g_q[h, r, j]  = scale sum_{e in r} gl_he x_c[j]       x_c the scattered CBSR row
    g_cbsr[c, l]  = sum_h sum_{e -> c} (alpha_he G[h, r, s] + scale gl_he q[h, r, s])

t is formed from the exact float64 out of the reference; sum_j out_j G_j = sum_e alpha_e ga_e
holds exactly (test_dot_attention_bwd_cpu.py pins it), so gl is the edge softmax's backward.  A
column without an addend is left out, as the kernel leaves out the columns where its `out` is 0:
a NaN or Inf of G there reaches nothing.  q enters only through the selected columns (the logits
of dot_attention_ref and the products gl q above), so a NaN of q at a column no neighbour of the
row selects reaches nothing.  Inf and NaN otherwise follow IEEE through numpy.

Bounds, u = 2^-24.  The kernel computes each factor once, so each carries its own entry's bound:

alpha   d_alpha = Dot.w_bound: the coefficient is rebuilt from the row statistics and the logit
        of the forward's own device functions, exactly as maxk_dot_edge_alpha_heads rebuilds it.
ga      d_ga = edge_grad_ref.bound: the same products and the same butterfly as
        maxk_edge_weight_grad_heads.
t       d_t = (n_t + 8) u sum_j |out_j G_j| + sum_j out_err_j |G_j|, n_t the number of the row's
        columns with an addend: n_t fused products summed by a lane loop and a 64-lane
        butterfly, plus the error of the `out` the kernel is given, carried through G.  out_err
        is the caller's: u |out| for the reference rounded to fp32 (rounded_out_err), Dot's
        out_bound for the kernel's own forward.
gl      the product bound of gat_attention_bwd_ref without the slope factor.  With x = ga - t:
        d_x = d_ga + d_t + u |x| (the subtraction); gl = alpha x:
        d_gl = d_alpha |x| + (|alpha| + d_alpha) d_x + u |gl|.
g_q     scale ((n + 9) (u sum |gl v| + 2^-149) + sum d_gl |v|), n the element's number of addends
        (numerics.count_fwd): the forward sum's (n + 8) rule on the products gl v, d_gl carried
        through |v|, and one more rounding for the product by scale -- taken per addend, since a
        cut row's pieces are scaled before they are added.  An element without addends is
        exactly 0.
g_cbsr  (n + 8) (u S + 2^-149) + u S_q + sum d_alpha |G| + sum d_gl |scale q|, n = 2 H times the
        in-degree (a product and one fma per further term in head order, then the CSC sum),
        S = sum |alpha G| + sum |scale gl q|, S_q = sum |scale gl q| the one extra rounding of the
        staged scale * q (none for a power of two).  0 where the selector is >= D or the column
        is unread.

The one place where this differs from the stored path: there t is the sum over the row's edges of
alpha ga, so a row of a single edge has ga - t = 0 exactly; here ga and t are the same number
summed in two orders, and such a row's gl is within d_gl of 0, not 0.

These constants are derived, not measured.  tests/test_dot_attention_bwd_cpu.py pins the formulas
against float64 torch autograd of the dense composition."""
from collections import namedtuple

import numpy as np

import dot_attention_ref as DR
import edge_grad_ref as R
import edge_softmax_ref as ER

U = DR.U
FLOOR = DR.FLOOR

Bwd = namedtuple("Bwd", "ga ga_bound t t_bound gl gl_bound g_q g_q_bound parts shared")
# the per-head parts of g_cbsr, which sums the heads: cbsr(b, H) adds the first H
Parts = namedtuple("Parts", "ref s_abs s_q carried cnt")


def _fabs(a):
    return np.where(np.isfinite(a), np.abs(a), 0.0)


def rounded_out_err(a):
    """out_err of the reference out rounded to fp32."""
    return U * _fabs(a.out)


def edge_grads(g, cv, ci, G):
    """edge_grad_ref of every head's G: the part of backward() that does not depend on q or on
    out_err, for callers that ask for several references of one G."""
    return [R.edge_grad_ref(g.rp, g.col, cv, ci, G[h], None) for h in range(G.shape[0])]


def _dense(rows, col, w, shape):
    """The [R, C] matrix of the finite per-edge numbers w >= 0 (parallel edges added): what a
    bound is carried through, so that a sum over a row's or a column's edges is a matmul."""
    return np.bincount(rows * shape[1] + col, w, minlength=shape[0] * shape[1]).reshape(shape)


def _shared(g, q, scale, cv, ci, G, D, a, ers):
    """What does not depend on out_err: the values, in the order of the formulas with every
    product formed per edge and slot (so Inf and NaN reach exactly the elements they are added
    to), and the sums of magnitudes of the bounds, formed as dense matmuls of finite numbers."""
    rp, col = g.rp, g.col.astype(np.int64)
    H = a.w.shape[0]
    C, k = ci.shape
    R_ = rp.size - 1
    rows = ER.edge_rows(rp).astype(np.int64)
    sc = np.float64(np.float32(scale))
    G64 = np.asarray(G[:H], np.float64)
    q64 = sc * np.asarray(q[:H], np.float64)
    sel = ci[col].astype(np.int64)                          # [E, k]
    ok = sel < D
    keep = ok.ravel()
    gidx = rows[:, None] * D + np.minimum(sel, D - 1)       # [E, k] into a flat [R, D]
    qidx = gidx.ravel()[keep]
    order = np.argsort(col, kind="stable")                  # the CSC order of the edges
    cptr = np.searchsorted(col[order], np.arange(C))
    indeg = np.bincount(col, minlength=C)
    with np.errstate(invalid="ignore"):
        v = cv[col].astype(np.float64)                      # [E, k]
        cv64 = cv.astype(np.float64)
    okc = ci.astype(np.int64) < D
    selcc = np.minimum(ci.astype(np.int64), D - 1)
    Xabs = np.zeros((C, D))                                 # sum |value| per column and selector
    np.add.at(Xabs, (np.arange(C)[:, None].repeat(k, 1)[okc], selcc[okc]), _fabs(cv64)[okc])
    cnt = np.where(okc, indeg[:, None], 0).astype(np.float64)

    def by_col(x):                                          # [E, k] -> [C, k]: the CSC sum
        out = np.zeros((C, k))
        live = indeg > 0
        out[live] = np.add.reduceat(x[order], cptr[live], axis=0)
        return out

    def at_sel(M):                                          # [C, D] -> [C, k] at the selectors
        return np.where(okc, M[np.arange(C)[:, None], selcc], 0.0)

    sh = dict(rows=rows, col=col, shape=(R_, C), Xabs=Xabs, at_sel=at_sel, cnt=cnt, sc=sc,
              absG=_fabs(G64), absq=_fabs(q64), heads=[])
    for h in range(H):
        er = ers[h]
        ga, d_ga = er.ref, R.bound(er)
        w, d_w = a.w[h], a.w_bound[h]
        has = a.out_bound[h] > 0                            # the columns with an addend
        with np.errstate(invalid="ignore", over="ignore"):
            og = np.where(has, a.out[h] * G64[h], 0.0)
            t = og.sum(1)
            n_t = has.sum(1).astype(np.float64)
            d_t0 = (n_t + 8) * U * _fabs(og).sum(1)
            x = ga - t[rows]
            gl = w * x
            gq = sc * np.bincount(qidx, (gl[:, None] * v).ravel()[keep],
                                  minlength=R_ * D).reshape(R_, D)
            Gs = np.where(ok, G64[h].ravel().take(gidx), 0.0)
            Qs = np.where(ok, q64[h].ravel().take(gidx), 0.0)
            ref = by_col(w[:, None] * Gs + gl[:, None] * Qs)
        A_gl = _dense(rows, col, _fabs(gl), (R_, C))
        s_q = at_sel(A_gl.T @ sh["absq"][h])
        sh["heads"].append(dict(
            ga=ga, d_ga=d_ga, w=w, d_w=d_w, has=has, t=t, d_t0=d_t0, x=x, gl=gl, gq=gq, ref=ref,
            gq_abs=A_gl @ Xabs, s_q=s_q,
            s_abs=at_sel(_dense(rows, col, _fabs(w), (R_, C)).T @ sh["absG"][h]) + s_q,
            carried_w=at_sel(_dense(rows, col, _fabs(d_w), (R_, C)).T @ sh["absG"][h])))
    return sh


def backward(g, a, q, scale, cv, ci, G, D, out_err, counts, ers=None, base=None):
    """g: the graph (rp, col, C), a: dot_attention_ref.Dot of H heads of q [H, R, D] (fp32) at
    `scale`, (cv, ci) the CBSR, G [H, R, D] fp32 the gradient of out, out_err [H, R, D] the bound
    of the `out` the kernel is given against a.out, counts [R, D] numerics.count_fwd.  ers:
    edge_grads(g, cv, ci, G), when the caller has them; base: a Bwd of the same arguments and
    another out_err, whose values are taken over."""
    H = a.w.shape[0]
    ers = edge_grads(g, cv, ci, G[:H]) if ers is None else ers
    sh = base.shared if base is not None else _shared(g, q, scale, cv, ci, G, D, a, ers)
    rows, col, shape, sc = sh["rows"], sh["col"], sh["shape"], sh["sc"]
    n = np.rint(np.asarray(counts, np.float64))
    res = {f: [] for f in Bwd._fields[:8]}
    parts = []
    for h in range(H):
        p = sh["heads"][h]
        with np.errstate(invalid="ignore", over="ignore"):
            d_t = p["d_t0"] + np.where(p["has"], out_err[h] * sh["absG"][h], 0.0).sum(1)
            d_x = p["d_ga"] + d_t[rows] + U * _fabs(p["x"])
            d_gl = (p["d_w"] * _fabs(p["x"]) + (_fabs(p["w"]) + p["d_w"]) * d_x
                    + U * _fabs(p["gl"]))
        A_d = _dense(rows, col, _fabs(d_gl), shape)
        gq_bound = np.where(n > 0, sc * ((n + 9) * (U * p["gq_abs"] + FLOOR)
                                         + A_d @ sh["Xabs"]), 0.0)
        parts.append(Parts(p["ref"], p["s_abs"], p["s_q"],
                           p["carried_w"] + sh["at_sel"](A_d.T @ sh["absq"][h]), sh["cnt"]))
        for f, val in zip(Bwd._fields[:8],
                          (p["ga"], p["d_ga"], p["t"], d_t, p["gl"], d_gl, p["gq"], gq_bound)):
            res[f].append(val)
    return Bwd(*(np.stack(res[f]) for f in Bwd._fields[:8]), parts, sh)


def cbsr(b, H):
    """(g_cbsr [C, k], its bound) of the first H heads of a Bwd."""
    ps = b.parts[:H]
    with np.errstate(invalid="ignore", over="ignore"):
        ref = sum(p.ref for p in ps)
        s_abs = sum(p.s_abs for p in ps)
        s_q = sum(p.s_q for p in ps)
        carried = sum(p.carried for p in ps)
    n = 2 * H * ps[0].cnt
    bound = np.where(n > 0, (n + 8) * (U * s_abs + FLOOR) + U * s_q + carried, 0.0)
    return np.where(n > 0, ref, 0.0), bound
