"""Expected values and bounds of the attention dropout inside the fused dot-product attention (the
dropout entries of dot_attention_heads.hip / dot_attention_heads_bwd.hip), in plain numpy float64,
built on attn_dropout_ref (the mask d and the float32 scale), dot_attention_ref (the undropped
attention, its alpha and statistics) and dot_attention_bwd_ref (ga, the dense sums of the bounds,
the per-head parts of g_cbsr).  Edge e lies in CSR row r, c = col[e], s = ci[c, l]:

    out[h, r, s] += alpha_he d_he cv[c, l]                 m, z: those of the undropped softmax
    ga_he = sum_l cv[c, l] G[h, r, s]
    t_hr  = sum_j out[h, r, j] G[h, r, j]  over the columns j where the dropped out is not 0
    gl_he = alpha_he (d_he ga_he - t_hr)
    g_q[h, r, j]  = scale sum_{e in r} gl_he x_c[j]
    g_cbsr[c, l]  = sum_h sum_{e -> c} (alpha_he d_he G[h, r, s] + scale gl_he q[h, r, s])

sum_j out_j G_j = sum_e alpha_e d_e ga_e holds exactly for the dropped out
(test_dot_attn_dropout_cpu.py pins it), so gl is the gradient of the logits through the dropout
and the softmax.  t leaves out the columns where the reference's dropped out is exactly 0 -- the
kernel's rule: a column without an addend and, for finite inputs, one all of whose addends are
dropped -- so a NaN or Inf of G there reaches nothing.  Inf and NaN otherwise follow IEEE through
numpy with d as a factor: 0 * NaN and 0 * Inf are NaN, dropping does not shield.

Bounds, u = 2^-24; each is the bound of the entry without dropout carried through the factor d
(0 or scale, exact), plus the roundings the factor adds:

coef    alpha d: d * d_alpha + u |alpha d|, the one product by scale (Dot.w_bound of the dropped
        Dot).  The forward kernel never forms it: it sums p * (0 or 1) * value as without dropout
        and multiplies the row by scale after the division, one rounding of the sum.
out     (n + 8) (u S + scale 2^-149) + sum_e d_e d_alpha_e |v_e| + u S, S = sum_e |alpha_e d_e v_e|:
        dot_attention_ref's out bound on the dropped terms (a dropped edge's exact 0 product still
        counts among the n addends: it rounds nothing), its subnormal floor scaled with the row,
        and u S for the product by scale.  An element without addends is exactly 0, and so is, for
        finite inputs, an element all of whose addends are dropped (S = 0 and the carried bound is
        0 where d is 0; the floor term bounds an error that is 0).
x       d ga - t: d_x = d * d_ga + u |d ga| (the product) + d_t + u |x| (the subtraction);
        d_t = (n_t + 8) u sum_j |out_j G_j| + sum_j out_err_j |G_j| is dot_attention_bwd_ref's with
        the dropped out and its out_err, n_t and the carried sum over the columns with an addend
        (a superset of the columns summed: where the reference is exactly 0 and the kernel's out
        is not, its term is within out_err |G|).
gl      alpha x, alpha the undropped coefficient: d_gl = d_alpha |x| + (|alpha| + d_alpha) d_x
        + u |gl|, dot_attention_bwd_ref's product rule on that x.
g_q     scale ((n + 9) (u sum |gl v| + 2^-149) + sum d_gl |v|), as there.
g_cbsr  (n + 8) (u S + 2^-149) + u S_q + sum d_coef |G| + sum d_gl |scale q|, as there with coef
        in the place of alpha: S = sum |alpha d G| + sum |scale gl q|.
stored  the rebuilt backward runs the stored passes on gw = d ga (bound d * d_ga + u |d ga|) and
        the feature gradient on the masked alpha (coef): rebuilt_bounds.

These constants are derived, not measured.  tests/test_dot_attn_dropout_cpu.py pins the formulas
against float64 torch autograd of the dense composition that multiplies the same d in."""
import types

import numpy as np

import attn_dropout_ref as AD
import dot_attention_bwd_ref as DB
import dot_attention_ref as DA
import edge_grad_ref as R
import edge_softmax_ref as ER

U = DA.U
FLOOR = DA.FLOOR
mask = AD.mask
scale = AD.scale
_fabs = DB._fabs


def drop_attention(a, d, rp, col, cv, ci, D, counts):
    """a: the dot_attention_ref.Dot of the undropped attention, d [H, E] the mask -> the Dot of the
    dropped one: out and its bound, m, z, l and heads as they were, w = alpha d with coef's
    bound."""
    H = a.w.shape[0]
    R_ = rp.size - 1
    rows = ER.edge_rows(rp)
    sel = ci[col].astype(np.int64)
    keep = (sel < D).ravel()
    idx = (rows[:, None].astype(np.int64) * D + sel).ravel()[keep]
    with np.errstate(invalid="ignore"):
        v = cv[col].astype(np.float64)
    av = _fabs(v)
    n = np.rint(np.asarray(counts, np.float64))
    sc = float(d.max()) if d.size else 1.0
    outs, bounds, ws, wbs = [], [], [], []
    for h in range(H):
        with np.errstate(invalid="ignore", over="ignore"):
            wd = a.w[h] * d[h]
            out = np.bincount(idx, (wd[:, None] * v).ravel()[keep],
                              minlength=R_ * D).reshape(R_, D)
            s_abs = np.bincount(idx, (_fabs(wd)[:, None] * av).ravel()[keep],
                                minlength=R_ * D).reshape(R_, D)
            carried = np.bincount(idx, ((a.w_bound[h] * d[h])[:, None] * av).ravel()[keep],
                                  minlength=R_ * D).reshape(R_, D)
        bounds.append(np.where(n > 0, (n + 8) * (U * s_abs + max(sc, 1.0) * FLOOR) + carried
                               + U * s_abs, 0.0))
        outs.append(out)
        ws.append(wd)
        wbs.append(a.w_bound[h] * d[h] + U * _fabs(wd))
    st = (lambda xs, shape: np.stack(xs) if xs else np.zeros(shape))
    E = col.size
    return a._replace(out=st(outs, (0, R_, D)), out_bound=st(bounds, (0, R_, D)),
                      w=st(ws, (0, E)), w_bound=st(wbs, (0, E)))


def attention(rp, col, q, scale_, cv, ci, D, counts, p, seed, base=None):
    """(the dropped Dot, the undropped Dot, d).  base: the undropped Dot where the caller has
    it."""
    a = DA.attention(rp, col, q, scale_, cv, ci, D, counts) if base is None else base
    d = mask(q.shape[0], col.size, p, seed)
    return drop_attention(a, d, rp, col, cv, ci, D, counts), a, d


def rounded_out_err(ad):
    """out_err of the dropped reference out rounded to fp32."""
    return U * _fabs(ad.out)


def backward(g, a, ad, d, q, scale_, cv, ci, G, D, out_err, counts, ers=None):
    """The fused backward under dropout.  g: the graph (rp, col, C), a: the undropped Dot of H
    heads of q [H, R, D] (fp32) at scale_, ad: the dropped one, d [H, E] the mask, G [H, R, D]
    fp32 the gradient of out, out_err [H, R, D] the bound of the dropped `out` the kernel is given
    against ad.out, counts [R, D] numerics.count_fwd -> dot_attention_bwd_ref.Bwd whose ga and
    ga_bound hold d ga; dot_attention_bwd_ref.cbsr(b, H) gives g_cbsr."""
    rp, col = g.rp, g.col.astype(np.int64)
    H = a.w.shape[0]
    ers = DB.edge_grads(g, cv, ci, G[:H]) if ers is None else ers
    C, k = ci.shape
    R_ = rp.size - 1
    shape = (R_, C)
    rows = ER.edge_rows(rp).astype(np.int64)
    sc = np.float64(np.float32(scale_))
    G64 = np.asarray(G[:H], np.float64)
    q64 = sc * np.asarray(q[:H], np.float64)
    absG, absq = _fabs(G64), _fabs(q64)
    sel = ci[col].astype(np.int64)
    ok = sel < D
    keep = ok.ravel()
    gidx = rows[:, None] * D + np.minimum(sel, D - 1)
    qidx = gidx.ravel()[keep]
    order = np.argsort(col, kind="stable")                  # the CSC order of the edges
    cptr = np.searchsorted(col[order], np.arange(C))
    indeg = np.bincount(col, minlength=C)
    with np.errstate(invalid="ignore"):
        v = cv[col].astype(np.float64)
        cv64 = cv.astype(np.float64)
    okc = ci.astype(np.int64) < D
    selcc = np.minimum(ci.astype(np.int64), D - 1)
    Xabs = np.zeros((C, D))
    np.add.at(Xabs, (np.arange(C)[:, None].repeat(k, 1)[okc], selcc[okc]), _fabs(cv64)[okc])
    cnt = np.where(okc, indeg[:, None], 0).astype(np.float64)
    n = np.rint(np.asarray(counts, np.float64))

    def by_col(x):
        out = np.zeros((C, k))
        live = indeg > 0
        out[live] = np.add.reduceat(x[order], cptr[live], axis=0)
        return out

    def at_sel(M):
        return np.where(okc, M[np.arange(C)[:, None], selcc], 0.0)

    res = {f: [] for f in DB.Bwd._fields[:8]}
    parts = []
    for h in range(H):
        ga, d_ga = ers[h].ref, R.bound(ers[h])
        w, d_w = a.w[h], a.w_bound[h]
        wd, d_wd = ad.w[h], ad.w_bound[h]
        with np.errstate(invalid="ignore", over="ignore"):
            summed = ad.out[h] != 0                         # the kernel's rule (a NaN is summed)
            has = ad.out_bound[h] > 0                       # the columns with an addend
            og = np.where(summed, ad.out[h] * G64[h], 0.0)
            t = og.sum(1)
            n_t = has.sum(1).astype(np.float64)
            d_t = ((n_t + 8) * U * _fabs(og).sum(1)
                   + np.where(has, out_err[h] * absG[h], 0.0).sum(1))
            dga = d[h] * ga
            d_dga = d[h] * d_ga + U * _fabs(dga)
            x = dga - t[rows]
            d_x = d_dga + d_t[rows] + U * _fabs(x)
            gl = w * x
            d_gl = d_w * _fabs(x) + (_fabs(w) + d_w) * d_x + U * _fabs(gl)
            gq = sc * np.bincount(qidx, (gl[:, None] * v).ravel()[keep],
                                  minlength=R_ * D).reshape(R_, D)
            Gs = np.where(ok, G64[h].ravel().take(gidx), 0.0)
            Qs = np.where(ok, q64[h].ravel().take(gidx), 0.0)
            ref = by_col(wd[:, None] * Gs + gl[:, None] * Qs)
        A_gl = DB._dense(rows, col, _fabs(gl), shape)
        A_d = DB._dense(rows, col, _fabs(d_gl), shape)
        gq_bound = np.where(n > 0, sc * ((n + 9) * (U * (A_gl @ Xabs) + FLOOR) + A_d @ Xabs), 0.0)
        s_q = at_sel(A_gl.T @ absq[h])
        parts.append(DB.Parts(
            ref, at_sel(DB._dense(rows, col, _fabs(wd), shape).T @ absG[h]) + s_q, s_q,
            at_sel(DB._dense(rows, col, _fabs(d_wd), shape).T @ absG[h])
            + at_sel(A_d.T @ absq[h]), cnt))
        for f, val in zip(DB.Bwd._fields[:8], (dga, d_dga, t, d_t, gl, d_gl, gq, gq_bound)):
            res[f].append(val)
    return DB.Bwd(*(np.stack(res[f]) for f in DB.Bwd._fields[:8]), parts, None)


def rebuilt_bounds(g, a, ad, d, q, scale_, ci, G, D, counts, ers, agg_ref, feat_grad_ref):
    """(bound of grad_q, bound of grad_cbsr) of the rebuilt sequence under dropout: the stored
    passes on gw = d ga with the undropped alpha (edge_softmax_ref.backward), that through the
    aggregation onto q with one rounding for the scale, and both feature gradients onto
    topk_values -- the first on the masked alpha (coef) -- with one rounding for the scale and one
    for the sum.  agg_ref(gl, gl_bound) and feat_grad_ref(weights, X) are the callers' references
    of the aggregation and of the feature gradient (test_dot_attention_gpu.agg_ref,
    test_gat_attention_gpu.feat_grad_ref on this graph)."""
    H = a.w.shape[0]
    s = float(np.float32(scale_))
    bs = []
    for h in range(H):
        with np.errstate(invalid="ignore", over="ignore"):
            gw = d[h] * ers[h].ref
            gwb = d[h] * R.bound(ers[h]) + U * _fabs(gw)
        bs.append(ER.backward(g.rp, g.col, a.heads[h]._replace(bound=a.w_bound[h]), gw,
                              gw_bound=gwb))
    gl = np.stack([b.gl for b in bs])
    gl_bound = np.stack([b.gl_bound for b in bs])
    gq = [agg_ref(gl[h], gl_bound[h]) for h in range(H)]
    gq_val = np.stack([x[0] for x in gq])
    gq_bound = s * np.stack([x[1] for x in gq]) + U * s * np.abs(gq_val)
    v1, b1 = feat_grad_ref(ad, G[:H])
    v2, b2 = feat_grad_ref(types.SimpleNamespace(w=gl, w_bound=gl_bound), q[:H])
    return gq_bound, b1 + s * b2 + 2 * U * (np.abs(v1) + s * np.abs(v2))
