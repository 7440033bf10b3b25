"""Expected values and bounds of the fused multi-head dot-product attention on CBSR keys
(dot_attention_heads.hip), in plain numpy float64.  Edge e lies in CSR row r, c = col[e]:

    l[h, e] = scale * sum_l cv[c, l] * q[h, r, ci[c, l]]            over the selectors below D
    m[h, r] = max_e l[h, e]        z[h, r] = sum_e exp(l[h, e] - m[h, r])   (the row statistics)
    alpha[h, e] = exp(l[h, e] - m[h, r]) / z[h, r]
    out[h, r, ci[c, l]] += alpha[h, e] * cv[c, l]

The logits are edge_grad_ref's float64 dot products with grad_out := q[h], times scale; the
softmax is edge_softmax_ref.forward on them; out and the statistics are formed as in
gat_attention_ref.  Inf and NaN follow IEEE through numpy: a NaN in q reaches a logit only through
a selected column (a column no neighbour selects is never multiplied), a NaN alpha makes every
element it is added to NaN and leaves the others alone, alpha = 0 (a -Inf logit) adds exactly 0.
The statistics take the maximum that ignores NaN, as fmaxf does; a row of nothing but -Inf has
m = -Inf and z = 0; a row without edges has m = z = 0 and out = 0.

Bounds, u = 2^-24, n_c the number of column c's selectors below D, n_r the row's degree,
A_r = max_e |l_e| over the row's finite values:

logit     d_e = (n_c + 8) (u scale sum_l |cv q| + 2^-149): the edge gradient's bound (numerics'
          rule, with the subnormal floor as its unit) times scale.  The kernel multiplies q by
          scale once per element when it stages the row (one rounding per term, none for a power
          of two), takes one fma per slot and a butterfly of at most six additions: at most
          n_c + 7 roundings per term.
weight    |alpha' - alpha| <= (n_r + 24 + 16 A_r) u alpha + expm1(2 d_r) alpha
          + (n_r + 16) 2^-149, d_r = max_e d_e over the row: the plain edge softmax's bound (the
          exponent's argument l - m is rounded once more, inside its 16 A_r u), the 8 u of a cut
          row's merge that gat_attention_ref derives, and the logits' absolute error carried
          through the exponent: exp(l + d) = exp(l) (1 + expm1(d)), once on the numerator (d_e)
          and once on the denominator (a weighted mean of the row's d_j, at most d_r).  The
          maximum's own error cancels between the two.
m         d_r: the maximum of values each within d_e.
z         (n_r + 24 + 16 A_r) u z + expm1(2 d_r) z: the weight bound's relative part on z
          (an error of l_j and one of m, each at most d_r, in every term's exponent).
out       (n + 8) (u sum_e |alpha_e v_e| + 2^-149) + sum_e dalpha_e |v_e|, n the element's
          number of addends (numerics.count_fwd): as gat_attention_ref.  An element without
          addends is exactly 0.
alpha     from the statistics, exp(l' - m') / z': the weight bound (m' and z' are the forward's
          own, so the shift cancels as above).

These constants are derived, not measured.  tests/test_dot_attention_cpu.py pins the formulas
against torch autograd of a dense float64 composition."""
from collections import namedtuple

import numpy as np

import edge_grad_ref as EG
import edge_softmax_ref as ER
import gat_attention_ref as AR

U = ER.U
FLOOR = ER.FLOOR

Dot = namedtuple("Dot", "out out_bound m m_bound z z_bound w w_bound l l_bound heads")


def logits(rp, col, q, scale, cv, ci):
    """(l [H, E] float64, d [H, E]) of q [H, R, D] (fp32) and the CBSR (cv, ci) [C, k]."""
    ls, ds = [], []
    sc = np.float64(np.float32(scale))
    for h in range(q.shape[0]):
        er = EG.edge_grad_ref(rp, col, cv, ci, q[h])
        with np.errstate(invalid="ignore", over="ignore"):
            ls.append(sc * er.ref)
            ds.append(np.where(er.n > 0, (er.n + 8) * (U * sc * er.s_abs + FLOOR), 0.0))
    E = col.size
    if not ls:
        return np.zeros((0, E)), np.zeros((0, E))
    return np.stack(ls), np.stack(ds)


def _row_max_of(d, rp):
    return ER._row_reduce(np.maximum, d, rp, 0.0)


def weight_bound(f, d_row, extra=8):
    """The weight bound above from a Fwd of edge_softmax_ref.forward and the row's logit bound
    d_row [R] (extra=0: without the cut-row merge, for the stored composition)."""
    wf = np.where(np.isfinite(f.w), f.w, 0.0)
    return f.bound + (extra * U + np.expm1(2 * d_row[f.rows])) * wf


def attention(rp, col, q, scale, cv, ci, D, counts, extra=8):
    """q [H, R, D] (fp32), scale, the CBSR (cv, ci) [C, k], counts [R, D] the number of addends
    per output element (numerics.count_fwd) -> Dot, everything stacked head-major."""
    H, R = q.shape[0], rp.size - 1
    l, d = logits(rp, col, q, scale, cv, ci)
    rows = ER.edge_rows(rp)
    sel = ci[col].astype(np.int64)                          # [E, k]
    keep = (sel < D).ravel()
    idx = (rows[:, None].astype(np.int64) * D + sel).ravel()[keep]
    with np.errstate(invalid="ignore"):
        v = cv[col].astype(np.float64)                      # [E, k]
    av = np.where(np.isfinite(v), np.abs(v), 0.0)
    n = np.rint(np.asarray(counts, np.float64))
    outs, bounds, ms, mbs, zs, zbs, ws, wbs, fs = [], [], [], [], [], [], [], [], []
    for h in range(H):
        f = ER.forward(rp, l[h])
        d_row = _row_max_of(d[h], rp)
        wb = weight_bound(f, d_row, extra)
        with np.errstate(invalid="ignore", over="ignore"):
            t = (f.w[:, None] * v).ravel()[keep]
            out = np.bincount(idx, t, minlength=R * D).reshape(R, D)
            wf = np.where(np.isfinite(f.w), f.w, 0.0)
            s_abs = np.bincount(idx, (wf[:, None] * av).ravel()[keep],
                                minlength=R * D).reshape(R, D)
            carried = np.bincount(idx, (wb[:, None] * av).ravel()[keep],
                                  minlength=R * D).reshape(R, D)
        bound = np.where(n > 0, (n + 8) * (U * s_abs + FLOOR) + carried, 0.0)
        m, z = AR._stats(rp, f)
        zf = np.where(np.isfinite(z), z, 0.0)
        outs.append(out)
        bounds.append(bound)
        ms.append(m)
        mbs.append(d_row)
        zs.append(z)
        zbs.append(((f.deg + 24 + 16 * f.A) * U + np.expm1(2 * d_row)) * zf)
        ws.append(f.w)
        wbs.append(wb)
        fs.append(f)
    st = (lambda xs, shape: np.stack(xs) if xs else np.zeros(shape))
    E = col.size
    return Dot(st(outs, (0, R, D)), st(bounds, (0, R, D)), st(ms, (0, R)), st(mbs, (0, R)),
               st(zs, (0, R)), st(zbs, (0, R)), st(ws, (0, E)), st(wbs, (0, E)), l, d, fs)


def alpha_from_stats(rp, l, m, z):
    """alpha [H, E] from the logits and the statistics, as the alpha entry computes it:
    exp(l - m) / z."""
    rows = ER.edge_rows(rp)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        shift = np.where(np.isneginf(m), 0.0, m)
        return np.exp(l - shift[:, rows]) / z[:, rows]


def heads_slice(a, H):
    """The first H heads of a Dot."""
    return Dot(*(x[:H] for x in a))
