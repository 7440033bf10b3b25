"""Expected values and bounds of the fused multi-head GAT attention (gat_attention_heads.hip), in
plain numpy float64.  Edge e lies in CSR row r, c = col[e]:

    out[h, r, ci[c, l]] += alpha[h, e] * cv[c, l]         alpha = edge_softmax_ref.gat_forward's w
    m[h, r] = max_e l_he        z[h, r] = sum_e exp(l_he - m[h, r])         (the row statistics)
    alpha[h, e] = exp(l_he - m[h, r]) / z[h, r]            (what the alpha entry rebuilds)

out is a float64 scatter-sum of the reference alpha per head; a selector >= D adds nothing.  Inf
and NaN follow IEEE through numpy: a NaN alpha makes every element it is added to NaN and leaves
the others alone, alpha = 0 (a -Inf logit) times an Inf value is NaN.  The statistics take the
maximum that ignores NaN, as fmaxf does (a row of nothing but NaN: -Inf); z of such a row is NaN
either way.  A row of nothing but -Inf has m = -Inf and z = 0 (nothing is subtracted from its
logits, as in the edge softmax kernels), so the alpha rebuilt from them is 0 / 0 = NaN, which is
what exp(-Inf - -Inf) gives.  A row without edges has m = z = 0 and out = 0.

Bounds, u = 2^-24, n_r the row's degree, A_r = max_e |z_e| over the row's finite values:

weight    |alpha' - alpha| <= (n_r + 24 + 16 A_r) u alpha + (n_r + 16) 2^-149: the edge softmax's
          bound with 8 u more.  The kernel never forms alpha: out = (sum_e p_e v_e) / z with
          p_e = exp(l_e - m_piece), and for a row cut over work items the merge scales a piece's
          sums, numerator and denominator alike, by exp(m_piece - m_r).  On each side that is,
          beside what edge_softmax_ref derives, one more rounded argument (m_piece - m_r, at most
          2 A_r u: the fourth of the four roundings per side that its 16 A_r u already pays
          for), one more exp (2 ulp, 4 u) and one more product (u): 10 u on both sides together,
          8 u of them added here and 2 u taken from the slack the softmax bound's n_r + 16 leaves
          over its n_r sum terms, its division and its own exps.  The division by z happens once
          per element after the sum instead of once per edge before it: the same single
          rounding.
out       (n + 8) (u sum_e |alpha_e v_e| + 2^-149) + sum_e dalpha_e |v_e|, n the element's number
          of addends (numerics.count_fwd): the forward aggregation's bound with the subnormal
          floor, plus the weight bound carried through the sum.  The order of the sum (lane
          groups, LDS copies, the pieces of a cut row) does not enter: an addend passes through
          at most n - 1 additions that round (adding the exact 0 of a copy or a piece without
          addends rounds nothing; the product is fused into its addition), then one scale
          product of its piece and the one division: n + 1 roundings, inside n + 8.  An element
          without addends is exactly 0.
m         2 A_r u: the fp32 score sum and the slope product, each at most A_r u.
z         the weight bound's relative part on z itself, (n_r + 24 + 16 A_r) u z: its terms are
          the denominator's share of the derivation above.
alpha     from the statistics: edge_softmax_ref's own bound of w (one exp per side on the
          numerator; the cut-row merge of z is the edge softmax's merge).

These constants are derived, not measured.  tests/test_gat_attention_cpu.py pins the formulas
against torch autograd of a dense float64 composition."""
from collections import namedtuple

import numpy as np

import edge_softmax_ref as ER

U = ER.U
FLOOR = ER.FLOOR

Attn = namedtuple("Attn", "out out_bound m m_bound z z_bound w w_bound heads")


def weight_bound(f, extra=8):
    """The weight bound above from a Fwd of edge_softmax_ref: its bound plus 8 u alpha
    (extra=0: the edge softmax's own, for the composition of the two stored entries)."""
    return f.bound + extra * U * np.where(np.isfinite(f.w), f.w, 0.0)


def _stats(rp, f):
    """(m, z) of one head: the NaN-ignoring maximum and the sum of exp(l - m) (of exp(l) where
    m = -Inf); 0 for a row without edges."""
    with np.errstate(invalid="ignore", over="ignore"):
        lm = np.where(np.isnan(f.l), -np.inf, f.l)
        m = ER._row_reduce(np.maximum, lm, rp, 0.0)
        shift = np.where(np.isneginf(m), 0.0, m)
        z = ER._row_reduce(np.add, np.exp(f.l - shift[f.rows]), rp, 0.0)
    return m, z


def attention(rp, col, s_dst, s_src, slope, cv, ci, D, counts, extra=8):
    """s_dst [H, R], s_src [H, C] (fp32), the CBSR (cv, ci) [C, k], counts [R, D] the number of
    addends per output element (numerics.count_fwd) -> Attn, everything stacked head-major.
    extra: see weight_bound."""
    H, R = s_dst.shape
    fs = [ER.gat_forward(rp, col, s_dst[h], s_src[h], slope) for h in range(H)]
    rows = fs[0].rows if H else ER.edge_rows(rp)
    sel = ci[col].astype(np.int64)                          # [E, k]
    keep = (sel < D).ravel()
    idx = (rows[:, None].astype(np.int64) * D + sel).ravel()[keep]
    v = cv[col].astype(np.float64)                          # [E, k]
    av = np.where(np.isfinite(v), np.abs(v), 0.0)
    n = np.rint(np.asarray(counts, np.float64))
    outs, bounds, ms, mbs, zs, zbs = [], [], [], [], [], []
    for f in fs:
        with np.errstate(invalid="ignore", over="ignore"):
            t = (f.w[:, None] * v).ravel()[keep]
            out = np.bincount(idx, t, minlength=R * D).reshape(R, D)
            wf = np.where(np.isfinite(f.w), f.w, 0.0)
            s_abs = np.bincount(idx, (wf[:, None] * av).ravel()[keep],
                                minlength=R * D).reshape(R, D)
            carried = np.bincount(idx, (weight_bound(f, extra)[:, None] * av).ravel()[keep],
                                  minlength=R * D).reshape(R, D)
        bound = np.where(n > 0, (n + 8) * (U * s_abs + FLOOR) + carried, 0.0)
        m, z = _stats(rp, f)
        outs.append(out)
        bounds.append(bound)
        ms.append(m)
        mbs.append(2 * f.A * U)
        zs.append(z)
        zf = np.where(np.isfinite(z), z, 0.0)
        zbs.append((f.deg + 24 + 16 * f.A) * U * zf)
    st = np.stack
    return Attn(st(outs), st(bounds), st(ms), st(mbs), st(zs), st(zbs),
                st([f.w for f in fs]), st([f.bound for f in fs]), fs)


def alpha_from_stats(rp, col, s_dst, s_src, slope, m, z):
    """alpha [H, E] from the statistics, as the alpha entry computes it: exp(l - m) / z."""
    out = []
    for h in range(s_dst.shape[0]):
        _, l = ER.gat_logits(rp, col, s_dst[h], s_src[h], slope)
        rows = ER.edge_rows(rp)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            shift = np.where(np.isneginf(m[h]), 0.0, m[h])
            out.append(np.exp(l - shift[rows]) / z[h][rows])
    return np.stack(out)


def heads_slice(a, H):
    """The first H heads of an Attn."""
    return Attn(*(x[:H] for x in a))
