"""Expected values and bounds of the attention dropout (attn_dropout.h, attn_dropout.hip and the
dropout entries of gat_attention_heads.hip / gat_attention_heads_bwd.hip), in plain numpy.

The mask.  Head h, edge e (its CSR position), rate p, 64-bit seed:

    (r0, r1, r2, r3) = Philox4x32-10(counter (e, 0, h >> 2, 0), key (seed & 0xffffffff, seed >> 32))
    dropped iff r[h & 3] < thr,  thr = min(floor(p * 2^32), 2^32 - 1)
    d[h, e] = 0 if dropped else scale,  scale = float32(1 / (1 - p))

p enters as the float32 the C ABI carries.  philox4x32_10 below is the generator in uint64
arithmetic (every product of two 32-bit words is exact there).

The dropped forward and backward, on the references of gat_attention_ref (alpha, the
statistics) and gat_attention_bwd_ref, in float64 with the exact float32 scale:

    out[h, r, ci[c, l]] += alpha_he d_he cv[c, l]          m, z: those of the undropped softmax
    ga, t as gat_attention_bwd_ref, t from the dropped out (sum_e alpha_e d_e ga_e exactly)
    gz_he = alpha_he (d_he ga_he - t_hr) (z_he > 0 ? 1 : slope)
    g_cbsr[c, l] = sum_h sum_{e -> c} alpha_he d_he G[h, r, ci[c, l]]

Inf and NaN follow IEEE through numpy with d as a factor: 0 * NaN and 0 * Inf are NaN.

Bounds, u = 2^-24; each is the bound of the entry without dropout carried through the factor d
(0 or scale, exact), plus the roundings the factor adds:

coef     alpha d: d * (alpha's bound) + u |alpha d|, the one product by scale.  The forward
         kernel never forms it: it sums p * (0 or 1) * value exactly as without dropout and
         multiplies the row by scale after the division, one rounding of the sum.
out      (n + 8) (u S + scale 2^-149) + d-carried weight bound + u S,  S = sum_e |alpha_e d_e v_e|:
         gat_attention_ref's out bound on the dropped terms (a dropped edge's exact 0 product
         still counts among the n addends: it rounds nothing), its subnormal floor scaled with
         the row, and u S for the product by scale.  An element without addends is exactly 0,
         and so is, for finite inputs, an element all of whose addends are dropped (S = 0 and
         the carried bound is 0 where d is 0).
x        d ga - t: d * d_ga + u |d ga| (the product) + d_t + u |x| (the subtraction); t's bound
         is gat_attention_bwd_ref's with the dropped out and its out_err.
gz       the product bound of gat_attention_bwd_ref with that x: alpha is the undropped
         coefficient with the edge softmax's bound.
scores   edge_softmax_ref._sum_bound over the row or the column, as there.
g_cbsr   feat_grad_ref on coef: (n + 8) u sum |alpha d G| plus coef's bound carried through |G|.
stored   the rebuilt backward runs the stored passes on gw = d ga (bound d * d_ga + u |d ga|):
         heads_softmax_ref.backward_heads with that gw and gw_bound (rebuilt_backward).

These constants are derived, not measured.  tests/test_attn_dropout_cpu.py pins the generator
against its known answers and the formulas against torch autograd of a dense float64
composition that multiplies the same d in."""
from collections import namedtuple

import numpy as np

import edge_grad_ref as R
import edge_softmax_ref as ER
import gat_attention_bwd_ref as BR
import gat_attention_ref as AR
import heads_softmax_ref as HS

U = AR.U
FLOOR = AR.FLOOR
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two ints -> four uint32 arrays."""
    x = [np.asarray(c, np.uint64) & MASK32 for c in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        a = M0 * x[0]
        b = M1 * x[2]
        x = [(b >> S32) ^ x[1] ^ np.uint64(k0), b & MASK32,
             (a >> S32) ^ x[3] ^ np.uint64(k1), a & MASK32]
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return [w.astype(np.uint32) for w in x]


def threshold(p):
    t = np.floor(float(np.float32(p)) * 4294967296.0)
    return int(min(t, 4294967295.0))


def scale(p):
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


def dropped(H, E, p, seed):
    """bool [H, E]: the dropped (head, edge) pairs."""
    seed = int(seed)
    e = np.arange(E, dtype=np.uint64)
    thr = threshold(p)
    out = np.zeros((H, E), bool)
    for q in range((H + 3) // 4):
        r = philox4x32_10((e, 0, q, 0), (seed & 0xFFFFFFFF, seed >> 32))
        for j in range(4):
            if 4 * q + j < H:
                out[4 * q + j] = r[j] < thr
    return out


def mask(H, E, p, seed):
    """d [H, E] float64: 0 where dropped, else the float32 scale."""
    return np.where(dropped(H, E, p, seed), 0.0, np.float64(scale(p)))


def _fabs(a):
    return np.where(np.isfinite(a), np.abs(a), 0.0)


def drop_attention(a, d, rp, col, cv, ci, D, counts):
    """a: gat_attention_ref.Attn of the undropped attention (extra = 8), d [H, E] -> the Attn of
    the dropped one: out and its bound, m and z as they were, w = alpha d with coef's bound, and
    heads whose w and bound are coef's (what feat_grad_ref reads)."""
    H = len(a.heads)
    R_ = rp.size - 1
    rows = ER.edge_rows(rp)
    sel = ci[col].astype(np.int64)
    keep = (sel < D).ravel()
    idx = (rows[:, None].astype(np.int64) * D + sel).ravel()[keep]
    v = cv[col].astype(np.float64)
    av = _fabs(v)
    n = np.rint(np.asarray(counts, np.float64))
    sc = float(d.max()) if d.size else 1.0
    outs, bounds, ws, wbs, heads = [], [], [], [], []
    for h in range(H):
        f = a.heads[h]
        with np.errstate(invalid="ignore", over="ignore"):
            wd = f.w * d[h]
            out = np.bincount(idx, (wd[:, None] * v).ravel()[keep],
                              minlength=R_ * D).reshape(R_, D)
            s_abs = np.bincount(idx, (_fabs(wd)[:, None] * av).ravel()[keep],
                                minlength=R_ * D).reshape(R_, D)
            carried = np.bincount(idx, ((AR.weight_bound(f) * d[h])[:, None] * av).ravel()[keep],
                                  minlength=R_ * D).reshape(R_, D)
        bound = np.where(n > 0, (n + 8) * (U * s_abs + max(sc, 1.0) * FLOOR) + carried
                         + U * s_abs, 0.0)
        wb = f.bound * d[h] + U * _fabs(wd)
        outs.append(out)
        bounds.append(bound)
        ws.append(wd)
        wbs.append(wb)
        heads.append(f._replace(w=wd, bound=wb))
    st = np.stack
    return AR.Attn(st(outs), st(bounds), a.m, a.m_bound, a.z, a.z_bound, st(ws), st(wbs), heads)


def attention(rp, col, s_dst, s_src, slope, cv, ci, D, counts, p, seed, base=None):
    """(the dropped Attn, the undropped Attn, d): see drop_attention.  base: the undropped Attn
    where the caller has it."""
    H = s_dst.shape[0]
    a = AR.attention(rp, col, s_dst, s_src, slope, cv, ci, D, counts) if base is None else base
    d = mask(H, col.size, p, seed)
    return drop_attention(a, d, rp, col, cv, ci, D, counts), a, d


def backward(g, a, ad, d, cv, ci, G, slope, D, out_err, feat_grad_ref=None, ers=None):
    """The fused backward under dropout.  g: the graph, a: the undropped Attn, ad: the dropped
    one, d the mask, G [H, R, D] fp32, out_err the bound of the dropped `out` the kernel is
    given against ad.out -> gat_attention_bwd_ref.Bwd, whose ga and ga_bound hold d ga."""
    rp, col = g.rp, g.col
    H = len(a.heads)
    ers = BR.edge_grads(g, cv, ci, G[:H]) if ers is None else ers
    rows = ER.edge_rows(rp)
    deg = np.diff(rp).astype(np.float64)
    cnt = np.bincount(col, minlength=g.C).astype(np.float64)
    G64 = np.asarray(G, np.float64)
    res = {k: [] for k in BR.Bwd._fields[:10]}
    for h in range(H):
        f = a.heads[h]
        er = ers[h]
        ga, d_ga = er.ref, R.bound(er)
        has = ad.out_bound[h] > 0                       # the columns with an addend
        with np.errstate(invalid="ignore", over="ignore"):
            og = np.where(has, ad.out[h] * G64[h], 0.0)
            t = og.sum(1)
            n_t = has.sum(1).astype(np.float64)
            d_t = ((n_t + 8) * U * _fabs(og).sum(1)
                   + np.where(has, out_err[h] * _fabs(G64[h]), 0.0).sum(1))
            dga = d[h] * ga
            d_dga = d[h] * d_ga + U * _fabs(dga)
            x = dga - t[rows]
            d_x = d_dga + d_t[rows] + U * _fabs(x)
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
        for k, v in zip(BR.Bwd._fields[:10], (dga, d_dga, t, d_t, gz, d_gz, g_dst, g_dst_bound,
                                              g_src, g_src_bound)):
            res[k].append(v)
    gc = gcb = None
    if feat_grad_ref is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            gc, gcb = feat_grad_ref(g, ad, G, ci, D)
    return BR.Bwd(*(np.stack(res[k]) for k in BR.Bwd._fields[:10]), gc, gcb)


def rebuilt_backward(g, a, d, ers, slope):
    """The score gradients of the rebuilt backward (the stored passes on gw = d ga):
    heads_softmax_ref.backward_heads with the masked weight gradient and its bound."""
    H = len(a.heads)
    with np.errstate(invalid="ignore", over="ignore"):
        gw = np.stack([d[h] * ers[h].ref for h in range(H)])
        gwb = np.stack([d[h] * R.bound(ers[h]) for h in range(H)]) + U * _fabs(gw)
    return HS.backward_heads(g.rp, g.col, HS.HeadsFwd(a.heads, a.w, a.w_bound), gw, slope, g.C,
                             gw_bound=gwb)
