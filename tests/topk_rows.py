"""One corpus of hard rows for the MaxK row selection, any width 1 <= D <= 1024.

The selection (the k-th largest order key by an MSB-first radix search over data-adaptive 8-bit
digits, ties in column order, the winners ranked key descending / column ascending) exists three
times: topk_cbsr.hip, topk_select.h (the fused linear layer) and x16_topk.hip.  rows(D, rng)
generalises the row kinds of test_parity_gpu.py's test_topk_threshold_search_edges and
test_topk_grid_stride_tails to any D, so that every copy can be held to the same rows.  The
reference ranking is x16_ref.topk; test_x16_cpu.py pins it against the C oracle.
"""
import numpy as np

BOUNDARIES = (64, 256, 512)  # a lane's slot changes at 64 j; the u8 / NE = 4 / NE = 8 widths end


def x16_ks(D):
    """The x16 encode's k sweep: the k4 padding (1..5), the rank loop's 64-slot steps (63..65,
    127..129, 255, 256), and k = D where the kernel allows it."""
    ks = {k for k in (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256) if k <= min(D, 256)}
    return sorted(ks | ({D} if D <= 256 else set()))


def fused_ks(D):
    """The fused layer's: the k4 padding, rows4<2> / rows4<4> / wave select at 32 | 33 and
    48 | 49, the wave select's second slot step at 64 | 65, and k = D."""
    return sorted({k for k in (1, 3, 4, 5, 31, 32, 33, 47, 48, 49, 63, 64, 65, D) if k <= D})


def _f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _kinds(D, rng):
    """[(name, row)], every row of D values; float64 rows are cast by rows()."""
    u, g = rng.random, rng.standard_normal
    out = [("equal+", np.full(D, 1.5)), ("equal-", np.full(D, -2.0)),
           ("zeros+", np.zeros(D)), ("zeros-", np.full(D, -0.0)),
           ("zeros+-", np.where(u(D) < .5, 0.0, -0.0)),
           ("nan", np.full(D, np.nan)),
           ("nan30", np.where(u(D) < .3, np.nan, 1.0)),
           ("inf+-", np.where(u(D) < .5, np.inf, -np.inf)),
           ("three", rng.integers(0, 3, D) * 1.0),
           ("halves", rng.integers(-2, 2, D) * 0.5),
           # two neighbouring floats: keys one apart, the search ends at shift 0 with ties
           ("ulp_pair", _f32(_bits(1.0) + rng.integers(0, 2, D).astype(np.uint32)))]
    # D consecutive floats, permuted: keys one apart, all distinct
    out.append(("steps", rng.permutation(_f32(_bits(1.0) + np.arange(D, dtype=np.uint32)))))
    out.append(("steps_subnormal", rng.permutation(_f32(1 + np.arange(D, dtype=np.uint32)))))
    # two clusters, each sharing its top 24 key bits (the low byte varies, with repeats past 256
    # columns): the first pass separates the clusters, a k inside one needs a second pass
    hi = np.where(u(D) < .5, _bits(1.0), _bits(3.0)).astype(np.uint32)
    out.append(("clusters8", _f32(hi + rng.integers(0, 256, D).astype(np.uint32))))
    # ... and 16 bits below a shared prefix: two passes inside a cluster
    out.append(("clusters16", _f32(hi + rng.integers(0, 1 << 16, D).astype(np.uint32))))
    for name, big in (("huge1e30", 1e30), ("huge3e38", 3e38)):
        row = u(D)
        row[int(rng.integers(0, D))] = big
        out.append((name, row))
    row = g(D)
    sp = [np.inf, -np.inf, np.nan, -0.0, 0.0, 3e38][:min(D, 6)]
    row[rng.choice(D, len(sp), replace=False)] = sp
    out.append(("specials", row))
    out += [("gauss", g(D)), ("gauss2", g(D)), ("uniform", u(D)), ("uniform-", -u(D))]
    for b in BOUNDARIES:  # equal maximal values on both sides of a slot / kernel-width boundary
        if b < D:
            row = g(D)
            row[b - 2:min(D, b + 3)] = 9.0
            out.append((f"run{b}", row))
    row = g(D)
    row[max(0, D - 5):] = 7.0  # equal maximal values ending at the last column
    out.append(("run_end", row))
    row = rng.integers(0, 2, D) * 1.0  # one bin holds every key still in play
    out.append(("two", row))
    return out


def rows(D, rng, names=False):
    """fp32 [2 n, D]: the n (about 30) kinds above, then the same rows with their columns
    permuted (one permutation).  names=True: (rows, the 2 n kind names)."""
    assert 1 <= D <= 1024
    kinds = _kinds(D, rng)
    x = np.stack([np.asarray(r).astype(np.float32) for _, r in kinds])
    x = np.concatenate([x, rng.permutation(x, axis=1)])
    if names:
        return x, [n for n, _ in kinds] + [n + "/perm" for n, _ in kinds]
    return x


def finite_mask(x):
    return np.isfinite(x).all(axis=1)


def finite(x):
    """The rows without Inf or NaN."""
    return x[finite_mask(x)]
