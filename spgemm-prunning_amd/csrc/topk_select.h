// The two MaxK row selections of the CBSR encode (topk_cbsr.hip), restated word for word as
// device functions on a row already in registers, for the fused linear + MaxK (linear_maxk.hip,
// rows read from the GEMM's LDS tile).  topk_cbsr.hip keeps its own bodies inside its kernels, so
// the encode's machine code is what it was; a change to either copy belongs in both.  Output
// order of both: key descending, column ascending on ties, NaN largest (torch.topk's ranking).
//  * wave_row_select: one wavefront per row, column lane + 64 i in slot i of each lane; the
//    k-th largest key by an MSB-first radix select over data-adaptive 8-bit digits.
//  * rows4_take + rows4_emit: four rows per wave, 16 lanes (one DPP row) per row, columns
//    64 i + 4 q + j in slot 4 i + j of lane q; the threshold by bisection over DPP row sums.
#pragma once

#include "common.h"

namespace maxk {

// The device's count of rows whose search took other than k winners (topk_cbsr.hip owns it;
// maxk_topk_error_rows reads and resets it); NULL if the runtime cannot name it.
uint32_t *topk_bad_rows_counter();

__device__ __forceinline__ uint32_t order_key(float x) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x007fffffu)) return 0xffffffffu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t order_key(uint8_t x) { return x; }

// ---- one wavefront per row ---------------------------------------------------------------
// v / key / ok: the row's up to four values per lane (column lane + 64 i), their keys (0 past
// D) and whether the column exists.  hist: 256 words, skey / sval / scol: kMaxDim + kWave slots
// of this wave's LDS (winner slots [0, k), padding slots [k, k4) with key 0 and column 255:
// never ranked above a winner, and per-lane scratch slots [kMaxDim, kMaxDim + 64) for lanes not
// taking).  Stores the row's k winners in order; out_dense (optional) gets the masked row.  A
// row that took other than k winners is counted in *bad_rows.  Ends with a fence: the LDS slots
// are free for the next row.
template <typename T>
__device__ __forceinline__ void wave_row_select(
    const T (&v)[4], const uint32_t (&key)[4], const bool (&ok)[4], int k, int lane, int row,
    int D, uint32_t *hist, uint32_t *skey, T *sval, uint8_t *scol, T *__restrict__ out_val,
    uint8_t *__restrict__ out_idx, int32_t *__restrict__ out_idx32, T *__restrict__ out_dense,
    uint32_t *bad_rows) {
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    // T = max t such that #{key >= t} >= k  (the k-th largest key), by MSB-first radix
    // select with data-adaptive 8-bit digits: each pass takes the wave min / max of the
    // keys still in play and histograms the 8 bits right below their common prefix
    // (256-bin LDS histogram, integer atomics), then keeps the largest digit whose suffix
    // count still reaches `need`.  Real activations share their top bits (sign, exponent),
    // so a fixed top-byte digit would pile them into one bin; the adaptive digit spreads
    // them, and the pass usually ends the search (the chosen bin holds exactly the keys
    // still needed).
    uint32_t thr = 0, pmask = 0;
    int need = k;  // how many of the keys in play are still to be taken
    int sh = 0;    // selection compares key >> sh with thr (after the final shift)
    for (;;) {
        uint32_t mx = 0u, mn = ~0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = ok[i] && (key[i] & pmask) == thr;
            mx = in && key[i] > mx ? key[i] : mx;
            mn = in && key[i] < mn ? key[i] : mn;
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            const uint32_t a = __shfl_xor(mx, off), b = __shfl_xor(mn, off);
            mx = a > mx ? a : mx;
            mn = b < mn ? b : mn;
        }
        const uint32_t diff = mx ^ mn;
        if (diff == 0u) {  // every key in play is equal: it is T, ties decide
            thr = mx;
            sh = 0;
            break;
        }
        const int hb = 31 - __builtin_clz(diff);  // highest bit where keys in play differ
        const int shift = hb >= 7 ? hb - 7 : 0;   // digit = bits [shift, shift + 8)
        reinterpret_cast<uint4 *>(hist)[lane] = make_uint4(0u, 0u, 0u, 0u);
        wave_lds_fence();
#pragma unroll
        for (int i = 0; i < 4; ++i)  // branch-free: keys out of play add 0
            atomicAdd(&hist[(key[i] >> shift) & 255u], (ok[i] && (key[i] & pmask) == thr) ? 1u : 0u);
        wave_lds_fence();
        const uint4 h = reinterpret_cast<const uint4 *>(hist)[lane];  // bins 4*lane .. 4*lane+3
        const uint32_t s3 = h.w, s2 = h.z + s3, s1 = h.y + s2, s0 = h.x + s1;
        uint32_t acc = s0;  // -> sum of s0 over lanes >= this one
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const uint32_t t = __shfl_down(acc, off);
            acc += lane + off < kWave ? t : 0u;
        }
        const uint32_t above = acc - s0;  // keys with a digit in a higher lane's bins
        const uint32_t nd = (uint32_t)need;
        // largest digit d with #{digit >= d} >= need: the highest lane holding one
        // (s0 >= s1 >= s2 >= s3: the conditions are monotone, m = their count - 1)
        const int m = (int)(above + s0 >= nd) + (int)(above + s1 >= nd) +
                      (int)(above + s2 >= nd) + (int)(above + s3 >= nd) - 1;
        const uint32_t gt_l = above + (uint32_t)(m == 0) * s1 + (uint32_t)(m == 1) * s2 +
                              (uint32_t)(m == 2) * s3;  // #{digit > 4*lane + m}
        const uint32_t ge_l = above + (uint32_t)(m == 0) * s0 + (uint32_t)(m == 1) * s1 +
                              (uint32_t)(m == 2) * s2 + (uint32_t)(m == 3) * s3;
        const uint64_t has = __ballot(m >= 0);
        const int src = 63 - __clzll(has);
        const int dm = __shfl(m, src);
        const uint32_t gt = __shfl(gt_l, src);
        const uint32_t in_bin = __shfl(ge_l, src) - gt;
        need -= (int)gt;
        // keys in play share every bit above shift + 8 (they differ first at bit hb)
        const uint32_t high = shift + 8 >= 32 ? 0u : (mx & (~0u << (shift + 8)));
        thr = high | ((uint32_t)(4 * src + dm) << shift);
        pmask = ~0u << shift;
        sh = shift;
        if (in_bin == (uint32_t)need || shift == 0) break;  // bin fully taken, or T exact
    }
    const int need_eq = need;
    thr >>= sh;

    // select, then compact winners into LDS slots [0, k)
    const int k4 = (k + 3) & ~3;
    for (int p = k + lane; p < k4; p += kWave) {
        skey[p] = 0u;
        scol[p] = 255;
    }
    int eq_base = 0, slot_base = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool eq = ok[i] && (key[i] >> sh) == thr;
        const uint64_t me = __ballot(eq);
        const int eq_rank = eq_base + __popcll(me & lt_mask);
        eq_base += __popcll(me);
        const bool take = (ok[i] && (key[i] >> sh) > thr) || (eq && eq_rank < need_eq);
        if (out_dense && ok[i])  // fused masked dense output (wave-uniform pointer test)
            out_dense[(int64_t)row * D + lane + kWave * i] = take ? v[i] : T(0);
        const uint64_t mt = __ballot(take);
        const int ws = slot_base + __popcll(mt & lt_mask);
        const int slot = take && ws < k ? ws : kMaxDim + lane;  // never past the k slots
        skey[slot] = key[i];
        sval[slot] = v[i];
        scol[slot] = (uint8_t)(lane + kWave * i);
        slot_base += __popcll(mt);
    }
    // any other count than k is a search bug: counted for the host (maxk_topk_error_rows)
    if (lane == 0 && slot_base != k) atomicAdd(bad_rows, 1u);
    wave_lds_fence();
    // rank of winner p among the winners: (key desc, column asc); 4 slots per LDS read
    for (int p = lane; p < k; p += kWave) {
        const uint32_t kp = skey[p];
        const int cp = scol[p];
        int pos = 0;
        for (int q = 0; q < k4; q += 4) {
            const uint4 kq = *reinterpret_cast<const uint4 *>(&skey[q]);
            const uint32_t cq = *reinterpret_cast<const uint32_t *>(&scol[q]);
            pos += (kq.x > kp) || (kq.x == kp && (int)(cq & 255u) < cp);
            pos += (kq.y > kp) || (kq.y == kp && (int)((cq >> 8) & 255u) < cp);
            pos += (kq.z > kp) || (kq.z == kp && (int)((cq >> 16) & 255u) < cp);
            pos += (kq.w > kp) || (kq.w == kp && (int)(cq >> 24) < cp);
        }
        const int64_t o = (int64_t)row * k + pos;
        out_val[o] = sval[p];
        out_idx[o] = (uint8_t)cp;
        if (out_idx32) out_idx32[o] = cp;
    }
    wave_lds_fence();  // this row's LDS slots are read before the next row overwrites them
}

// ---- four rows per wave: 16 lanes per row ------------------------------------------------
// A row lives on 16 lanes (one DPP row, 16 values per lane: columns 64i + 4q + j), so every
// cross-lane step of a row is a DPP row operation folded into a VALU instruction and one
// wave instruction works on four rows.  Per row: the k-th largest key by a bitwise search
// (no LDS, no histogram atomics), tie-exact selection in column order, winners compacted to
// LDS and ranked (key desc, column asc) against each other.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true);
}
// all-reduce over the 16 lanes of a row (row_ror 8, 4, 2, 1)
__device__ __forceinline__ uint32_t row_max(uint32_t x) {
    x = max(x, dpp<0x128>(x));
    x = max(x, dpp<0x124>(x));
    x = max(x, dpp<0x122>(x));
    return max(x, dpp<0x121>(x));
}
__device__ __forceinline__ uint32_t row_min(uint32_t x) {
    x = min(x, dpp<0x128>(x));
    x = min(x, dpp<0x124>(x));
    x = min(x, dpp<0x122>(x));
    return min(x, dpp<0x121>(x));
}
__device__ __forceinline__ uint32_t row_sum(uint32_t x) {
    x += dpp<0x128>(x);
    x += dpp<0x124>(x);
    x += dpp<0x122>(x);
    return x + dpp<0x121>(x);
}
// exclusive prefix (lanes below in the row; row_shr: lane i reads lane i-n, 0 past the row)
__device__ __forceinline__ uint32_t row_prefix_excl(uint32_t x) {
    uint32_t a = x;
    a += dpp<0x111>(a);
    a += dpp<0x112>(a);
    a += dpp<0x114>(a);
    a += dpp<0x118>(a);
    return a - x;
}

#if MAXK_TOPK_FENCE_WAIT  // tools only: drain the wave's LDS queue at every fence
#define wave_lds_fence()                                  \
    do {                                                  \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
        maxk::wave_lds_fence();                           \
    } while (0)
#endif

// take[t] = whether the row keeps the key in slot t: exactly k per row.  key holds 0 in the
// slots past D (ok false).  q = the lane in its row; `live` = the row exists (a dead sub-row
// runs the same search on whatever it holds and only skips the stores); n_bad counts, on lane
// q == 0, the live rows whose search was wrong.
template <int J>
__device__ __forceinline__ void rows4_take(const uint32_t (&key)[16], const bool (&ok)[16],
                                           int k, int q, bool live, bool (&take)[16],
                                           uint32_t &n_bad) {
    // ---- threshold T = the k-th largest key, built bit by bit from the highest bit where
    // the row's keys differ: T | bit is kept while at least k keys are >= it (one compare
    // per key and a DPP row sum per bit, no LDS).  A candidate with exactly k keys >= it
    // ends the row's search: selecting key >= T then takes exactly k.
    // The search starts at the highest bit where mx and a lower bound lb of the answer
    // differ: lb = max(smallest key, smallest over the row's lanes of the lane's j-th
    // largest key, j = ceil(k / 16)), since 16 lanes x j keys are >= the latter.  The
    // answer lies in [lb, mx] and so shares their common prefix; on Gaussian rows this
    // skips the sign and most exponent bits.
    // m[0..J) = the lane's J largest keys (an insertion network, lowest slot first so
    // every slot reads the previous key's values); the lane's j-th largest with
    // j = ceil(k / 16) <= J bounds the answer from below: 16 lanes x j keys are >= the
    // smallest of them over the row, and 16 j >= k.
    uint32_t mx = 0u, mn = ~0u, m[J];
#pragma unroll
    for (int j = 0; j < J; ++j) m[j] = 0u;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        mx = key[t] > mx ? key[t] : mx;  // columns past D hold key 0
        mn = ok[t] && key[t] < mn ? key[t] : mn;
#pragma unroll
        for (int j = J - 1; j > 0; --j) m[j] = max(m[j], min(m[j - 1], key[t]));
        m[0] = max(m[0], key[t]);
    }
    mx = row_max(mx);
    mn = row_min(mn);
    uint32_t mj = m[0];
#pragma unroll
    for (int j = 1; j < J; ++j) mj = k > 16 * j ? m[j] : mj;
    uint32_t lb = MAXK_TOPK_LB ? row_min(mj) : 0u;
    lb = lb > mn ? lb : mn;
    uint32_t thr;
    int need = k;
    if (MAXK_TOPK_BISECT) {
        // Bisection over the key interval [lb, mx] itself: the answer is the largest c
        // with at least k keys >= c.  Invariant: >= k keys are >= lo, the answer <= hi.
        // The bit search below halves a power-of-two interval instead, which is 2^31
        // wide whenever [lb, mx] straddles a float exponent boundary with a carry (a
        // Gaussian row's does: 0x3F7F... -> 0x4000...); the count of keys >= mid == k
        // ends a row early in both.
        uint32_t lo = lb, hi = mx;
        bool done = lo == hi;  // rows past the end search too (see `take` below)
        for (;;) {
            const bool go = !done;
            if (__ballot(go) == 0) break;
            const uint32_t d = hi - lo;
            const uint32_t mid = lo + (d >> 1) + (d & 1u);  // in (lo, hi]: >= 1
            uint32_t n = 0;  // columns past D hold key 0 < mid: no mask needed
#pragma unroll
            for (int t = 0; t < 16; ++t) n += key[t] >= mid ? 1u : 0u;
            n = row_sum(n);
            if (go) {
                if (n >= (uint32_t)k) lo = mid;
                else hi = mid - 1u;
                if (n == (uint32_t)k || lo == hi) done = true;
            }
        }
        thr = lo;
    } else {
        const uint32_t diff = mx ^ lb;
        int bit = diff ? 31 - __builtin_clz(diff) : -1;
        // common prefix of the keys (all keys are >= it); bit 31 differing -> no prefix
        thr = !diff ? mx : (bit == 31 ? 0u : mx & (~0u << (bit + 1)));
        bool done = diff == 0u;
        for (;;) {
            const bool go = !done && bit >= 0;
            if (__ballot(go) == 0) break;
            const uint32_t c = thr | (1u << (bit & 31));
            uint32_t n = 0;  // columns past D hold key 0 < c (c >= 1): no mask needed
#pragma unroll
            for (int t = 0; t < 16; ++t) n += key[t] >= c ? 1u : 0u;
            n = row_sum(n);
            if (go) {
                if (n >= (uint32_t)k) thr = c;
                if (n == (uint32_t)k) done = true;
                --bit;
            }
        }
    }
    const int sh = 0;
    // keys > thr are taken; `need` of the keys == thr (ties: lowest columns first)
    {
        uint32_t ngt = 0;
#pragma unroll
        for (int t = 0; t < 16; ++t) ngt += (ok[t] && key[t] > thr) ? 1u : 0u;
        need = k - (int)row_sum(ngt);
    }
    const uint32_t T_ = thr >> sh;
    // ---- selection: key > T, plus the lowest-column keys == T until k are taken
    uint32_t neq = 0;
#pragma unroll
    for (int t = 0; t < 16; ++t) neq += (ok[t] && (key[t] >> sh) == T_) ? 1u : 0u;
    const uint32_t neq_row = row_sum(neq);  // every lane: DPP reads the whole row
    // Rows past the end (the last row group's dead sub-rows, holding a copy of the last
    // row) run the same exact search and take exactly k winners; they only skip the
    // stores.  Skipping their search (r02) left thr at their lower bound, so "key >= thr"
    // took 32-100 winners whose compaction ran past the row's 3*k4 LDS words into the next
    // wave's winners -- which that wave, one grid-stride round behind, could still be
    // ranking (r02's k = 48 mismatch on row 2186888 of the seed-0 [2449029, 256] Gaussian
    // input).  Searching costs nothing there; a `live` test per key cost 2-3 %.
    const bool ties = neq_row != (uint32_t)need;
    // The selection below takes (k - need) keys above the threshold plus min(need, neq_row)
    // equal ones: exactly k whenever 0 <= need <= neq_row, which the search guarantees.  A
    // row outside that is a bug in the search (r02's dead sub-rows were one): it is counted
    // for the host (maxk_topk_error_rows) and takes no winners at all, so its compaction
    // cannot write past its k LDS slots into another row's or another wave's winners, and
    // the good rows need no per-winner bound check.  Such a row always has ties
    // (neq_row != need: need < 0 wraps past any count), so the check sits in that branch.
    if (__ballot(ties) == 0) {
#pragma unroll
        for (int t = 0; t < 16; ++t) take[t] = ok[t] && (key[t] >> sh) >= T_;
    } else {  // rank the equal keys in column order: chunk i, then lane, then j
        uint32_t base = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t c = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) c += (ok[4 * i + j] && (key[4 * i + j] >> sh) == T_);
            uint32_t r = base + row_prefix_excl(c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = 4 * i + j;
                const bool eq = ok[t] && (key[t] >> sh) == T_;
                take[t] = (ok[t] && (key[t] >> sh) > T_) || (eq && r < (uint32_t)need);
                r += eq ? 1u : 0u;
            }
            base += row_sum(c);
        }
        const bool bad = (uint32_t)need > neq_row;
        if (__ballot(bad) != 0) {  // never taken unless the search is wrong
            n_bad += live && q == 0 && bad ? 1u : 0u;
#pragma unroll
            for (int t = 0; t < 16; ++t) take[t] = take[t] && !bad;
        }
    }
}

// Compacts the row's winners (take) into its LDS slots wkey / wval / wcol (k4 words each),
// ranks them (key desc, column asc) and, for a live row, stores them.  Fenced at both ends:
// the previous group's winners are read before these overwrite them, and these before the
// next group's.
template <typename T>
__device__ __forceinline__ void rows4_emit(const T (&v)[16], const uint32_t (&key)[16],
                                           const bool (&take)[16], int k, int q, bool live,
                                           int row, uint32_t *wkey, uint32_t *wval,
                                           uint32_t *wcol, T *__restrict__ out_val,
                                           uint8_t *__restrict__ out_idx,
                                           int32_t *__restrict__ out_idx32) {
    const int k4 = (k + 3) & ~3;
    uint32_t nw = 0;
#pragma unroll
    for (int t = 0; t < 16; ++t) nw += take[t] ? 1u : 0u;
    uint32_t slot = row_prefix_excl(nw);  // a row's winners fill slots [0, k) (`bad` above)
    wave_lds_fence();  // the previous group's winners are no longer read
    for (int p = k + q; p < k4; p += 16) {
        wkey[p] = 0u;
        wcol[p] = 255u;
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        if (take[t]) {
            wkey[slot] = key[t];
            wval[slot] = sizeof(T) == 4 ? __builtin_bit_cast(uint32_t, (float)v[t])
                                        : (uint32_t)v[t];
            wcol[slot] = (uint32_t)(64 * (t >> 2) + 4 * q + (t & 3));
            ++slot;
        }
    }
    wave_lds_fence();
    if (live) {
        for (int p = q; p < k; p += 16) {
            const uint32_t kp = wkey[p], cp = wcol[p];
            int pos = 0;
            for (int o = 0; o < k4; o += 4) {
                const uint4 kq = *reinterpret_cast<const uint4 *>(&wkey[o]);
                const uint4 cq = *reinterpret_cast<const uint4 *>(&wcol[o]);
                pos += (kq.x > kp) || (kq.x == kp && cq.x < cp);
                pos += (kq.y > kp) || (kq.y == kp && cq.y < cp);
                pos += (kq.z > kp) || (kq.z == kp && cq.z < cp);
                pos += (kq.w > kp) || (kq.w == kp && cq.w < cp);
            }
            const int64_t o = (int64_t)row * k + pos;
            const uint32_t vb = wval[p];
            if constexpr (sizeof(T) == 4)
                out_val[o] = __builtin_bit_cast(float, vb);
            else
                out_val[o] = (T)vb;
            out_idx[o] = (uint8_t)cp;
            if (out_idx32) out_idx32[o] = (int32_t)cp;
        }
    }
    wave_lds_fence();  // winners read before the next group's overwrite them
}

#ifdef wave_lds_fence
#undef wave_lds_fence
#endif

}  // namespace maxk
