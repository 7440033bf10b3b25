// Edge softmax over the incoming edges of every destination (CSR row), for gfx950: the
// normalisation that turns per-edge scores into the weights the aggregation takes, forward and
// backward, in a plain form over caller-given logits and a GAT form that builds the logits from
// two per-vertex scores,
//
//   z_e = s_dst[r] + s_src[c]     l_e = z_e > 0 ? z_e : slope * z_e       (GAT form only)
//   w_e = exp(l_e - m_r) / sum_{j in r} exp(l_j - m_r)      m_r = max_{j in r} l_j
//
//   t_r  = sum_{e in r} w_e * gw_e
//   gl_e = w_e * (gw_e - t_r)                               (plain form: grad_logits)
//   gz_e = gl_e * (z_e > 0 ? 1 : slope)
//   grad_s_dst[r] = sum_{e in r} gz_e     grad_s_src[c] = sum_{e: col_idx[e] = c} gz_e
//
// Partition: the token stream (token_items.h), one wavefront per item of `chunk` tokens, cut at
// the item's end (CutAtEnd), so a hub row is spread over as many waves as it has items and no
// wave walks more than `chunk` edges.  Within an item
//   * rows of at most kShort edges go to lane groups of kLR lanes through RowHandout, a row's
//     edges held in registers: one read of col_idx, one gather, one write of w;
//   * a longer piece goes to the whole wave, lane-strided: up to kRegPiece edges in registers
//     again, past that in three passes -- logits staged in w itself (each lane rereads what it
//     wrote), then the sum, then the division.
// A row that lies in one item is finished by that item.  A row cut over items leaves one
// partial per piece -- forward (max, sum of exp), backward t and the piece's sum of gz -- in
// the item's head slot (the continuation of the row before its first token) or tail slot (its
// last row, cut at the item's end); a fix-up, one thread per row, merges a row's slots in item
// order and hands the result back to every slot; a second walk over the cut pieces only
// normalises (forward: from the logits staged in w) or writes the gradients (backward).
// The column sums of the GAT backward walk the CSC of the transpose plan by the same items over
// col_ptr, gathering gz through csc_eid in slot order, with the same slots and fix-up.
//
// Every sum has a fixed order: a lane adds its elements in index order, lanes combine in a fixed
// butterfly, slots merge in item order.  No atomics, no allocation, copy or synchronisation.
// Results depend on chunk (the grouping of a row's sum), not on the run.
//
// Non-finite values follow IEEE through the formulas: the max drops NaN and the sum then carries
// it; exp(-inf) is 0; the one special value is a piece whose max is -inf, which subtracts 0
// instead (its terms are exp(-inf) = 0 either way; -inf - -inf would poison rows that hold
// finite logits elsewhere), and a row of nothing but -inf still ends as 0 / 0 = NaN.
#include <cmath>

#include "common.h"

namespace maxk {
namespace {

constexpr int kU = 4;                // whole-wave piece walk: wave steps of loads in flight
constexpr int kLR = 8;               // lanes per short row
constexpr int kNG = kWave / kLR;     // short rows per wave round
constexpr int kPer = 4;              // edges per lane of a short row
constexpr int kShort = kLR * kPer;   // a row of at most this many edges is a short row
constexpr int kMaxChunk = 1 << 24;   // pieces are walked with 32-bit offsets of 4-B elements

template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
    return __int_as_float(
        __builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}
struct Sum {
    static __device__ __forceinline__ float f(float a, float b) { return a + b; }
};
struct Max {  // fmaxf drops a NaN operand: the sums carry it
    static __device__ __forceinline__ float f(float a, float b) { return fmaxf(a, b); }
};
// Op over each aligned group of KG lanes (8 or 64), left in every lane of the group: the fixed
// butterfly of edge_grad.hip's group_sum, both lanes of a pair combining the same two numbers.
template <int KG, class Op>
__device__ __forceinline__ float lane_tree(float x) {
    x = Op::f(x, dpp_f<0xB1>(x));   // quad_perm [1,0,3,2]
    x = Op::f(x, dpp_f<0x4E>(x));   // quad_perm [2,3,0,1]
    x = Op::f(x, dpp_f<0x141>(x));  // row_half_mirror
    if constexpr (KG >= 16) x = Op::f(x, dpp_f<0x140>(x));  // row_mirror
    if constexpr (KG >= 32)
        x = Op::f(x, __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(x), 0x401F)));
    if constexpr (KG >= 64) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x),
                                                        false, false);
        x = Op::f(__uint_as_float(r[0]), __uint_as_float(r[1]));
    }
    return x;
}

// The value subtracted from a piece's logits: its max, or 0 for a piece of nothing but -inf.
__device__ __forceinline__ float shift_of(float m) { return m == -INFINITY ? 0.f : m; }

// The logit of an edge of one row: pointers are offset to the piece, i is 32-bit.
template <bool GAT>
struct Logits {
    const int32_t *__restrict__ col;   // GAT
    const float *__restrict__ s_src;   // GAT
    const float *__restrict__ lg;      // plain
    float sd, slope;
    __device__ __forceinline__ float z(int i) const { return sd + s_src[col[i]]; }
    __device__ __forceinline__ float at(int i) const {
        if constexpr (GAT) {
            const float v = z(i);
            return v > 0.f ? v : slope * v;
        } else {
            return lg[i];
        }
    }
};

// Per-row partials of the rows cut over items: slot 2i is item i's head (the continuation of
// the row before its first owned one), slot 2i + 1 its tail (its last owned row, cut at the
// item's end); row < 0: the item has no such piece.
struct Slots {
    int32_t *__restrict__ row;
    float *__restrict__ a;
    float *__restrict__ b;
};

__device__ __forceinline__ int item_of_wave(int n_items) {
    const int blk = MAXK_FWD_XCD ? xcd_contiguous_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int item = blk * kWavesPerBlock + (int)(threadIdx.x / kWave);
    return item < n_items ? item : -1;
}

// ---- whole-wave pieces (n edges, n >= 1, wave-uniform) --------------------------------------

// wp[i] = l_i; returns the piece's max.
template <bool GAT>
__device__ __forceinline__ float piece_logits(const Logits<GAT> &L, float *__restrict__ wp, int n,
                                              int lane) {
    float m = -INFINITY;
    for (int base = 0; base < n; base += kWave * kU) {
        float l[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = base + u * kWave + lane;
            l[u] = i < n ? L.at(i) : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = base + u * kWave + lane;
            if (i < n) wp[i] = l[u];
            m = fmaxf(m, l[u]);
        }
    }
    return lane_tree<kWave, Max>(m);
}

// sum_i exp(wp[i] - shift), wp holding the staged logits.
__device__ __forceinline__ float piece_expsum(const float *wp, float shift, int n, int lane) {
    float s = 0.f;
    for (int base = 0; base < n; base += kWave * kU) {
        float l[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = base + u * kWave + lane;
            l[u] = i < n ? wp[i] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) s += expf(l[u] - shift);  // past the end: exp(-inf) = 0
    }
    return lane_tree<kWave, Sum>(s);
}

// wp[i] = exp(wp[i] - shift) / s.
__device__ __forceinline__ void piece_normalise(float *wp, float shift, float s, int n, int lane) {
    for (int base = 0; base < n; base += kWave * kU) {
        float l[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = base + u * kWave + lane;
            l[u] = i < n ? wp[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = base + u * kWave + lane;
            if (i < n) wp[i] = expf(l[u] - shift) / s;
        }
    }
}

// sum_i w_i * gw_i.
__device__ __forceinline__ float piece_dot(const float *__restrict__ wp,
                                           const float *__restrict__ gp, int n, int lane) {
    float t = 0.f;
    for (int base = 0; base < n; base += kWave * kU) {
        float a[kU], b[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = base + u * kWave + lane;
            a[u] = i < n ? wp[i] : 0.f;
            b[u] = i < n ? gp[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) t += a[u] * b[u];
    }
    return lane_tree<kWave, Sum>(t);
}

// op[i] = gl_i (plain) or gz_i (GAT); returns the piece's sum of what it wrote.
template <bool GAT>
__device__ __forceinline__ float piece_emit(const Logits<GAT> &L, const float *__restrict__ wp,
                                            const float *__restrict__ gp, float t,
                                            float *__restrict__ op, int n, int lane) {
    float acc = 0.f;
    for (int base = 0; base < n; base += kWave * kU) {
        float g[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = base + u * kWave + lane;
            g[u] = 0.f;
            if (i < n) {
                g[u] = wp[i] * (gp[i] - t);
                if constexpr (GAT) g[u] *= L.z(i) > 0.f ? 1.f : L.slope;
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = base + u * kWave + lane;
            if (i < n) op[i] = g[u];
            acc += g[u];
        }
    }
    return lane_tree<kWave, Sum>(acc);
}

// sum over the CSC slots [0, n) of gz[eid[i]].
__device__ __forceinline__ float piece_gather(const float *__restrict__ gz,
                                              const int32_t *__restrict__ eid, int n, int lane) {
    float acc = 0.f;
    for (int base = 0; base < n; base += kWave * kU) {
        float g[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = base + u * kWave + lane;
            g[u] = i < n ? gz[(uint32_t)eid[i]] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) acc += g[u];
    }
    return lane_tree<kWave, Sum>(acc);
}

// ---- a whole-wave piece, either way ----------------------------------------------------------
// A piece of at most kRegPiece edges is held in registers, kReg per lane: every load of the
// piece is in flight at once and w is written once (against three passes for every piece:
// forward 1.007 -> 0.907 ms Reddit-sized, 1.756 -> 1.619 ms products-sized,
// profiles/r10/edge_softmax/).  A longer one takes the three passes above.

constexpr int kReg = 8;
constexpr int kRegPiece = kWave * kReg;

// (max, sum of exp) of the piece; `whole`: the piece is its row, w is finished; else w holds the
// logits for the second walk.
template <bool GAT>
__device__ __forceinline__ void piece_fwd(const Logits<GAT> &L, float *__restrict__ wp, int n,
                                          bool whole, int lane, float &m, float &s) {
    if (n > kRegPiece) {
        m = piece_logits<GAT>(L, wp, n, lane);
        s = piece_expsum(wp, shift_of(m), n, lane);
        if (whole) piece_normalise(wp, shift_of(m), s, n, lane);
        return;
    }
    float l[kReg];
    m = -INFINITY;
#pragma unroll
    for (int u = 0; u < kReg; ++u) {
        const int i = u * kWave + lane;
        l[u] = i < n ? L.at(i) : -INFINITY;
    }
#pragma unroll
    for (int u = 0; u < kReg; ++u) m = fmaxf(m, l[u]);
    m = lane_tree<kWave, Max>(m);
    const float shift = shift_of(m);
    float p[kReg];
    s = 0.f;
#pragma unroll
    for (int u = 0; u < kReg; ++u) {
        p[u] = expf(l[u] - shift);  // past the end: exp(-inf) = 0
        s += p[u];
    }
    s = lane_tree<kWave, Sum>(s);
#pragma unroll
    for (int u = 0; u < kReg; ++u) {
        const int i = u * kWave + lane;
        if (i < n) wp[i] = whole ? p[u] / s : l[u];
    }
}

// t of the piece; `whole`: the gradients are written too and their sum returned in acc.
template <bool GAT>
__device__ __forceinline__ void piece_bwd(const Logits<GAT> &L, const float *__restrict__ wp,
                                          const float *__restrict__ gp, float *__restrict__ op,
                                          int n, bool whole, int lane, float &t, float &acc) {
    acc = 0.f;
    if (n > kRegPiece) {
        t = piece_dot(wp, gp, n, lane);
        if (whole) acc = piece_emit<GAT>(L, wp, gp, t, op, n, lane);
        return;
    }
    float wv[kReg], gv[kReg], fac[kReg];
#pragma unroll
    for (int u = 0; u < kReg; ++u) {
        const int i = u * kWave + lane;
        wv[u] = i < n ? wp[i] : 0.f;
        gv[u] = i < n ? gp[i] : 0.f;
        fac[u] = 1.f;
        if constexpr (GAT)
            if (whole && i < n) fac[u] = L.z(i) > 0.f ? 1.f : L.slope;
    }
    t = 0.f;
#pragma unroll
    for (int u = 0; u < kReg; ++u) t += wv[u] * gv[u];
    t = lane_tree<kWave, Sum>(t);
    if (!whole) return;  // wave-uniform
#pragma unroll
    for (int u = 0; u < kReg; ++u) {
        const int i = u * kWave + lane;
        float v = wv[u] * (gv[u] - t);  // a lane without an edge: 0 * (0 - t), not stored
        if constexpr (GAT) v *= fac[u];
        if (i < n) {
            op[i] = v;
            acc += v;
        }
    }
    acc = lane_tree<kWave, Sum>(acc);
}

// ---- short rows: one row per lane group, its edges in registers ------------------------------

// The cut row a group took (at most one per item: the item's last), as wave-uniform values.
struct Tail {
    int row;
    float a, b;
};
__device__ __forceinline__ void tail_from_group(Tail &t, int crow, float ca, float cb) {
    const uint64_t m = __ballot(crow >= 0);
    if (!m) return;
    const int src = __builtin_ctzll(m);
    t.row = __shfl(crow, src);
    t.a = __shfl(ca, src);
    t.b = __shfl(cb, src);
}

// Forward over the short rows from `first` on; returns the first row not taken.  A whole row is
// finished; a cut one leaves its logits in w and its (max, sum) in `tail`.
template <bool GAT>
__device__ __forceinline__ int short_rows_fwd(const int32_t *__restrict__ row_ptr,
                                              const int32_t *__restrict__ col_idx,
                                              const float *__restrict__ s_dst,
                                              const float *__restrict__ s_src,
                                              const float *__restrict__ logits, float slope,
                                              float *__restrict__ w, int num_rows, int first,
                                              int64_t d1, int lane, Tail &tail) {
    const int g = lane / kLR, j = lane % kLR;
    RowHandout<CutAtEnd> h(row_ptr, num_rows, first, d1, kShort, lane);
    int crow = -1;
    float cm = 0.f, cs = 0.f;
    for (;;) {
        int row = -1, b = 0, e = 0;
        h.template assign<1>(true, kNG, kLR, g, lane, [&](int r, int rb, int re) {
            row = r;
            b = rb;
            e = re;
        });
        if (!__ballot(row >= 0)) break;
        const bool has = row >= 0;
        const int n = has ? e - b : 0;  // this lane's row piece: [b, b + n)
        const int full = has ? row_ptr[row + 1] : 0;
        const Logits<GAT> L{col_idx, s_src, logits, GAT && has ? s_dst[row] : 0.f, slope};
        float l[kPer], m = -INFINITY;
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int o = j + kLR * u;  // offsets, not indices: b + o may pass 2^31 past e
            l[u] = o < n ? L.at(b + o) : -INFINITY;
            m = fmaxf(m, l[u]);
        }
        m = lane_tree<kLR, Max>(m);
        const float shift = shift_of(m);
        float p[kPer], s = 0.f;
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            p[u] = expf(l[u] - shift);  // a lane without an edge: exp(-inf) = 0
            s += p[u];
        }
        s = lane_tree<kLR, Sum>(s);
        const bool cut = has && e < full;
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int o = j + kLR * u;
            if (o < n) w[b + o] = cut ? l[u] : p[u] / s;
        }
        if (cut && e > b) {
            crow = row;
            cm = m;
            cs = s;
        }
    }
    tail_from_group(tail, crow, cm, cs);
    return h.next;
}

// Backward over the short rows: a whole row writes its gradients and (GAT) grad_s_dst, 0 for a
// row without edges; a cut one leaves t in `tail`.
template <bool GAT>
__device__ __forceinline__ int short_rows_bwd(const int32_t *__restrict__ row_ptr,
                                              const int32_t *__restrict__ col_idx,
                                              const float *__restrict__ s_dst,
                                              const float *__restrict__ s_src, float slope,
                                              const float *__restrict__ w,
                                              const float *__restrict__ gw,
                                              float *__restrict__ out,
                                              float *__restrict__ grad_s_dst, int num_rows,
                                              int first, int64_t d1, int lane, Tail &tail) {
    const int g = lane / kLR, j = lane % kLR;
    RowHandout<CutAtEnd> h(row_ptr, num_rows, first, d1, kShort, lane);
    int crow = -1;
    float ct = 0.f;
    for (;;) {
        int row = -1, b = 0, e = 0;
        h.template assign<1>(true, kNG, kLR, g, lane, [&](int r, int rb, int re) {
            row = r;
            b = rb;
            e = re;
        });
        if (!__ballot(row >= 0)) break;
        const bool has = row >= 0;
        const int n = has ? e - b : 0;  // this lane's row piece: [b, b + n)
        const int full = has ? row_ptr[row + 1] : 0;
        const Logits<GAT> L{col_idx, s_src, nullptr, GAT && has ? s_dst[row] : 0.f, slope};
        float wv[kPer], gv[kPer], t = 0.f;
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int o = j + kLR * u;
            wv[u] = o < n ? w[b + o] : 0.f;
            gv[u] = o < n ? gw[b + o] : 0.f;
            t += wv[u] * gv[u];
        }
        t = lane_tree<kLR, Sum>(t);
        const bool cut = has && e < full;
        float acc = 0.f;
        if (!cut) {
#pragma unroll
            for (int u = 0; u < kPer; ++u) {
                const int o = j + kLR * u;
                if (o < n) {
                    float v = wv[u] * (gv[u] - t);
                    if constexpr (GAT) v *= L.z(b + o) > 0.f ? 1.f : slope;
                    out[b + o] = v;
                    acc += v;
                }
            }
        }
        acc = lane_tree<kLR, Sum>(acc);
        if constexpr (GAT)
            if (has && !cut && j == 0) grad_s_dst[row] = acc;
        if (cut && e > b) {
            crow = row;
            ct = t;
        }
    }
    tail_from_group(tail, crow, ct, 0.f);
    return h.next;
}

// Column sums over the short columns of the CSC: a whole column writes grad_s_src, 0 for an
// unread one; a cut one leaves its partial in `tail`.
__device__ __forceinline__ int short_cols_sum(const int32_t *__restrict__ col_ptr,
                                              const int32_t *__restrict__ eid,
                                              const float *__restrict__ gz,
                                              float *__restrict__ grad_s_src, int num_cols,
                                              int first, int64_t d1, int lane, Tail &tail) {
    const int g = lane / kLR, j = lane % kLR;
    RowHandout<CutAtEnd> h(col_ptr, num_cols, first, d1, kShort, lane);
    int crow = -1;
    float ca = 0.f;
    for (;;) {
        int row = -1, b = 0, e = 0;
        h.template assign<1>(true, kNG, kLR, g, lane, [&](int r, int rb, int re) {
            row = r;
            b = rb;
            e = re;
        });
        if (!__ballot(row >= 0)) break;
        const bool has = row >= 0;
        const int n = has ? e - b : 0;  // this lane's row piece: [b, b + n)
        const int full = has ? col_ptr[row + 1] : 0;
        float acc = 0.f;
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int o = j + kLR * u;
            acc += o < n ? gz[(uint32_t)eid[b + o]] : 0.f;
        }
        acc = lane_tree<kLR, Sum>(acc);
        const bool cut = has && e < full;
        if (has && !cut && j == 0) grad_s_src[row] = acc;
        if (cut && e > b) {
            crow = row;
            ca = acc;
        }
    }
    tail_from_group(tail, crow, ca, 0.f);
    return h.next;
}

__device__ __forceinline__ void store_slots(const Slots &sl, int item, const Tail &head,
                                            const Tail &tail, int lane) {
    if (lane != 0) return;
    sl.row[2 * item] = head.row;
    sl.a[2 * item] = head.a;
    sl.b[2 * item] = head.b;
    sl.row[2 * item + 1] = tail.row;
    sl.a[2 * item + 1] = tail.a;
    sl.b[2 * item + 1] = tail.b;
}

// ---- forward ---------------------------------------------------------------------------------

template <bool GAT>
__global__ __launch_bounds__(kBlock) void esm_fwd_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const float *__restrict__ s_dst, const float *__restrict__ s_src,
    const float *__restrict__ logits, float slope, float *__restrict__ w, Slots sl, int num_rows,
    int64_t num_e, int chunk, int n_items) {
    const int item = item_of_wave(n_items);
    if (item < 0) return;  // whole wave; no workgroup barrier below
    const int lane = lane_id();
    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);
    Tail head{-1, 0.f, 0.f}, tail{-1, 0.f, 0.f};

    // (max, sum) of row q's piece [sb, se); whole: w finished, else the logits left in w
    auto walk = [&](int q, int64_t sb, int64_t se, bool whole, float &m, float &s) {
        const Logits<GAT> L{col_idx + sb, s_src, logits + sb, GAT ? s_dst[q] : 0.f, slope};
        piece_fwd<GAT>(L, w + sb, (int)(se - sb), whole, lane, m, s);
    };

    if (it.r > 0) {  // the tail of row r - 1, whose token precedes the item
        const RowPiece p = cont_piece(CutAtEnd{}, it.p_lo, it.d1, it.r, row_ptr[it.r]);
        if (p.sb < p.se) {
            head.row = it.r - 1;
            walk(head.row, p.sb, p.se, false, head.a, head.b);
        }
    }
    int q = it.r;
    while (q < num_rows) {
        q = short_rows_fwd<GAT>(row_ptr, col_idx, s_dst, s_src, logits, slope, w, num_rows, q,
                                it.d1, lane, tail);
        if (q >= num_rows) break;
        const int64_t rb = row_ptr[q];
        if (!row_owned(it.d1, q, rb)) break;  // row q's token belongs to a later item
        const int64_t re = row_ptr[q + 1];
        const RowPiece p = row_piece(CutAtEnd{}, it.d1, q, rb, re);
        if (p.sb < p.se) {
            float m, s;
            walk(q, p.sb, p.se, p.se == re, m, s);
            if (p.se < re) tail = Tail{q, m, s};
        }
        ++q;
    }
    store_slots(sl, item, head, tail, lane);
}

// The second walk: the cut pieces only, w = exp(l - max of the row) / sum of the row.
__global__ __launch_bounds__(kBlock) void esm_normalise_kernel(
    const int32_t *__restrict__ row_ptr, float *__restrict__ w, Slots sl, int num_rows,
    int64_t num_e, int chunk, int n_items) {
    const int item = item_of_wave(n_items);
    if (item < 0) return;
    const int lane = lane_id();
    const int64_t total = (int64_t)num_rows + num_e;
    const int64_t d0 = (int64_t)item * chunk;
    const int64_t d1 = d0 + chunk < total ? d0 + chunk : total;
    const int hrow = sl.row[2 * item];
    if (hrow >= 0) {
        const int r = hrow + 1;
        const RowPiece p = cont_piece(CutAtEnd{}, d0 - r, d1, r, row_ptr[r]);
        piece_normalise(w + p.sb, shift_of(sl.a[2 * item]), sl.b[2 * item], (int)(p.se - p.sb),
                        lane);
    }
    const int trow = sl.row[2 * item + 1];
    if (trow >= 0) {
        const RowPiece p = row_piece(CutAtEnd{}, d1, trow, row_ptr[trow], row_ptr[trow + 1]);
        piece_normalise(w + p.sb, shift_of(sl.a[2 * item + 1]), sl.b[2 * item + 1],
                        (int)(p.se - p.sb), lane);
    }
}

// ---- the merge of a cut row's slots ----------------------------------------------------------

constexpr int kMergeSoftmax = 0;  // (a, b) = (max, sum of exp) -> the row's, back into every slot
constexpr int kMergeShare = 1;    // a = a partial sum -> the row's sum, back into every slot's a
constexpr int kMergeOut = 2;      // val = a partial sum -> out[row] = the row's sum

// One thread per slot; the thread of a row's first slot merges the row's slots in item order.
// A row's slots are its tail slot (if its owner holds some of its edges) and then the head slots
// of the items after it.
template <int MODE>
__global__ __launch_bounds__(kBlock) void esm_merge_kernel(Slots sl, float *__restrict__ val,
                                                           float *__restrict__ out, int n_slots) {
    const int s0 = (int)(blockIdx.x * (int64_t)kBlock + threadIdx.x);
    if (s0 >= n_slots) return;
    const int row = sl.row[s0];
    if (row < 0) return;
    if (!(s0 & 1)) {  // a head slot starts a row only when the row's owner holds none of it
        if (s0 >= 1 && sl.row[s0 - 1] == row) return;
        if (s0 >= 2 && sl.row[s0 - 2] == row) return;
    }
    const int s1 = s0 + 1 + !(s0 & 1);  // the next head slot
    auto more = [&](int s) { return s < n_slots && sl.row[s] == row; };
    if constexpr (MODE == kMergeSoftmax) {
        float m = sl.a[s0];
        for (int s = s1; more(s); s += 2) m = fmaxf(m, sl.a[s]);
        // a piece of nothing but -inf has sum 0 (or NaN) and scale exp(-inf) = 0
        const float shift = shift_of(m);
        float sum = sl.b[s0] * expf(sl.a[s0] - shift);
        for (int s = s1; more(s); s += 2) sum += sl.b[s] * expf(sl.a[s] - shift);
        sl.a[s0] = m;
        sl.b[s0] = sum;
        for (int s = s1; more(s); s += 2) {
            sl.a[s] = m;
            sl.b[s] = sum;
        }
    } else {
        float sum = val[s0];
        for (int s = s1; more(s); s += 2) sum += val[s];
        if constexpr (MODE == kMergeShare) {
            val[s0] = sum;
            for (int s = s1; more(s); s += 2) val[s] = sum;
        } else {
            out[row] = sum;
        }
    }
}

// ---- backward --------------------------------------------------------------------------------

// First walk: t of every piece; a row inside one item is finished (gradients written, and for
// GAT grad_s_dst, 0 for a row without edges), a cut piece leaves t in its slot.
template <bool GAT>
__global__ __launch_bounds__(kBlock) void esm_bwd_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const float *__restrict__ s_dst, const float *__restrict__ s_src, float slope,
    const float *__restrict__ w, const float *__restrict__ gw, float *__restrict__ out,
    float *__restrict__ grad_s_dst, Slots sl, int num_rows, int64_t num_e, int chunk,
    int n_items) {
    const int item = item_of_wave(n_items);
    if (item < 0) return;
    const int lane = lane_id();
    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);
    Tail head{-1, 0.f, 0.f}, tail{-1, 0.f, 0.f};
    if (it.r > 0) {
        const RowPiece p = cont_piece(CutAtEnd{}, it.p_lo, it.d1, it.r, row_ptr[it.r]);
        if (p.sb < p.se) {
            head.row = it.r - 1;
            float acc;
            piece_bwd<GAT>(Logits<GAT>{}, w + p.sb, gw + p.sb, nullptr, (int)(p.se - p.sb), false,
                           lane, head.a, acc);
        }
    }
    int q = it.r;
    while (q < num_rows) {
        q = short_rows_bwd<GAT>(row_ptr, col_idx, s_dst, s_src, slope, w, gw, out, grad_s_dst,
                                num_rows, q, it.d1, lane, tail);
        if (q >= num_rows) break;
        const int64_t rb = row_ptr[q];
        if (!row_owned(it.d1, q, rb)) break;
        const int64_t re = row_ptr[q + 1];
        const RowPiece p = row_piece(CutAtEnd{}, it.d1, q, rb, re);
        const int n = (int)(p.se - p.sb);
        if (n > 0) {
            const Logits<GAT> L{col_idx + p.sb, s_src, nullptr, GAT ? s_dst[q] : 0.f, slope};
            float t, acc;
            piece_bwd<GAT>(L, w + p.sb, gw + p.sb, out + p.sb, n, p.se == re, lane, t, acc);
            if (p.se == re) {
                if constexpr (GAT)
                    if (lane == 0) grad_s_dst[q] = acc;
            } else {
                tail = Tail{q, t, 0.f};
            }
        } else if (GAT && re == rb && lane == 0) {
            grad_s_dst[q] = 0.f;
        }
        ++q;
    }
    store_slots(sl, item, head, tail, lane);
}

// Second walk: the cut pieces' gradients from the row's t (slot a); the piece's sum of gz goes
// to slot b (GAT).
template <bool GAT>
__global__ __launch_bounds__(kBlock) void esm_bwd_emit_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const float *__restrict__ s_dst, const float *__restrict__ s_src, float slope,
    const float *__restrict__ w, const float *__restrict__ gw, float *__restrict__ out, Slots sl,
    int num_rows, int64_t num_e, int chunk, int n_items) {
    const int item = item_of_wave(n_items);
    if (item < 0) return;
    const int lane = lane_id();
    const int64_t total = (int64_t)num_rows + num_e;
    const int64_t d0 = (int64_t)item * chunk;
    const int64_t d1 = d0 + chunk < total ? d0 + chunk : total;
    auto emit = [&](int slot, int row, const RowPiece &p) {
        const Logits<GAT> L{col_idx + p.sb, s_src, nullptr, GAT ? s_dst[row] : 0.f, slope};
        const float acc = piece_emit<GAT>(L, w + p.sb, gw + p.sb, sl.a[slot], out + p.sb,
                                          (int)(p.se - p.sb), lane);
        if (lane == 0) sl.b[slot] = acc;
    };
    const int hrow = sl.row[2 * item];
    if (hrow >= 0) {
        const int r = hrow + 1;
        emit(2 * item, hrow, cont_piece(CutAtEnd{}, d0 - r, d1, r, row_ptr[r]));
    }
    const int trow = sl.row[2 * item + 1];
    if (trow >= 0)
        emit(2 * item + 1, trow,
             row_piece(CutAtEnd{}, d1, trow, row_ptr[trow], row_ptr[trow + 1]));
}

// grad_s_src[c] = the sum of gz over column c's CSC slots, in slot order; a cut column leaves
// its partials in the slots.
__global__ __launch_bounds__(kBlock) void esm_colsum_kernel(
    const int32_t *__restrict__ col_ptr, const int32_t *__restrict__ eid,
    const float *__restrict__ gz, float *__restrict__ grad_s_src, Slots sl, int num_cols,
    int64_t num_e, int chunk, int n_items) {
    const int item = item_of_wave(n_items);
    if (item < 0) return;
    const int lane = lane_id();
    const ItemRange it = item_range(col_ptr, num_cols, num_e, item, chunk);
    Tail head{-1, 0.f, 0.f}, tail{-1, 0.f, 0.f};
    if (it.r > 0) {
        const RowPiece p = cont_piece(CutAtEnd{}, it.p_lo, it.d1, it.r, col_ptr[it.r]);
        if (p.sb < p.se) {
            head.row = it.r - 1;
            head.a = piece_gather(gz, eid + p.sb, (int)(p.se - p.sb), lane);
        }
    }
    int c = it.r;
    while (c < num_cols) {
        c = short_cols_sum(col_ptr, eid, gz, grad_s_src, num_cols, c, it.d1, lane, tail);
        if (c >= num_cols) break;
        const int64_t cb = col_ptr[c];
        if (!row_owned(it.d1, c, cb)) break;
        const int64_t ce = col_ptr[c + 1];
        const RowPiece p = row_piece(CutAtEnd{}, it.d1, c, cb, ce);
        const int n = (int)(p.se - p.sb);
        if (n > 0) {
            const float acc = piece_gather(gz, eid + p.sb, n, lane);
            if (p.se == ce) {
                if (lane == 0) grad_s_src[c] = acc;
            } else {
                tail = Tail{c, acc, 0.f};
            }
        } else if (ce == cb && lane == 0) {
            grad_s_src[c] = 0.f;
        }
        ++c;
    }
    store_slots(sl, item, head, tail, lane);
}

// ---- host ------------------------------------------------------------------------------------

// Items per launch the auto rule aims at: 8 per resident wave slot (32 per CU).
int64_t auto_items() { return device_cus() * 32 * 8; }

// chunk_edges = 0: the forward's rule for large graphs, about auto_items() items of 256 to 2048
// tokens.  (Its one-round sizing of small graphs, down to 64 tokens, is left out: an item here is
// a few loads per token, not a chain of dependent record gathers.)
int esm_chunk(int64_t tokens, int chunk) {
    if (chunk > 0) return chunk < kMaxChunk ? chunk : kMaxChunk;
    const int64_t c = ceil_div(tokens, auto_items());
    return (int)(c < 256 ? 256 : c > 2048 ? 2048 : c);
}

// Slot capacity, in items: at least token_items(.., esm_chunk(..)) and non-decreasing in the
// token count, which the item count of the auto rule is not (one token more can make the items
// one token longer and fewer).
int64_t esm_item_cap(int64_t tokens, int chunk) {
    if (chunk > 0) return token_items(tokens, 0, esm_chunk(tokens, chunk));
    const int64_t k = auto_items();
    const int64_t lo = ceil_div(tokens, 256) < k ? ceil_div(tokens, 256) : k;
    const int64_t hi = ceil_div(tokens, 2048);
    const int64_t cap = lo > hi ? lo : hi;
    return cap > 0 ? cap : 1;
}

// Workspace: the row slots [row | a | b], and for the GAT backward gz[num_e] and the column
// slots.
struct SlotLayout {
    int chunk, n_items;
    size_t row_off, a_off, b_off, end;
};
SlotLayout slot_layout(int64_t n, int64_t num_e, int chunk, size_t base) {
    SlotLayout L{};
    L.chunk = esm_chunk(n + num_e, chunk);
    L.n_items = token_items(n, num_e, L.chunk);
    const size_t bytes = al256((size_t)esm_item_cap(n + num_e, chunk) * 2 * sizeof(float));
    L.row_off = base;
    L.a_off = L.row_off + bytes;
    L.b_off = L.a_off + bytes;
    L.end = L.b_off + bytes;
    return L;
}
Slots slots_at(void *ws, const SlotLayout &L) {
    uint8_t *p = reinterpret_cast<uint8_t *>(ws);
    return Slots{reinterpret_cast<int32_t *>(p + L.row_off), reinterpret_cast<float *>(p + L.a_off),
                 reinterpret_cast<float *>(p + L.b_off)};
}
struct GatBwdLayout {
    SlotLayout rows, cols;
    size_t gz_off, total;
};
GatBwdLayout gat_bwd_layout(int64_t num_rows, int64_t num_cols, int64_t num_e, int chunk) {
    GatBwdLayout G{};
    G.rows = slot_layout(num_rows, num_e, chunk, 0);
    G.gz_off = G.rows.end;
    G.cols = slot_layout(num_cols, num_e, chunk, G.gz_off + al256((size_t)num_e * sizeof(float)));
    G.total = G.cols.end;
    return G;
}

dim3 item_grid(int n_items) {
    const int64_t blocks = ceil_div(n_items, kWavesPerBlock);
    return dim3((unsigned)(MAXK_FWD_XCD ? xcd_grid(blocks) : blocks));
}
dim3 slot_grid(int n_items) { return dim3((unsigned)ceil_div(2 * (int64_t)n_items, kBlock)); }

int check_sizes(int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t chunk_edges) {
    MAXK_REQUIRE(num_rows >= 0 && num_rows < (1LL << 31), "num_rows out of range: %lld",
                 (long long)num_rows);
    MAXK_REQUIRE(num_cols >= 0 && num_cols < (1LL << 31), "num_cols out of range: %lld",
                 (long long)num_cols);
    MAXK_REQUIRE(num_e >= 0 && num_e < (1LL << 31), "num_e out of range: %lld", (long long)num_e);
    MAXK_REQUIRE(chunk_edges >= 0, "chunk_edges must be >= 0");
    return MAXK_OK;
}
int check_slope(float slope) {
    MAXK_REQUIRE(slope >= 0.f && slope <= 1.f, "negative_slope must be in [0, 1], got %g",
                 (double)slope);  // a NaN fails both comparisons
    return MAXK_OK;
}
int check_workspace(const void *workspace, size_t bytes, size_t need) {
    MAXK_REQUIRE(workspace && bytes >= need, "workspace too small: need %zu bytes, got %zu", need,
                 workspace ? bytes : (size_t)0);
    MAXK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-B aligned");
    return MAXK_OK;
}
bool sizes_ok(int64_t num_rows, int64_t num_cols, int64_t num_e) {
    return num_rows >= 0 && num_cols >= 0 && num_e >= 0;
}

template <bool GAT>
int launch_fwd(const int32_t *row_ptr, const int32_t *col_idx, const float *s_dst,
               const float *s_src, const float *logits, float slope, float *w, int64_t num_rows,
               int64_t num_e, int32_t chunk_edges, void *workspace, hipStream_t s) {
    const SlotLayout L = slot_layout(num_rows, num_e, chunk_edges, 0);
    const Slots sl = slots_at(workspace, L);
    hipLaunchKernelGGL(esm_fwd_kernel<GAT>, item_grid(L.n_items), dim3(kBlock), 0, s, row_ptr,
                       col_idx, s_dst, s_src, logits, slope, w, sl, (int)num_rows, num_e, L.chunk,
                       L.n_items);
    MAXK_LAUNCHED("esm_fwd_kernel");
    hipLaunchKernelGGL(esm_merge_kernel<kMergeSoftmax>, slot_grid(L.n_items), dim3(kBlock), 0, s,
                       sl, (float *)nullptr, (float *)nullptr, 2 * L.n_items);
    MAXK_LAUNCHED("esm_merge_kernel");
    hipLaunchKernelGGL(esm_normalise_kernel, item_grid(L.n_items), dim3(kBlock), 0, s, row_ptr, w,
                       sl, (int)num_rows, num_e, L.chunk, L.n_items);
    MAXK_LAUNCHED("esm_normalise_kernel");
    return MAXK_OK;
}

// The row side of the backward: out = grad_logits (plain) or gz (GAT), and for GAT grad_s_dst.
template <bool GAT>
int launch_bwd_rows(const int32_t *row_ptr, const int32_t *col_idx, const float *s_dst,
                    const float *s_src, float slope, const float *w, const float *gw, float *out,
                    float *grad_s_dst, int64_t num_rows, int64_t num_e, const SlotLayout &L,
                    void *workspace, hipStream_t s) {
    const Slots sl = slots_at(workspace, L);
    hipLaunchKernelGGL(esm_bwd_kernel<GAT>, item_grid(L.n_items), dim3(kBlock), 0, s, row_ptr,
                       col_idx, s_dst, s_src, slope, w, gw, out, grad_s_dst, sl, (int)num_rows,
                       num_e, L.chunk, L.n_items);
    MAXK_LAUNCHED("esm_bwd_kernel");
    hipLaunchKernelGGL(esm_merge_kernel<kMergeShare>, slot_grid(L.n_items), dim3(kBlock), 0, s, sl,
                       sl.a, (float *)nullptr, 2 * L.n_items);
    MAXK_LAUNCHED("esm_merge_kernel");
    hipLaunchKernelGGL(esm_bwd_emit_kernel<GAT>, item_grid(L.n_items), dim3(kBlock), 0, s, row_ptr,
                       col_idx, s_dst, s_src, slope, w, gw, out, sl, (int)num_rows, num_e, L.chunk,
                       L.n_items);
    MAXK_LAUNCHED("esm_bwd_emit_kernel");
    if constexpr (GAT) {
        hipLaunchKernelGGL(esm_merge_kernel<kMergeOut>, slot_grid(L.n_items), dim3(kBlock), 0, s,
                           sl, sl.b, grad_s_dst, 2 * L.n_items);
        MAXK_LAUNCHED("esm_merge_kernel");
    }
    return MAXK_OK;
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" size_t maxk_edge_softmax_workspace_size(int64_t num_rows, int64_t num_cols,
                                                   int64_t num_e, int32_t chunk_edges) {
    if (!sizes_ok(num_rows, num_cols, num_e) || chunk_edges < 0) return 0;
    return slot_layout(num_rows, num_e, chunk_edges, 0).end;
}

extern "C" size_t maxk_edge_softmax_backward_workspace_size(int64_t num_rows, int64_t num_cols,
                                                            int64_t num_e, int32_t chunk_edges) {
    return maxk_edge_softmax_workspace_size(num_rows, num_cols, num_e, chunk_edges);
}

extern "C" size_t maxk_gat_edge_softmax_workspace_size(int64_t num_rows, int64_t num_cols,
                                                       int64_t num_e, int32_t chunk_edges) {
    return maxk_edge_softmax_workspace_size(num_rows, num_cols, num_e, chunk_edges);
}

extern "C" size_t maxk_gat_edge_softmax_backward_workspace_size(int64_t num_rows,
                                                                int64_t num_cols, int64_t num_e,
                                                                int32_t chunk_edges) {
    if (!sizes_ok(num_rows, num_cols, num_e) || chunk_edges < 0) return 0;
    return gat_bwd_layout(num_rows, num_cols, num_e, chunk_edges).total;
}

extern "C" int maxk_edge_softmax(const int32_t *row_ptr, const float *logits, float *w,
                                 int64_t num_rows, int64_t num_cols, int64_t num_e,
                                 int32_t chunk_edges, void *workspace, size_t workspace_bytes,
                                 void *stream) {
    clear_error();
    if (int rc = check_sizes(num_rows, num_cols, num_e, chunk_edges)) return rc;
    if (num_e == 0) return MAXK_OK;  // no edge, nothing to write
    MAXK_REQUIRE(num_rows > 0, "edges present but num_rows == 0");
    MAXK_REQUIRE(row_ptr && logits && w, "row_ptr / logits / w must not be NULL");
    if (int rc = check_workspace(workspace, workspace_bytes,
                                 slot_layout(num_rows, num_e, chunk_edges, 0).end))
        return rc;
    return launch_fwd<false>(row_ptr, nullptr, nullptr, nullptr, logits, 0.f, w, num_rows, num_e,
                             chunk_edges, workspace, as_stream(stream));
}

extern "C" int maxk_edge_softmax_backward(const int32_t *row_ptr, const float *w,
                                          const float *grad_w, float *grad_logits,
                                          int64_t num_rows, int64_t num_cols, int64_t num_e,
                                          int32_t chunk_edges, void *workspace,
                                          size_t workspace_bytes, void *stream) {
    clear_error();
    if (int rc = check_sizes(num_rows, num_cols, num_e, chunk_edges)) return rc;
    if (num_e == 0) return MAXK_OK;
    MAXK_REQUIRE(num_rows > 0, "edges present but num_rows == 0");
    MAXK_REQUIRE(row_ptr && w && grad_w && grad_logits,
                 "row_ptr / w / grad_w / grad_logits must not be NULL");
    const SlotLayout L = slot_layout(num_rows, num_e, chunk_edges, 0);
    if (int rc = check_workspace(workspace, workspace_bytes, L.end)) return rc;
    return launch_bwd_rows<false>(row_ptr, nullptr, nullptr, nullptr, 0.f, w, grad_w, grad_logits,
                                  nullptr, num_rows, num_e, L, workspace, as_stream(stream));
}

extern "C" int maxk_gat_edge_softmax(const int32_t *row_ptr, const int32_t *col_idx,
                                     const float *s_dst, const float *s_src, float negative_slope,
                                     float *w, int64_t num_rows, int64_t num_cols, int64_t num_e,
                                     int32_t chunk_edges, void *workspace, size_t workspace_bytes,
                                     void *stream) {
    clear_error();
    if (int rc = check_sizes(num_rows, num_cols, num_e, chunk_edges)) return rc;
    if (int rc = check_slope(negative_slope)) return rc;
    if (num_e == 0) return MAXK_OK;
    MAXK_REQUIRE(num_rows > 0 && num_cols > 0, "edges present but num_rows or num_cols == 0");
    MAXK_REQUIRE(row_ptr && col_idx && s_dst && s_src && w,
                 "row_ptr / col_idx / s_dst / s_src / w must not be NULL");
    if (int rc = check_workspace(workspace, workspace_bytes,
                                 slot_layout(num_rows, num_e, chunk_edges, 0).end))
        return rc;
    return launch_fwd<true>(row_ptr, col_idx, s_dst, s_src, nullptr, negative_slope, w, num_rows,
                            num_e, chunk_edges, workspace, as_stream(stream));
}

extern "C" int maxk_gat_edge_softmax_backward(
    const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr,
    const int32_t *csc_eid, const float *s_dst, const float *s_src, float negative_slope,
    const float *w, const float *grad_w, float *grad_s_dst, float *grad_s_src, int64_t num_rows,
    int64_t num_cols, int64_t num_e, int32_t chunk_edges, void *workspace, size_t workspace_bytes,
    void *stream) {
    clear_error();
    if (int rc = check_sizes(num_rows, num_cols, num_e, chunk_edges)) return rc;
    if (int rc = check_slope(negative_slope)) return rc;
    MAXK_REQUIRE((grad_s_dst || num_rows == 0) && (grad_s_src || num_cols == 0),
                 "grad_s_dst / grad_s_src must not be NULL");
    hipStream_t s = as_stream(stream);
    if (num_e == 0) {  // no edge: both gradients are zeros
        if (int rc = zero_words(grad_s_dst, num_rows, s)) return rc;
        return zero_words(grad_s_src, num_cols, s);
    }
    MAXK_REQUIRE(num_rows > 0 && num_cols > 0, "edges present but num_rows or num_cols == 0");
    MAXK_REQUIRE(row_ptr && col_idx && col_ptr && csc_eid && s_dst && s_src && w && grad_w,
                 "CSR / CSC / score / w / grad_w pointers must not be NULL");
    const GatBwdLayout G = gat_bwd_layout(num_rows, num_cols, num_e, chunk_edges);
    if (int rc = check_workspace(workspace, workspace_bytes, G.total)) return rc;
    float *gz = reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(workspace) + G.gz_off);
    if (int rc = launch_bwd_rows<true>(row_ptr, col_idx, s_dst, s_src, negative_slope, w, grad_w,
                                       gz, grad_s_dst, num_rows, num_e, G.rows, workspace, s))
        return rc;
    const Slots csl = slots_at(workspace, G.cols);
    hipLaunchKernelGGL(esm_colsum_kernel, item_grid(G.cols.n_items), dim3(kBlock), 0, s, col_ptr,
                       csc_eid, gz, grad_s_src, csl, (int)num_cols, num_e, G.cols.chunk,
                       G.cols.n_items);
    MAXK_LAUNCHED("esm_colsum_kernel");
    hipLaunchKernelGGL(esm_merge_kernel<kMergeOut>, slot_grid(G.cols.n_items), dim3(kBlock), 0, s,
                       csl, csl.a, grad_s_src, 2 * G.cols.n_items);
    MAXK_LAUNCHED("esm_merge_kernel");
    return MAXK_OK;
}
