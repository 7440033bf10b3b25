// The device helpers and host-side layouts the edge softmax kernels share: edge_softmax.hip (one
// head) and edge_softmax_heads.hip (H heads over one walk).  The scheme is described at the top
// of edge_softmax.hip.
#pragma once

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

// ---- the merge of a cut row's slots ----------------------------------------------------------

constexpr int kMergeSoftmax = 0;  // (a, b) = (max, sum of exp) -> the row's, back into every slot
constexpr int kMergeShare = 1;    // a = a partial sum -> the row's sum, back into every slot's a
constexpr int kMergeOut = 2;      // val = a partial sum -> out[row] = the row's sum

// One thread per slot; the thread of a row's first slot merges the row's slots in item order.
// A row's slots are its tail slot (if its owner holds some of its edges) and then the head slots
// of the items after it.
template <int MODE>
__device__ __forceinline__ void merge_slots(const Slots &sl, float *__restrict__ val,
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
template <int MODE>
__global__ __launch_bounds__(kBlock) void esm_merge_kernel(Slots sl, float *__restrict__ val,
                                                           float *__restrict__ out, int n_slots) {
    merge_slots<MODE>(sl, val, out, n_slots);
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
inline SlotLayout slot_layout(int64_t n, int64_t num_e, int chunk, size_t base) {
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
dim3 item_grid(int n_items) {
    const int64_t blocks = ceil_div(n_items, kWavesPerBlock);
    return dim3((unsigned)(MAXK_FWD_XCD ? xcd_grid(blocks) : blocks));
}
inline dim3 slot_grid(int n_items) { return dim3((unsigned)ceil_div(2 * (int64_t)n_items, kBlock)); }

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

}  // namespace
}  // namespace maxk
