// The device helpers and host-side layouts the edge softmax kernels share: edge_softmax.hip (one
// head) and edge_softmax_heads.hip (H heads over one walk).  The scheme is described at the top
// of edge_softmax.hip.  The last section (H heads) also serves the fused attention's two files,
// gat_attention_heads.hip and gat_attention_heads_bwd.hip.
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
// Op over each aligned group of KG lanes (8 .. 64), left in every lane of the group: a butterfly
// of fixed shape, both lanes of a pair combining the same two numbers, so the group agrees bitwise
// and the order is the same every run.
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
inline dim3 slot_grid(int n_items) { return dim3((unsigned)ceil_div(2 * (int64_t)n_items, kBlock)); }

// inline, as check_slope and check_workspace: not every unit that includes this has such an entry
inline int check_sizes(int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t chunk_edges) {
    MAXK_REQUIRE(num_rows >= 0 && num_rows < (1LL << 31), "num_rows out of range: %lld",
                 (long long)num_rows);
    MAXK_REQUIRE(num_cols >= 0 && num_cols < (1LL << 31), "num_cols out of range: %lld",
                 (long long)num_cols);
    MAXK_REQUIRE(num_e >= 0 && num_e < (1LL << 31), "num_e out of range: %lld", (long long)num_e);
    MAXK_REQUIRE(chunk_edges >= 0, "chunk_edges must be >= 0");
    return MAXK_OK;
}
inline int check_slope(float slope) {
    MAXK_REQUIRE(slope >= 0.f && slope <= 1.f, "negative_slope must be in [0, 1], got %g",
                 (double)slope);  // a NaN fails both comparisons
    return MAXK_OK;
}
inline int check_workspace(const void *workspace, size_t bytes, size_t need) {
    MAXK_REQUIRE(workspace && bytes >= need, "workspace too small: need %zu bytes, got %zu", need,
                 workspace ? bytes : (size_t)0);
    MAXK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-B aligned");
    return MAXK_OK;
}
inline bool sizes_ok(int64_t num_rows, int64_t num_cols, int64_t num_e) {
    return num_rows >= 0 && num_cols >= 0 && num_e >= 0;
}

// ---- H heads: what edge_softmax_heads.hip, gat_attention_heads.hip and the fused attention
// backward (gat_attention_heads_bwd.hip) share --------------------------------------------------
// The scores interleaved to ss_t [C, HP], the slots of H heads with their merge, and the column
// sums over gzT [E, HP] through the CSC.  Each translation unit instantiates what it launches.

template <int HP>
struct alignas(4 * HP) VecF {
    float v[HP];
};

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : slope * v; }

// Slots of H heads: one row array, head h's partials at a / b + h * stride.
struct SlotsH {
    int32_t *__restrict__ row;
    float *__restrict__ a;
    float *__restrict__ b;
    int64_t stride;
    __device__ __forceinline__ Slots head(int h) const {
        return Slots{row, a + h * stride, b + h * stride};
    }
};

template <int HP>
struct TailH {
    int row;
    float a[HP], b[HP];
    __device__ __forceinline__ TailH() : row(-1) {
#pragma unroll
        for (int h = 0; h < HP; ++h) a[h] = b[h] = 0.f;
    }
};

template <int HP>
__device__ __forceinline__ void tail_from_group(TailH<HP> &t, int crow, const float (&ca)[HP],
                                                const float (&cb)[HP]) {
    const uint64_t m = __ballot(crow >= 0);
    if (!m) return;
    const int src = __builtin_ctzll(m);
    t.row = __shfl(crow, src);
#pragma unroll
    for (int h = 0; h < HP; ++h) {
        t.a[h] = __shfl(ca[h], src);
        t.b[h] = __shfl(cb[h], src);
    }
}

template <int HP>
__device__ __forceinline__ void store_slots(const SlotsH &sl, int H, int item,
                                            const TailH<HP> &head, const TailH<HP> &tail,
                                            int lane) {
    if (lane != 0) return;
    sl.row[2 * item] = head.row;
    sl.row[2 * item + 1] = tail.row;
#pragma unroll
    for (int h = 0; h < HP; ++h) {
        if (h < H) {
            const Slots s = sl.head(h);
            s.a[2 * item] = head.a[h];
            s.b[2 * item] = head.b[h];
            s.a[2 * item + 1] = tail.a[h];
            s.b[2 * item + 1] = tail.b[h];
        }
    }
}

// The interleave pre-pass: ss_t[c] = the HP scores of column c (pad heads 0).
template <int HP>
__global__ __launch_bounds__(kBlock) void esmh_interleave_kernel(
    const float *__restrict__ s_src, VecF<HP> *__restrict__ ss_t, int H, int64_t num_cols) {
    const int64_t c = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (c >= num_cols) return;
    VecF<HP> x;
#pragma unroll
    for (int h = 0; h < HP; ++h) x.v[h] = h < H ? s_src[h * num_cols + c] : 0.f;
    ss_t[c] = x;
}

// acc[h] = the sum over the CSC slots [0, n) of gzT[eid[i]].v[h].
template <int HP>
__device__ __forceinline__ void piece_gather(const VecF<HP> *__restrict__ gzT,
                                             const int32_t *__restrict__ eid, int H, int n,
                                             int lane, float (&acc)[HP]) {
#pragma unroll
    for (int h = 0; h < HP; ++h) acc[h] = 0.f;
    for (int base = 0; base < n; base += kWave * kU) {
        VecF<HP> g[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = base + u * kWave + lane;
#pragma unroll
            for (int h = 0; h < HP; ++h) g[u].v[h] = 0.f;
            if (i < n) g[u] = gzT[(uint32_t)eid[i]];
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
#pragma unroll
            for (int h = 0; h < HP; ++h) acc[h] += g[u].v[h];
    }
#pragma unroll
    for (int h = 0; h < HP; ++h)
        if (h < H) acc[h] = lane_tree<kWave, Sum>(acc[h]);
}

// A whole column writes grad_s_src, 0 for an unread one; a cut one leaves its partials in `tail`.
template <int HP>
__device__ __forceinline__ int short_cols_sum(const int32_t *__restrict__ col_ptr,
                                              const int32_t *__restrict__ eid,
                                              const VecF<HP> *__restrict__ gzT,
                                              float *__restrict__ grad_s_src, int H,
                                              int64_t num_cols, int first, int64_t d1, int lane,
                                              TailH<HP> &tail) {
    const int g = lane / kLR, j = lane % kLR;
    RowHandout<CutAtEnd> ho(col_ptr, (int)num_cols, first, d1, kShort, lane);
    int crow = -1;
    float ca[HP], zero[HP];
#pragma unroll
    for (int h = 0; h < HP; ++h) ca[h] = zero[h] = 0.f;
    for (;;) {
        int row = -1, b = 0, e = 0;
        ho.template assign<1>(true, kNG, kLR, g, lane, [&](int r, int rb, int re) {
            row = r;
            b = rb;
            e = re;
        });
        if (!__ballot(row >= 0)) break;
        const bool has = row >= 0;
        const int n = has ? e - b : 0;  // this lane's row piece: [b, b + n)
        const int full = has ? col_ptr[row + 1] : 0;
        const bool cut = has && e < full;
        float acc[HP];
#pragma unroll
        for (int h = 0; h < HP; ++h) acc[h] = 0.f;
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int o = j + kLR * u;
            VecF<HP> x;
#pragma unroll
            for (int h = 0; h < HP; ++h) x.v[h] = 0.f;
            if (o < n) x = gzT[(uint32_t)eid[b + o]];
#pragma unroll
            for (int h = 0; h < HP; ++h) acc[h] += x.v[h];
        }
#pragma unroll
        for (int h = 0; h < HP; ++h) {
            if (h < H) {
                acc[h] = lane_tree<kLR, Sum>(acc[h]);
                if (has && !cut && j == 0) grad_s_src[h * num_cols + row] = acc[h];
                if (cut && e > b) ca[h] = acc[h];
            }
        }
        if (cut && e > b) crow = row;
    }
    tail_from_group<HP>(tail, crow, ca, zero);
    return ho.next;
}

// The merge above, one head per blockIdx.y.  VAL_B: the partial sums are in b.
template <int MODE, bool VAL_B>
__global__ __launch_bounds__(kBlock) void esmh_merge_kernel(SlotsH slh, float *__restrict__ out,
                                                            int64_t out_stride, int n_slots) {
    const Slots sl = slh.head((int)blockIdx.y);
    merge_slots<MODE>(sl, VAL_B ? sl.b : sl.a, out ? out + blockIdx.y * out_stride : nullptr,
                      n_slots);
}

// grad_s_src[h, c] = the sum of gzT[.].v[h] over column c's CSC slots, in slot order; a cut
// column leaves its partials in the slots.
template <int HP>
__global__ __launch_bounds__(kBlock) void esmh_colsum_kernel(
    const int32_t *__restrict__ col_ptr, const int32_t *__restrict__ eid,
    const VecF<HP> *__restrict__ gzT, float *__restrict__ grad_s_src, SlotsH sl, int H,
    int64_t num_cols, int64_t num_e, int chunk, int n_items) {
    const int item = item_of_wave(n_items);
    if (item < 0) return;
    const int lane = lane_id();
    const int nc = (int)num_cols;
    const ItemRange it = item_range(col_ptr, nc, num_e, item, chunk);
    TailH<HP> head, tail;
    if (it.r > 0) {
        const RowPiece p = cont_piece(CutAtEnd{}, it.p_lo, it.d1, it.r, col_ptr[it.r]);
        if (p.sb < p.se) {
            head.row = it.r - 1;
            piece_gather<HP>(gzT, eid + p.sb, H, (int)(p.se - p.sb), lane, head.a);
        }
    }
    int c = it.r;
    while (c < nc) {
        c = short_cols_sum<HP>(col_ptr, eid, gzT, grad_s_src, H, num_cols, c, it.d1, lane, tail);
        if (c >= nc) break;
        const int64_t cb = col_ptr[c];
        if (!row_owned(it.d1, c, cb)) break;
        const int64_t ce = col_ptr[c + 1];
        const RowPiece p = row_piece(CutAtEnd{}, it.d1, c, cb, ce);
        const int n = (int)(p.se - p.sb);
        if (n > 0) {
            float acc[HP];
            piece_gather<HP>(gzT, eid + p.sb, H, n, lane, acc);
            if (p.se == ce) {
#pragma unroll
                for (int h = 0; h < HP; ++h)
                    if (h < H && lane == 0) grad_s_src[h * num_cols + c] = acc[h];
            } else {
                tail.row = c;
#pragma unroll
                for (int h = 0; h < HP; ++h) tail.a[h] = acc[h];
            }
        } else if (ce == cb && lane == 0) {
#pragma unroll
            for (int h = 0; h < HP; ++h)
                if (h < H) grad_s_src[h * num_cols + c] = 0.f;
        }
        ++c;
    }
    store_slots<HP>(sl, H, item, head, tail, lane);
}

// Heads padded to a vector of 2, 4 or 8 scores.
inline int hp_of(int H) { return H <= 2 ? 2 : H <= 4 ? 4 : 8; }

// Slots of H heads over n rows (or columns): [row | a x H | b x H], each part the single-head
// size, so head h's a and b are arrays the single-head merge takes.
struct SlotLayoutH {
    int chunk, n_items;
    size_t row_off, a_off, b_off, end;
    int64_t stride;  // floats between two heads' partials
};
inline SlotLayoutH slot_layout_h(int64_t n, int64_t num_e, int chunk, int H, size_t base) {
    const SlotLayout one = slot_layout(n, num_e, chunk, 0);
    const size_t bytes = one.a_off;  // one part
    SlotLayoutH L{};
    L.chunk = one.chunk;
    L.n_items = one.n_items;
    L.row_off = base;
    L.a_off = L.row_off + bytes;
    L.b_off = L.a_off + (size_t)H * bytes;
    L.end = L.b_off + (size_t)H * bytes;
    L.stride = (int64_t)(bytes / sizeof(float));
    return L;
}
inline SlotsH slots_at(void *ws, const SlotLayoutH &L) {
    uint8_t *p = reinterpret_cast<uint8_t *>(ws);
    return SlotsH{reinterpret_cast<int32_t *>(p + L.row_off),
                  reinterpret_cast<float *>(p + L.a_off), reinterpret_cast<float *>(p + L.b_off),
                  L.stride};
}

inline dim3 with_heads(dim3 g, int H) { return dim3(g.x, (unsigned)H); }

inline int check_heads(int32_t num_heads) {
    MAXK_REQUIRE(num_heads >= 1 && num_heads <= MAXK_MAX_HEADS,
                 "num_heads must be in [1,%d], got %d", MAXK_MAX_HEADS, num_heads);
    return MAXK_OK;
}

// The column sums of the heads' backward over gzT [E, HP]: esmh_colsum_kernel and the merge of
// the cut columns, into grad_s_src [H, num_cols] (every element written).
template <int HP>
int launch_heads_colsum(const int32_t *col_ptr, const int32_t *csc_eid, const VecF<HP> *gzT,
                        float *grad_s_src, void *workspace, const SlotLayoutH &C, int H,
                        int64_t num_cols, int64_t num_e, hipStream_t s) {
    const SlotsH csl = slots_at(workspace, C);
    hipLaunchKernelGGL(esmh_colsum_kernel<HP>, item_grid(C.n_items), dim3(kBlock), 0, s, col_ptr,
                       csc_eid, gzT, grad_s_src, csl, H, num_cols, num_e, C.chunk, C.n_items);
    MAXK_LAUNCHED("esmh_colsum_kernel");
    hipLaunchKernelGGL((esmh_merge_kernel<kMergeOut, false>), with_heads(slot_grid(C.n_items), H),
                       dim3(kBlock), 0, s, csl, grad_s_src, num_cols, 2 * C.n_items);
    MAXK_LAUNCHED("esmh_merge_kernel");
    return MAXK_OK;
}

}  // namespace
}  // namespace maxk
