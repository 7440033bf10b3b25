// The GAT edge softmax of H heads over one walk of the graph, for gfx950: what H calls of
// maxk_gat_edge_softmax / _backward (edge_softmax.hip) compute, head-major, with the per-edge
// reads the heads share done once.
//
//   * col_idx[e] is read once per edge instead of once per edge and head;
//   * the scores s_src [H, C] are first copied to ss_t [C, HP], HP = H rounded up to 2, 4 or 8
//     (pad heads 0): a column's HP scores are one aligned 4 * HP-byte vector inside one 64-B
//     sector, so the random gather per edge costs one sector for all heads, forward and backward;
//   * the backward writes gz edge-major, gzT [E, HP] (lane e stores one vector, coalesced across
//     the wave), and the column sums gather one vector per CSC slot through csc_eid, read once.
//   w, grad_w, s_dst and the gradients stay head-major: they stream, or are read once per row.
//   One head has nothing to share: num_heads == 1 is handed to the single-head entries (HP = 1
//   is not instantiated).
//
// Partition, item rule, lane assignment, butterflies and slot order are those of the single-head
// kernels (edge_softmax.h holds the shared parts): every head's sums add the same numbers in the
// same order.  The forward is bitwise the single-head entry on slice h for the same chunk_edges
// (tests/test_heads_softmax_gpu.py holds it to that): the same walks of the same pieces, and
// the forward has no multiply feeding an add.  The backward has two, w * gw into t and
// gz = x * fac into the piece's sum, and the compiler contracts each inlined copy of them its own
// way (the single-head register walk fuses six of a lane's eight products of t and multiplies
// the last two as a pair; its staged walk fuses none), so the backward agrees with the
// single-head entry within the bound of both, not bitwise: DESIGN.md 5.9.  It takes the staged
// walk (piece_dot per head, then one emit) for every whole-wave piece.
//
// H is a run-time value under wave-uniform `h < H` tests inside loops unrolled over HP: nothing
// is indexed by a run-time value, nothing lives in scratch.  Every index scaled by H or HP or
// offset by h * num_e is 64-bit (pointer arithmetic on 4 * HP-byte vectors, int64_t strides).
#include "edge_softmax.h"

namespace maxk {
namespace {

// VecF, the slots of H heads, the interleave pre-pass, the merge and the column sums are in
// edge_softmax.h: the fused attention backward (gat_attention_heads_bwd.hip) runs them too.

// What every walk of the heads needs beside the graph.
template <int HP>
struct Heads {
    const VecF<HP> *__restrict__ ss_t;  // [C] vectors of HP scores
    const float *__restrict__ s_dst;    // [H, num_rows]
    int64_t num_rows, num_e;
    float slope;
    int H;
    __device__ __forceinline__ void row_scores(int row, float (&sd)[HP]) const {
#pragma unroll
        for (int h = 0; h < HP; ++h) sd[h] = h < H && row >= 0 ? s_dst[h * num_rows + row] : 0.f;
    }
};

// ---- whole-wave pieces (n edges, n >= 1, wave-uniform; pointers offset to the piece) ----------

// (max, sum of exp) of the piece per head; `whole`: the piece is its row, w is finished; else w
// holds the logits for the second walk.
template <int HP>
__device__ __forceinline__ void piece_fwd(const Heads<HP> &A, const float (&sd)[HP],
                                          const int32_t *__restrict__ col, float *__restrict__ wp,
                                          int n, bool whole, int lane, float (&m)[HP],
                                          float (&s)[HP]) {
    constexpr int REG = kReg;  // as the single-head walk: 160 VGPRs at HP = 8, no scratch
    if (n > kRegPiece) {  // staged: the logits of every head from one gather, then per head
#pragma unroll
        for (int h = 0; h < HP; ++h) m[h] = -INFINITY;
        for (int base = 0; base < n; base += kWave * kU) {
            VecF<HP> x[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int i = base + u * kWave + lane;
                if (i < n) x[u] = A.ss_t[(uint32_t)col[i]];
            }
#pragma unroll
            for (int h = 0; h < HP; ++h) {
                if (h < A.H) {
#pragma unroll
                    for (int u = 0; u < kU; ++u) {
                        const int i = base + u * kWave + lane;
                        const float l = i < n ? leaky(sd[h] + x[u].v[h], A.slope) : -INFINITY;
                        if (i < n) wp[h * A.num_e + i] = l;
                        m[h] = fmaxf(m[h], l);
                    }
                }
            }
        }
#pragma unroll
        for (int h = 0; h < HP; ++h) {
            if (h < A.H) {
                float *wh = wp + h * A.num_e;
                m[h] = lane_tree<kWave, Max>(m[h]);
                s[h] = piece_expsum(wh, shift_of(m[h]), n, lane);
                if (whole) piece_normalise(wh, shift_of(m[h]), s[h], n, lane);
            }
        }
        return;
    }
    VecF<HP> x[REG];
#pragma unroll
    for (int u = 0; u < REG; ++u) {
        const int i = u * kWave + lane;
        if (i < n) x[u] = A.ss_t[(uint32_t)col[i]];
    }
#pragma unroll
    for (int h = 0; h < HP; ++h) {
        if (h < A.H) {
            float l[REG], p[REG];
            float mh = -INFINITY;
#pragma unroll
            for (int u = 0; u < REG; ++u) {
                const int i = u * kWave + lane;
                l[u] = i < n ? leaky(sd[h] + x[u].v[h], A.slope) : -INFINITY;
            }
#pragma unroll
            for (int u = 0; u < REG; ++u) mh = fmaxf(mh, l[u]);
            mh = lane_tree<kWave, Max>(mh);
            const float shift = shift_of(mh);
            float sh = 0.f;
#pragma unroll
            for (int u = 0; u < REG; ++u) {
                p[u] = expf(l[u] - shift);  // past the end: exp(-inf) = 0
                sh += p[u];
            }
            sh = lane_tree<kWave, Sum>(sh);
#pragma unroll
            for (int u = 0; u < REG; ++u) {
                const int i = u * kWave + lane;
                if (i < n) wp[h * A.num_e + i] = whole ? p[u] / sh : l[u];
            }
            m[h] = mh;
            s[h] = sh;
        }
    }
}

// gzT[i] = the gz of every head of edge i; acc[h] = the piece's sum of head h's.
template <int HP>
__device__ __forceinline__ void piece_emit(const Heads<HP> &A, const float (&sd)[HP],
                                           const int32_t *__restrict__ col,
                                           const float *__restrict__ wp,
                                           const float *__restrict__ gp, const float (&t)[HP],
                                           VecF<HP> *__restrict__ op, int n, int lane,
                                           float (&acc)[HP]) {
#pragma unroll
    for (int h = 0; h < HP; ++h) acc[h] = 0.f;
    for (int base = 0; base < n; base += kWave * kU) {
        VecF<HP> g[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = base + u * kWave + lane;
#pragma unroll
            for (int h = 0; h < HP; ++h) g[u].v[h] = 0.f;
            if (i < n) {
                const VecF<HP> x = A.ss_t[(uint32_t)col[i]];
#pragma unroll
                for (int h = 0; h < HP; ++h) {
                    if (h < A.H) {
                        float v = wp[h * A.num_e + i] * (gp[h * A.num_e + i] - t[h]);
                        v *= sd[h] + x.v[h] > 0.f ? 1.f : A.slope;
                        g[u].v[h] = v;
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = base + u * kWave + lane;
            if (i < n) op[i] = g[u];
#pragma unroll
            for (int h = 0; h < HP; ++h) acc[h] += g[u].v[h];
        }
    }
#pragma unroll
    for (int h = 0; h < HP; ++h)
        if (h < A.H) acc[h] = lane_tree<kWave, Sum>(acc[h]);
}

// ---- short rows: one row per lane group, its edges in registers ------------------------------

template <int HP>
__device__ __forceinline__ int short_rows_fwd(const Heads<HP> &A,
                                              const int32_t *__restrict__ row_ptr,
                                              const int32_t *__restrict__ col_idx,
                                              float *__restrict__ w, int num_rows, int first,
                                              int64_t d1, int lane, TailH<HP> &tail) {
    const int g = lane / kLR, j = lane % kLR;
    RowHandout<CutAtEnd> ho(row_ptr, num_rows, first, d1, kShort, lane);
    int crow = -1;
    float cm[HP], cs[HP];
#pragma unroll
    for (int h = 0; h < HP; ++h) cm[h] = cs[h] = 0.f;
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
        const int full = has ? row_ptr[row + 1] : 0;
        const bool cut = has && e < full;
        float sd[HP];
        A.row_scores(row, sd);
        VecF<HP> x[kPer];
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int o = j + kLR * u;  // offsets, not indices: b + o may pass 2^31 past e
            if (o < n) x[u] = A.ss_t[(uint32_t)col_idx[b + o]];
        }
#pragma unroll
        for (int h = 0; h < HP; ++h) {
            if (h < A.H) {
                float l[kPer], p[kPer], m = -INFINITY;
#pragma unroll
                for (int u = 0; u < kPer; ++u) {
                    const int o = j + kLR * u;
                    l[u] = o < n ? leaky(sd[h] + x[u].v[h], A.slope) : -INFINITY;
                    m = fmaxf(m, l[u]);
                }
                m = lane_tree<kLR, Max>(m);
                const float shift = shift_of(m);
                float s = 0.f;
#pragma unroll
                for (int u = 0; u < kPer; ++u) {
                    p[u] = expf(l[u] - shift);  // a lane without an edge: exp(-inf) = 0
                    s += p[u];
                }
                s = lane_tree<kLR, Sum>(s);
#pragma unroll
                for (int u = 0; u < kPer; ++u) {
                    const int o = j + kLR * u;
                    if (o < n) w[h * A.num_e + b + o] = cut ? l[u] : p[u] / s;
                }
                if (cut && e > b) {
                    cm[h] = m;
                    cs[h] = s;
                }
            }
        }
        if (cut && e > b) crow = row;
    }
    tail_from_group<HP>(tail, crow, cm, cs);
    return ho.next;
}

// A whole row writes gzT and grad_s_dst, 0 for a row without edges; a cut one leaves t in `tail`.
template <int HP>
__device__ __forceinline__ int short_rows_bwd(const Heads<HP> &A,
                                              const int32_t *__restrict__ row_ptr,
                                              const int32_t *__restrict__ col_idx,
                                              const float *__restrict__ w,
                                              const float *__restrict__ gw,
                                              VecF<HP> *__restrict__ gzT,
                                              float *__restrict__ grad_s_dst, int num_rows,
                                              int first, int64_t d1, int lane, TailH<HP> &tail) {
    const int g = lane / kLR, j = lane % kLR;
    RowHandout<CutAtEnd> ho(row_ptr, num_rows, first, d1, kShort, lane);
    int crow = -1;
    float ct[HP], zero[HP];
#pragma unroll
    for (int h = 0; h < HP; ++h) ct[h] = zero[h] = 0.f;
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
        const int full = has ? row_ptr[row + 1] : 0;
        const bool cut = has && e < full;
        float sd[HP];
        A.row_scores(row, sd);
        VecF<HP> x[kPer], gz[kPer];
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int o = j + kLR * u;
#pragma unroll
            for (int h = 0; h < HP; ++h) x[u].v[h] = gz[u].v[h] = 0.f;
            if (!cut && o < n) x[u] = A.ss_t[(uint32_t)col_idx[b + o]];
        }
#pragma unroll
        for (int h = 0; h < HP; ++h) {
            if (h < A.H) {
                const float *wh = w + h * A.num_e, *gh = gw + h * A.num_e;
                float wv[kPer], gv[kPer], t = 0.f;
#pragma unroll
                for (int u = 0; u < kPer; ++u) {
                    const int o = j + kLR * u;
                    wv[u] = o < n ? wh[b + o] : 0.f;
                    gv[u] = o < n ? gh[b + o] : 0.f;
                    t += wv[u] * gv[u];
                }
                t = lane_tree<kLR, Sum>(t);
                float acc = 0.f;
                if (!cut) {
#pragma unroll
                    for (int u = 0; u < kPer; ++u) {
                        const int o = j + kLR * u;
                        if (o < n) {
                            float v = wv[u] * (gv[u] - t);
                            v *= sd[h] + x[u].v[h] > 0.f ? 1.f : A.slope;
                            gz[u].v[h] = v;
                            acc += v;
                        }
                    }
                }
                acc = lane_tree<kLR, Sum>(acc);
                if (has && !cut && j == 0) grad_s_dst[h * A.num_rows + row] = acc;
                if (cut && e > b) ct[h] = t;
            }
        }
        if (!cut) {
#pragma unroll
            for (int u = 0; u < kPer; ++u) {
                const int o = j + kLR * u;
                if (o < n) gzT[b + o] = gz[u];
            }
        }
        if (cut && e > b) crow = row;
    }
    tail_from_group<HP>(tail, crow, ct, zero);
    return ho.next;
}

// ---- forward ---------------------------------------------------------------------------------

template <int HP>
__global__ __launch_bounds__(kBlock) void esmh_fwd_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx, Heads<HP> A,
    float *__restrict__ w, SlotsH sl, int chunk, int n_items) {
    const int item = item_of_wave(n_items);
    if (item < 0) return;  // whole wave; no workgroup barrier below
    const int lane = lane_id();
    const int num_rows = (int)A.num_rows;
    const ItemRange it = item_range(row_ptr, num_rows, A.num_e, item, chunk);
    TailH<HP> head, tail;

    if (it.r > 0) {  // the tail of row r - 1, whose token precedes the item
        const RowPiece p = cont_piece(CutAtEnd{}, it.p_lo, it.d1, it.r, row_ptr[it.r]);
        if (p.sb < p.se) {
            head.row = it.r - 1;
            float sd[HP];
            A.row_scores(head.row, sd);
            piece_fwd<HP>(A, sd, col_idx + p.sb, w + p.sb, (int)(p.se - p.sb), false, lane,
                          head.a, head.b);
        }
    }
    int q = it.r;
    while (q < num_rows) {
        q = short_rows_fwd<HP>(A, row_ptr, col_idx, w, num_rows, q, it.d1, lane, tail);
        if (q >= num_rows) break;
        const int64_t rb = row_ptr[q];
        if (!row_owned(it.d1, q, rb)) break;  // row q's token belongs to a later item
        const int64_t re = row_ptr[q + 1];
        const RowPiece p = row_piece(CutAtEnd{}, it.d1, q, rb, re);
        if (p.sb < p.se) {
            float sd[HP], m[HP], s[HP];
            A.row_scores(q, sd);
            piece_fwd<HP>(A, sd, col_idx + p.sb, w + p.sb, (int)(p.se - p.sb), p.se == re, lane,
                          m, s);
            if (p.se < re) {
                tail.row = q;
#pragma unroll
                for (int h = 0; h < HP; ++h) {
                    if (h < A.H) {
                        tail.a[h] = m[h];
                        tail.b[h] = s[h];
                    }
                }
            }
        }
        ++q;
    }
    store_slots<HP>(sl, A.H, item, head, tail, lane);
}

// The second walk, one head per blockIdx.y: the cut pieces only.
__global__ __launch_bounds__(kBlock) void esmh_normalise_kernel(
    const int32_t *__restrict__ row_ptr, float *__restrict__ w_all, SlotsH slh, int num_rows,
    int64_t num_e, int chunk, int n_items) {
    const int item = item_of_wave(n_items);
    if (item < 0) return;
    const int lane = lane_id();
    const Slots sl = slh.head((int)blockIdx.y);
    float *w = w_all + blockIdx.y * num_e;
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

// ---- backward --------------------------------------------------------------------------------

// First walk: t of every piece and head; a row inside one item is finished (gzT and grad_s_dst
// written, 0 for a row without edges), a cut piece leaves t in its slot.
template <int HP>
__global__ __launch_bounds__(kBlock) void esmh_bwd_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx, Heads<HP> A,
    const float *__restrict__ w, const float *__restrict__ gw, VecF<HP> *__restrict__ gzT,
    float *__restrict__ grad_s_dst, SlotsH sl, int chunk, int n_items) {
    const int item = item_of_wave(n_items);
    if (item < 0) return;
    const int lane = lane_id();
    const int num_rows = (int)A.num_rows;
    const ItemRange it = item_range(row_ptr, num_rows, A.num_e, item, chunk);
    TailH<HP> head, tail;
    auto dots = [&](int64_t sb, int n, float(&t)[HP]) {
#pragma unroll
        for (int h = 0; h < HP; ++h)
            if (h < A.H)
                t[h] = piece_dot(w + h * A.num_e + sb, gw + h * A.num_e + sb, n, lane);
    };
    if (it.r > 0) {
        const RowPiece p = cont_piece(CutAtEnd{}, it.p_lo, it.d1, it.r, row_ptr[it.r]);
        if (p.sb < p.se) {
            head.row = it.r - 1;
            dots(p.sb, (int)(p.se - p.sb), head.a);
        }
    }
    int q = it.r;
    while (q < num_rows) {
        q = short_rows_bwd<HP>(A, row_ptr, col_idx, w, gw, gzT, grad_s_dst, num_rows, q, it.d1,
                               lane, tail);
        if (q >= num_rows) break;
        const int64_t rb = row_ptr[q];
        if (!row_owned(it.d1, q, rb)) break;
        const int64_t re = row_ptr[q + 1];
        const RowPiece p = row_piece(CutAtEnd{}, it.d1, q, rb, re);
        const int n = (int)(p.se - p.sb);
        if (n > 0) {
            float t[HP];
#pragma unroll
            for (int h = 0; h < HP; ++h) t[h] = 0.f;
            dots(p.sb, n, t);
            if (p.se == re) {
                float sd[HP], acc[HP];
                A.row_scores(q, sd);
                piece_emit<HP>(A, sd, col_idx + p.sb, w + p.sb, gw + p.sb, t, gzT + p.sb, n, lane,
                               acc);
#pragma unroll
                for (int h = 0; h < HP; ++h)
                    if (h < A.H && lane == 0) grad_s_dst[h * A.num_rows + q] = acc[h];
            } else {
                tail.row = q;
#pragma unroll
                for (int h = 0; h < HP; ++h) tail.a[h] = t[h];
            }
        } else if (re == rb && lane == 0) {
#pragma unroll
            for (int h = 0; h < HP; ++h)
                if (h < A.H) grad_s_dst[h * A.num_rows + q] = 0.f;
        }
        ++q;
    }
    store_slots<HP>(sl, A.H, item, head, tail, lane);
}

// Second walk: the cut pieces' gz from the row's t (slot a); the piece's sums go to slot b.
template <int HP>
__global__ __launch_bounds__(kBlock) void esmh_bwd_emit_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx, Heads<HP> A,
    const float *__restrict__ w, const float *__restrict__ gw, VecF<HP> *__restrict__ gzT,
    SlotsH sl, int chunk, int n_items) {
    const int item = item_of_wave(n_items);
    if (item < 0) return;
    const int lane = lane_id();
    const int64_t total = A.num_rows + A.num_e;
    const int64_t d0 = (int64_t)item * chunk;
    const int64_t d1 = d0 + chunk < total ? d0 + chunk : total;
    auto emit = [&](int slot, int row, const RowPiece &p) {
        float sd[HP], t[HP], acc[HP];
        A.row_scores(row, sd);
#pragma unroll
        for (int h = 0; h < HP; ++h) t[h] = h < A.H ? sl.head(h).a[slot] : 0.f;
        piece_emit<HP>(A, sd, col_idx + p.sb, w + p.sb, gw + p.sb, t, gzT + p.sb,
                       (int)(p.se - p.sb), lane, acc);
#pragma unroll
        for (int h = 0; h < HP; ++h)
            if (h < A.H && lane == 0) sl.head(h).b[slot] = acc[h];
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

// ---- host ------------------------------------------------------------------------------------
// (one head takes the single-head entry: hp_of is asked from two heads on)

// Workspace: ss_t [C, HP], the row slots x H, and for the backward gzT [E, HP] and the column
// slots x H.
struct HeadsLayout {
    size_t ss_off, gz_off, total;
    SlotLayoutH rows, cols;
};
HeadsLayout heads_layout(int H, int64_t num_rows, int64_t num_cols, int64_t num_e, int chunk,
                         bool backward) {
    const size_t vec = (size_t)hp_of(H) * sizeof(float);
    HeadsLayout G{};
    G.ss_off = 0;
    G.rows = slot_layout_h(num_rows, num_e, chunk, H, al256((size_t)num_cols * vec));
    G.total = G.rows.end;
    if (backward) {
        G.gz_off = G.rows.end;
        G.cols = slot_layout_h(num_cols, num_e, chunk, H, G.gz_off + al256((size_t)num_e * vec));
        G.total = G.cols.end;
    }
    return G;
}

template <int HP>
int launch_interleave(const float *s_src, void *workspace, const HeadsLayout &G, int H,
                      int64_t num_cols, hipStream_t s) {
    VecF<HP> *ss_t =
        reinterpret_cast<VecF<HP> *>(reinterpret_cast<uint8_t *>(workspace) + G.ss_off);
    hipLaunchKernelGGL(esmh_interleave_kernel<HP>, dim3((unsigned)ceil_div(num_cols, kBlock)),
                       dim3(kBlock), 0, s, s_src, ss_t, H, num_cols);
    MAXK_LAUNCHED("esmh_interleave_kernel");
    return MAXK_OK;
}

template <int HP>
int launch_fwd_heads(const int32_t *row_ptr, const int32_t *col_idx, const float *s_dst,
                     const float *s_src, float slope, float *w, int H, int64_t num_rows,
                     int64_t num_cols, int64_t num_e, int32_t chunk_edges, void *workspace,
                     hipStream_t s) {
    const HeadsLayout G = heads_layout(H, num_rows, num_cols, num_e, chunk_edges, false);
    if (int rc = launch_interleave<HP>(s_src, workspace, G, H, num_cols, s)) return rc;
    const Heads<HP> A{
        reinterpret_cast<const VecF<HP> *>(reinterpret_cast<uint8_t *>(workspace) + G.ss_off),
        s_dst, num_rows, num_e, slope, H};
    const SlotLayoutH &L = G.rows;
    const SlotsH sl = slots_at(workspace, L);
    hipLaunchKernelGGL(esmh_fwd_kernel<HP>, item_grid(L.n_items), dim3(kBlock), 0, s, row_ptr,
                       col_idx, A, w, sl, L.chunk, L.n_items);
    MAXK_LAUNCHED("esmh_fwd_kernel");
    hipLaunchKernelGGL((esmh_merge_kernel<kMergeSoftmax, false>),
                       with_heads(slot_grid(L.n_items), H), dim3(kBlock), 0, s, sl,
                       (float *)nullptr, (int64_t)0, 2 * L.n_items);
    MAXK_LAUNCHED("esmh_merge_kernel");
    hipLaunchKernelGGL(esmh_normalise_kernel, with_heads(item_grid(L.n_items), H), dim3(kBlock),
                       0, s, row_ptr, w, sl, (int)num_rows, num_e, L.chunk, L.n_items);
    MAXK_LAUNCHED("esmh_normalise_kernel");
    return MAXK_OK;
}

template <int HP>
int launch_bwd_heads(const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr,
                     const int32_t *csc_eid, const float *s_dst, const float *s_src, float slope,
                     const float *w, const float *gw, float *grad_s_dst, float *grad_s_src, int H,
                     int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t chunk_edges,
                     void *workspace, hipStream_t s) {
    const HeadsLayout G = heads_layout(H, num_rows, num_cols, num_e, chunk_edges, true);
    if (int rc = launch_interleave<HP>(s_src, workspace, G, H, num_cols, s)) return rc;
    uint8_t *base = reinterpret_cast<uint8_t *>(workspace);
    const Heads<HP> A{reinterpret_cast<const VecF<HP> *>(base + G.ss_off), s_dst, num_rows, num_e,
                      slope, H};
    VecF<HP> *gzT = reinterpret_cast<VecF<HP> *>(base + G.gz_off);
    const SlotLayoutH &L = G.rows;
    const SlotsH sl = slots_at(workspace, L);
    hipLaunchKernelGGL(esmh_bwd_kernel<HP>, item_grid(L.n_items), dim3(kBlock), 0, s, row_ptr,
                       col_idx, A, w, gw, gzT, grad_s_dst, sl, L.chunk, L.n_items);
    MAXK_LAUNCHED("esmh_bwd_kernel");
    hipLaunchKernelGGL((esmh_merge_kernel<kMergeShare, false>),
                       with_heads(slot_grid(L.n_items), H), dim3(kBlock), 0, s, sl,
                       (float *)nullptr, (int64_t)0, 2 * L.n_items);
    MAXK_LAUNCHED("esmh_merge_kernel");
    hipLaunchKernelGGL(esmh_bwd_emit_kernel<HP>, item_grid(L.n_items), dim3(kBlock), 0, s,
                       row_ptr, col_idx, A, w, gw, gzT, sl, L.chunk, L.n_items);
    MAXK_LAUNCHED("esmh_bwd_emit_kernel");
    hipLaunchKernelGGL((esmh_merge_kernel<kMergeOut, true>), with_heads(slot_grid(L.n_items), H),
                       dim3(kBlock), 0, s, sl, grad_s_dst, num_rows, 2 * L.n_items);
    MAXK_LAUNCHED("esmh_merge_kernel");
    return launch_heads_colsum<HP>(col_ptr, csc_eid, gzT, grad_s_src, workspace, G.cols, H,
                                   num_cols, num_e, s);
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" size_t maxk_gat_edge_softmax_heads_workspace_size(int32_t num_heads, int64_t num_rows,
                                                             int64_t num_cols, int64_t num_e,
                                                             int32_t chunk_edges) {
    if (!sizes_ok(num_rows, num_cols, num_e) || chunk_edges < 0 || num_heads < 1 ||
        num_heads > MAXK_MAX_HEADS)
        return 0;
    if (num_heads == 1)
        return maxk_gat_edge_softmax_workspace_size(num_rows, num_cols, num_e, chunk_edges);
    return heads_layout(num_heads, num_rows, num_cols, num_e, chunk_edges, false).total;
}

extern "C" size_t maxk_gat_edge_softmax_heads_backward_workspace_size(
    int32_t num_heads, int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t chunk_edges) {
    if (!sizes_ok(num_rows, num_cols, num_e) || chunk_edges < 0 || num_heads < 1 ||
        num_heads > MAXK_MAX_HEADS)
        return 0;
    if (num_heads == 1)
        return maxk_gat_edge_softmax_backward_workspace_size(num_rows, num_cols, num_e,
                                                             chunk_edges);
    return heads_layout(num_heads, num_rows, num_cols, num_e, chunk_edges, true).total;
}

extern "C" int maxk_gat_edge_softmax_heads(const int32_t *row_ptr, const int32_t *col_idx,
                                           const float *s_dst, const float *s_src,
                                           float negative_slope, float *w, int32_t num_heads,
                                           int64_t num_rows, int64_t num_cols, int64_t num_e,
                                           int32_t chunk_edges, void *workspace,
                                           size_t workspace_bytes, void *stream) {
    clear_error();
    if (int rc = check_heads(num_heads)) return rc;
    if (num_heads == 1)  // nothing to share: the single-head entry, its workspace and its bytes
        return maxk_gat_edge_softmax(row_ptr, col_idx, s_dst, s_src, negative_slope, w, num_rows,
                                     num_cols, num_e, chunk_edges, workspace, workspace_bytes,
                                     stream);
    if (int rc = check_sizes(num_rows, num_cols, num_e, chunk_edges)) return rc;
    if (int rc = check_slope(negative_slope)) return rc;
    if (num_e == 0) return MAXK_OK;  // no edge, nothing to write
    MAXK_REQUIRE(num_rows > 0 && num_cols > 0, "edges present but num_rows or num_cols == 0");
    MAXK_REQUIRE(row_ptr && col_idx && s_dst && s_src && w,
                 "row_ptr / col_idx / s_dst / s_src / w must not be NULL");
    const size_t need =
        heads_layout(num_heads, num_rows, num_cols, num_e, chunk_edges, false).total;
    if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    hipStream_t s = as_stream(stream);
#define MAXK_ESMH_FWD(HP)                                                                      \
    launch_fwd_heads<HP>(row_ptr, col_idx, s_dst, s_src, negative_slope, w, num_heads, num_rows, \
                         num_cols, num_e, chunk_edges, workspace, s)
    switch (hp_of(num_heads)) {
        case 2: return MAXK_ESMH_FWD(2);
        case 4: return MAXK_ESMH_FWD(4);
        default: return MAXK_ESMH_FWD(8);
    }
#undef MAXK_ESMH_FWD
}

extern "C" int maxk_gat_edge_softmax_heads_backward(
    const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr,
    const int32_t *csc_eid, const float *s_dst, const float *s_src, float negative_slope,
    const float *w, const float *grad_w, float *grad_s_dst, float *grad_s_src, int32_t num_heads,
    int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t chunk_edges, void *workspace,
    size_t workspace_bytes, void *stream) {
    clear_error();
    if (int rc = check_heads(num_heads)) return rc;
    if (num_heads == 1)
        return maxk_gat_edge_softmax_backward(row_ptr, col_idx, col_ptr, csc_eid, s_dst, s_src,
                                              negative_slope, w, grad_w, grad_s_dst, grad_s_src,
                                              num_rows, num_cols, num_e, chunk_edges, workspace,
                                              workspace_bytes, stream);
    if (int rc = check_sizes(num_rows, num_cols, num_e, chunk_edges)) return rc;
    if (int rc = check_slope(negative_slope)) return rc;
    MAXK_REQUIRE((grad_s_dst || num_rows == 0) && (grad_s_src || num_cols == 0),
                 "grad_s_dst / grad_s_src must not be NULL");
    hipStream_t s = as_stream(stream);
    if (num_e == 0) {  // no edge: both gradients are zeros
        if (int rc = zero_words(grad_s_dst, num_heads * num_rows, s)) return rc;
        return zero_words(grad_s_src, num_heads * num_cols, s);
    }
    MAXK_REQUIRE(num_rows > 0 && num_cols > 0, "edges present but num_rows or num_cols == 0");
    MAXK_REQUIRE(row_ptr && col_idx && col_ptr && csc_eid && s_dst && s_src && w && grad_w,
                 "CSR / CSC / score / w / grad_w pointers must not be NULL");
    const size_t need = heads_layout(num_heads, num_rows, num_cols, num_e, chunk_edges, true).total;
    if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
#define MAXK_ESMH_BWD(HP)                                                                        \
    launch_bwd_heads<HP>(row_ptr, col_idx, col_ptr, csc_eid, s_dst, s_src, negative_slope, w,    \
                         grad_w, grad_s_dst, grad_s_src, num_heads, num_rows, num_cols, num_e,   \
                         chunk_edges, workspace, s)
    switch (hp_of(num_heads)) {
        case 2: return MAXK_ESMH_BWD(2);
        case 4: return MAXK_ESMH_BWD(4);
        default: return MAXK_ESMH_BWD(8);
    }
#undef MAXK_ESMH_BWD
}
