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
#include "edge_softmax.h"

namespace maxk {
namespace {

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
