// Fused backward of the multi-head GAT attention (gat_attention_heads.hip) for gfx950: the edge
// gradient, the softmax backward and the feature contribution of every edge in one walk of the
// graph, without alpha [H, E], grad_alpha [H, E] or any other tensor of H * E elements.
//
//   alpha_he = exp(l_he - row_max[h, r]) / row_sum[h, r]          e in row r, c = col_idx[e]
//   ga_he    = sum_l cbsr_val[c, l] * grad_out[h, r, cbsr_idx[c, l]]
//   t_hr     = sum_{j : out[h, r, j] != 0} out[h, r, j] * grad_out[h, r, j]
//   gz_he    = alpha_he * (ga_he - t_hr) * (z_he > 0 ? 1 : negative_slope)
//   grad_s_dst[h, r] = sum_{e in r} gz_he      grad_s_src[h, c] = sum_{e: col = c} gz_he
//   grad_cbsr[c, l]  = sum_h sum_{e -> c} alpha_he * grad_out[h, r, cbsr_idx[c, l]]
//
// t is the softmax backward's sum_e alpha_he * ga_he, which equals the dot product of the two
// dense rows out[h, r, :] and grad_out[h, r, :]: every item computes it for itself before it
// touches an edge, so a row cut over items needs no second walk.
//
//  1. launch_cbsr_pack and esmh_interleave_kernel fill the workspace's records and ss_t.
//  2. gath_bwd_kernel, a staged-row walk (piece_walk.h): one wavefront per item of `chunk` tokens
//     cut at the item's end (CutAtEnd), KG = pow2ceil(k) lanes per edge (8 .. 64), G = 64 / KG
//     edges per wave step, U steps in flight.
//     * per row piece: the H rows grad_out[h, r, :] staged side by side in the wave's LDS
//       (H * DS floats, the pad columns [D, DS) zero), out[h, r, :] streamed beside them, and
//       t_h reduced by the fixed 64-lane butterfly: the same number in every item holding a
//       piece of the row.  Lane h < H of every group keeps s_dst, row_max, row_sum and t of
//       head h.
//     * per edge: one col_idx load, one packed record (value and selector) and, by lane
//       h < HP of the group alone, head h's score out of the column's ss_t vector, its alpha
//       (one expf and one division per edge and head) and the sign of z.
//     * per head: x = g_h[selector] is read from LDS once; ga_h = the group's butterfly sum of
//       value * x over the kept slots (a folded or skipped selector adds nothing), kept by lane
//       h; T[e, l] gains alpha_h * x in head order (a product for head 0, one fma per further
//       head, as sspmm_bwd_heads_kernel).  The record's low selector byte is the caller's
//       selector, so a repeated selector's slot receives its gradient although the pack folded
//       its value; a selector >= D reads the zero pad.
//     * lane h then forms gz_h; the group's HP lanes store gzT[e, 0:HP] (pad heads 0), all
//       lanes the contribution row T[e, 0:k].  k > 64: ga in passes over l per head, then T in
//       passes over l, the record reloaded from the caches.
//     * grad_s_dst: lane h adds its gz over the piece, the groups are added in group order; a
//       row inside one item is stored, a cut row leaves its pieces' sums in the slots (slot 2i
//       the item's continuation, 2i + 1 its cut last row) and esmh_merge_kernel adds them in
//       item order.  A row without edges stores 0.
//  3. launch_heads_colsum: grad_s_src from gzT through the CSC, in slot order.
//  4. csc_sum_rows: grad_cbsr from T through the CSC, in slot order (the csc phase 2).
// No global atomics, no LDS atomics; every sum has an order fixed by (graph, chunk, k, H).  Head
// h's score gradients are computed from head h's scores, statistics, out and grad_out alone.
// maxk_gat_attention_heads_dropout_backward is the same walk under the attention-dropout mask of
// attn_dropout.h (the DROP instantiations): gz = alpha * (d * ga - t) * (z > 0 ? 1 : slope) and
// T gains alpha * d * x; t is still out . grad_out, out being the dropped forward's, since
// sum_e alpha_e d_e ga_e is that dot product.  p == 0 launches the kernels without a mask.
#include <cmath>

#include "attn_dropout.h"
#include "edge_softmax.h"
#include "piece_walk.h"
#include "sspmm_bwd.h"

// Wave steps of record loads in flight.  4: 97 to 122 VGPRs over the twelve instantiations (four
// waves per SIMD), no scratch; 8 takes 133 to 165 (three waves).  The depth of the multi-head
// phase 1 it replaces (kHeadsDepth).
#ifndef MAXK_GATB_U
#define MAXK_GATB_U 4
#endif

namespace maxk {
namespace {

// What lane h of a group holds of head h for the row being walked (pad heads: 0, 0, 1, 0).
struct HeadLane {
    float sd, shift, sum, t;
};

// The edges [sb, se) (sb < se) of one row whose grad_out rows are staged in grow: stores their
// T rows and gzT vectors; returns this lane's sum of the gz of head lane % KG over its group's
// edges (lanes % KG >= H: 0).  DROP: lane h takes its head's bits of the step from step_gone
// (attn_dropout.h) and keeps d = 0 or scale beside alpha: T gains alpha * d * x and
// gz = alpha * (d * ga - t), t from the dropped out.
template <int KG, int HP, int U, bool DROP>
__device__ __forceinline__ float walk_piece_bwd(const float *grow, int DS,
                                                const int32_t *__restrict__ col_idx,
                                                const float *__restrict__ ss,
                                                const uint8_t *__restrict__ rec, int RS,
                                                float *__restrict__ T, float *__restrict__ gzT,
                                                int H, int D, int sb, int se, int k,
                                                const HeadLane &hd, float slope, int lane,
                                                const MaskArg<DROP> &dm) {
    constexpr int G = kWave / KG;
    const int grp = lane / KG, l0 = lane % KG;
    const int lane0 = lane - l0;  // the group's first lane
    const int trash = DS - 1;
    const int n = se - sb;  // wave-uniform, <= chunk <= kBwdMaxChunk
    const bool hl = l0 < HP, hon = l0 < H;
    const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
    const auto rrs = wave_buffer(rec, 0xffffffffu);  // offsets < num_cols * RS < 2^32
    const auto trs = wave_buffer(T + (size_t)(uint32_t)sb * k, (uint32_t)n * (uint32_t)k * 4u);
    const auto zrs = wave_buffer(gzT + (size_t)(uint32_t)sb * HP, (uint32_t)n * HP * 4u);
    float gsum = 0.f;
    for (int base = 0; base < n; base += G * U) {
        int c[U];
#pragma unroll
        for (int u = 0; u < U; ++u)  // past the piece's end the column reads 0 (column 0)
            c[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(crs, (base + u * G + grp) * 4, 0, 0);
        // lane h of the group: head h's coefficient of each of the group's U edges
        float al[U];
        uint32_t pos = 0u;
#pragma unroll
        for (int u = 0; u < U; ++u) al[u] = 0.f;
        if (hl) {
            float x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = ss[(uint32_t)c[u] * (uint32_t)HP + (uint32_t)l0];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float z = hd.sd + x[u];
                const float p = expf(leaky(z, slope) - hd.shift);
                al[u] = hon ? p / hd.sum : 0.f;
                pos |= (z > 0.f ? 1u : 0u) << u;
            }
        }
        // DROP, lane h: bit u, head h of the group's edge u is dropped
        const uint32_t gone = step_gone<KG, HP, U, DROP>(dm, sb + base, grp, l0, lane0);
        auto dk = [&](int u) {  // the mask factor d
            if constexpr (DROP) return (gone >> u) & 1u ? 0.f : dm.scale;
            else return 1.f;
        };
        // the coefficient of the feature gradient: alpha, under DROP alpha * d
        float ad[DROP ? U : 1];
        if constexpr (DROP) {
#pragma unroll
            for (int u = 0; u < U; ++u) ad[u] = al[u] * dk(u);
        }
        auto coef = [&](int u) {
            if constexpr (DROP) return ad[u];
            else return al[u];
        };
        float ga[U];
#pragma unroll
        for (int u = 0; u < U; ++u) ga[u] = 0.f;
        if (k <= KG) {  // one slot per lane: the record is loaded once for all heads
            const RecordSlot sl(l0, k);
            const PackedSrc src = sl.src(rrs, k, RS);
            float v[U];
            int s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) src.load(c[u], v[u], s[u]);
            const uint32_t keep = caller_columns(s, sl.ok, D, trash);
            float tc[U];
#pragma unroll
            for (int h = 0; h < HP; ++h) {
                if (h < H) {
                    const float *gh = grow + h * DS;
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const float x = gh[s[u]];
                        const float a = __shfl(coef(u), lane0 + h);
                        // a slot without a kept value adds nothing, whatever x is
                        const float d = lane_tree<KG, Sum>((keep >> u) & 1u ? v[u] * x : 0.f);
                        ga[u] = l0 == h ? d : ga[u];
                        tc[u] = h == 0 ? a * x : __builtin_fmaf(a, x, tc[u]);
                    }
                }
            }
            store_t_rows<KG, U>(trs, tc, sl.ok, base, grp, k, l0);
        } else {  // k > 64 (KG == 64, one edge per wave step): passes over l
#pragma unroll
            for (int h = 0; h < HP; ++h) {
                if (h < H) {
                    const float *gh = grow + h * DS;
                    float acc[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) acc[u] = 0.f;
                    for (int lb = 0; lb < k; lb += KG) {
                        const RecordSlot sl(lb + l0, k);
                        const PackedSrc src = sl.src(rrs, k, RS);
                        float v[U];
                        int s[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) src.load(c[u], v[u], s[u]);
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const bool keep = sl.ok && s[u] < 0x100;
                            const float x = gh[min(s[u], trash)];
                            acc[u] = keep ? __builtin_fmaf(v[u], x, acc[u]) : acc[u];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const float d = lane_tree<KG, Sum>(acc[u]);
                        ga[u] = l0 == h ? d : ga[u];
                    }
                }
            }
            for (int lb = 0; lb < k; lb += KG) {
                const RecordSlot sl(lb + l0, k);
                const PackedSrc src = sl.src(rrs, k, RS);
                float v[U], tc[U];
                int s[U];
#pragma unroll
                for (int u = 0; u < U; ++u) src.load(c[u], v[u], s[u]);
                caller_columns(s, sl.ok, D, trash);
#pragma unroll
                for (int h = 0; h < HP; ++h) {
                    if (h < H) {
                        const float *gh = grow + h * DS;
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const float x = gh[s[u]];
                            const float a = __shfl(coef(u), lane0 + h);
                            tc[u] = h == 0 ? a * x : __builtin_fmaf(a, x, tc[u]);
                        }
                    }
                }
                store_t_rows<KG, U>(trs, tc, sl.ok, base, grp, k, lb + l0);
            }
        }
        // lane h: gz of head h (a pad head: 0 * (0 - 0)), one vector per edge from the HP lanes
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = base + u * G + grp;
            float gz;
            if constexpr (DROP) gz = al[u] * (dk(u) * ga[u] - hd.t);
            else gz = al[u] * (ga[u] - hd.t);
            gz *= (pos >> u) & 1u ? 1.f : slope;
            gsum += hon && i < n ? gz : 0.f;
            __builtin_amdgcn_raw_buffer_store_b32(
                __float_as_uint(gz), zrs, hl && i < n ? (i * HP + l0) * 4 : (int)0x80000000, 0, 0);
        }
    }
    return gsum;
}

// DROP: held to the four waves per SIMD of the kernels without a mask.
template <int KG, int HP, int U, bool DROP>
__global__ __launch_bounds__(kBlock, DROP ? 4 : 1) void gath_bwd_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const float *__restrict__ ss, const float *__restrict__ s_dst, float slope,
    const uint8_t *__restrict__ rec, int RS, const float *__restrict__ out,
    const float *__restrict__ row_max, const float *__restrict__ row_sum,
    const float *__restrict__ grad_out, float *__restrict__ T, float *__restrict__ gzT,
    float *__restrict__ grad_s_dst, SlotsH sl, int num_rows, int64_t num_e, int D, int DS, int k,
    int chunk, int n_items, int H, int vec, MaskArg<DROP> dm) {
    constexpr int G = kWave / KG;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wid = threadIdx.x / kWave;
    const int lane = lane_id();
    const int item = item_of_wave(n_items);
    if (item < 0) return;  // whole wave; no workgroup barrier below
    float *grow = lds + (size_t)wid * H * DS;
    // the pad columns [D, DS) of every head's row are never staged over: zeroed once
    for (int h = 0; h < H; ++h)
        if (lane < DS - D) grow[h * DS + D + lane] = 0.f;
    const int l0 = lane % KG;

    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);
    // slot values of lane h < H: the continuation's sum and the cut last row's
    int head_row = -1, tail_row = -1;
    float head_v = 0.f, tail_v = 0.f;
    // Rows q = r - 1 (the continuation: its token precedes the item), r, r + 1, ...: each one's
    // piece under CutAtEnd, through one walk site, so t is formed by the same instructions in
    // every item that holds a piece of a row.
    int q = it.r - 1;
    bool cont = true;
    int64_t rb = 0, re = 0;
    RowPiece p{0, 0, false};
    if (it.r > 0) p = cont_piece(CutAtEnd{}, it.p_lo, it.d1, it.r, row_ptr[it.r]);
    for (;;) {
        if (q >= 0 && p.sb < p.se) {
            HeadLane hd{0.f, 0.f, 1.f, 0.f};
            if (l0 < H) {
                const int64_t o = (int64_t)l0 * num_rows + q;
                hd.sd = s_dst[o];
                hd.shift = shift_of(row_max[o]);
                hd.sum = row_sum[o];
            }
            wave_lds_fence();  // the previous piece's reads of grow are done
            for (int h = 0; h < H; ++h) {
                const int64_t o = ((int64_t)h * num_rows + q) * D;
                const float th = lane_tree<kWave, Sum>(
                    stage_dot(grow + h * DS, grad_out + o, out + o, D, vec != 0, lane));
                hd.t = l0 == h ? th : hd.t;
            }
            wave_lds_fence();
            const float gsum = walk_piece_bwd<KG, HP, U, DROP>(grow, DS, col_idx, ss, rec, RS, T,
                                                               gzT, H, D, (int)p.sb, (int)p.se, k,
                                                               hd, slope, lane, dm);
            float tot = 0.f;  // head l0's sum over the piece: the groups in group order
#pragma unroll
            for (int g = 0; g < G; ++g) tot += __shfl(gsum, g * KG + l0);
            if (cont) {
                head_row = q;
                head_v = tot;
            } else if (p.se == re) {
                if (lane < H) grad_s_dst[(int64_t)lane * num_rows + q] = tot;
            } else {
                tail_row = q;
                tail_v = tot;
            }
        } else if (!cont && q >= 0 && re == rb) {  // a row without edges
            if (lane < H) grad_s_dst[(int64_t)lane * num_rows + q] = 0.f;
        }
        cont = false;
        ++q;
        if (q >= num_rows) break;
        rb = row_ptr[q];
        if (!row_owned(it.d1, q, rb)) break;  // row q's token belongs to a later item
        re = row_ptr[q + 1];
        p = row_piece(CutAtEnd{}, it.d1, q, rb, re);
    }
    if (lane == 0) {
        sl.row[2 * item] = head_row;
        sl.row[2 * item + 1] = tail_row;
    }
    if (lane < H) {
        float *a = sl.a + lane * sl.stride;
        a[2 * item] = head_v;
        a[2 * item + 1] = tail_v;
    }
}

// Resident waves per CU the items are sized for: four per SIMD by VGPRs, fewer where the staged
// rows fill the LDS first.
constexpr int kBwdResident = 16;

// Workspace: [T (num_e + 1 rows) and the phase-2 slabs | records | ss_t | gzT | row slots x H |
// column slots x H].
struct BwdLayout : RecordGeom {
    int chunk, n_items, hp;
    size_t rec_off, ss_off, gz_off, srow_off, sa_off, total;
    int64_t sstride;  // floats between two heads' row slots
    SlotLayoutH cols;
};

BwdLayout bwd_layout(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k, int H,
                     int chunk) {
    BwdLayout L{record_geom(num_cols, D, k)};
    L.hp = hp_of(H);
    const size_t per_block = (size_t)kWavesPerBlock * H * L.DS * sizeof(float);
    L.chunk = walk_chunk(num_rows, num_e, chunk, per_block, kBwdResident, kBwdMaxChunk);
    L.n_items = token_items(num_rows, num_e, L.chunk);
    const int64_t cap = item_cap(num_rows + num_e, chunk, L.n_items);
    const size_t part = al256((size_t)cap * 2 * sizeof(float));
    const size_t vec = (size_t)L.hp * sizeof(float);
    L.rec_off = csc_sum_workspace_size(num_cols, num_e, k, chunk);
    L.ss_off = L.rec_off + al256((size_t)num_cols * L.RS);
    L.gz_off = L.ss_off + al256((size_t)num_cols * vec);
    L.srow_off = L.gz_off + al256((size_t)num_e * vec);
    L.sa_off = L.srow_off + part;
    L.sstride = (int64_t)(part / sizeof(float));
    L.cols = slot_layout_h(num_cols, num_e, chunk, H, L.sa_off + (size_t)H * part);
    L.total = L.cols.end;
    return L;
}

template <int HP, bool DROP>
int launch_attention_bwd(const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr,
                         const int32_t *csc_eid, const float *s_dst, const float *s_src,
                         float slope, const float *cbsr_val, const uint8_t *cbsr_idx,
                         const float *out, const float *row_max, const float *row_sum,
                         const float *grad_out, float *grad_s_dst, float *grad_s_src,
                         float *grad_cbsr, int64_t num_rows, int64_t num_cols, int64_t num_e,
                         int D, int k, int H, int chunk_edges, const BwdLayout &L, void *workspace,
                         hipStream_t s, const MaskArg<DROP> &dm) {
    char *ws = reinterpret_cast<char *>(workspace);
    float *T = reinterpret_cast<float *>(ws);
    uint8_t *rec = reinterpret_cast<uint8_t *>(ws + L.rec_off);
    VecF<HP> *ss_t = reinterpret_cast<VecF<HP> *>(ws + L.ss_off);
    VecF<HP> *gzT = reinterpret_cast<VecF<HP> *>(ws + L.gz_off);
    float *sa = reinterpret_cast<float *>(ws + L.sa_off);
    const SlotsH sl{reinterpret_cast<int32_t *>(ws + L.srow_off), sa, sa, L.sstride};
    if (int rc = launch_cbsr_pack(cbsr_val, cbsr_idx, rec, num_cols, k, L.RS, D, L.DS - 1, s))
        return rc;
    hipLaunchKernelGGL(esmh_interleave_kernel<HP>, dim3((unsigned)ceil_div(num_cols, kBlock)),
                       dim3(kBlock), 0, s, s_src, ss_t, H, num_cols);
    MAXK_LAUNCHED("esmh_interleave_kernel");
    constexpr int U = MAXK_GATB_U;
    const size_t lds = (size_t)kWavesPerBlock * H * L.DS * sizeof(float);
    const int vec = D % 4 == 0 && ((uintptr_t)grad_out & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const bool ok = with_const<8, 16, 32, 64>(L.kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        hipLaunchKernelGGL((gath_bwd_kernel<KG, HP, U, DROP>), item_grid(L.n_items), dim3(kBlock), lds,
                           s, row_ptr, col_idx, reinterpret_cast<const float *>(ss_t), s_dst,
                           slope, rec, L.RS, out, row_max, row_sum, grad_out, T,
                           reinterpret_cast<float *>(gzT), grad_s_dst, sl, (int)num_rows, num_e,
                           D, L.DS, k, L.chunk, L.n_items, H, vec, dm);
    });
    if (!ok) return bad_lanes(L.kg);
    MAXK_LAUNCHED("gath_bwd_kernel");
    hipLaunchKernelGGL((esmh_merge_kernel<kMergeOut, false>), with_heads(slot_grid(L.n_items), H),
                       dim3(kBlock), 0, s, sl, grad_s_dst, num_rows, 2 * L.n_items);
    MAXK_LAUNCHED("esmh_merge_kernel");
    if (int rc = launch_heads_colsum<HP>(col_ptr, csc_eid, gzT, grad_s_src, workspace, L.cols, H,
                                         num_cols, num_e, s))
        return rc;
    return csc_sum_rows(s, col_ptr, csc_eid, ws, grad_cbsr, num_cols, num_e, k, chunk_edges);
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" size_t maxk_gat_attention_heads_backward_workspace_size(
    int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
    int32_t num_heads, int32_t chunk_edges) {
    if (num_rows < 0 || num_cols < 0 || num_e < 0 || dim_origin <= 0 || dim_k <= 0 ||
        chunk_edges < 0 || num_heads < 1 || num_heads > MAXK_MAX_HEADS)
        return 0;
    return bwd_layout(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads, chunk_edges).total;
}

namespace {
// Both backward entries; dm: the dropout entry's mask, null for none.
int attention_heads_backward(
    const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr,
    const int32_t *csc_eid, const float *s_dst, const float *s_src, float negative_slope,
    const float *cbsr_val, const uint8_t *cbsr_idx, const float *out, const float *row_max,
    const float *row_sum, const float *grad_out, float *grad_s_dst, float *grad_s_src,
    float *grad_cbsr, int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin,
    int32_t dim_k, int32_t num_heads, int32_t chunk_edges, void *workspace,
    size_t workspace_bytes, void *stream, const DropMask *dm) {
    if (int rc = check_heads(num_heads)) return rc;
    if (int rc = check_sizes(num_rows, num_cols, num_e, chunk_edges)) return rc;
    if (int rc = check_slope(negative_slope)) return rc;
    if (int rc = check_cbsr_dims(dim_origin, dim_k, num_cols)) return rc;
    MAXK_REQUIRE((grad_s_dst || num_rows == 0) && ((grad_s_src && grad_cbsr) || num_cols == 0),
                 "grad_s_dst / grad_s_src / grad_cbsr must not be NULL");
    const int D = dim_origin, k = dim_k, H = num_heads;
    hipStream_t s = as_stream(stream);
    if (num_e == 0) {  // nothing to walk: all three gradients are zeros
        if (num_rows > 0)
            if (int rc = zero_words(grad_s_dst, (int64_t)H * num_rows, s)) return rc;
        if (num_cols == 0) return MAXK_OK;
        if (int rc = zero_words(grad_s_src, (int64_t)H * num_cols, s)) return rc;
        return zero_words(grad_cbsr, num_cols * k, s);
    }
    MAXK_REQUIRE(num_rows > 0 && num_cols > 0, "edges present but num_rows or num_cols == 0");
    MAXK_REQUIRE(row_ptr && col_idx && col_ptr && csc_eid,
                 "row_ptr / col_idx / col_ptr / csc_eid must not be NULL");
    MAXK_REQUIRE(s_dst && s_src && cbsr_val && cbsr_idx,
                 "s_dst / s_src / cbsr_val / cbsr_idx must not be NULL");
    MAXK_REQUIRE(out && row_max && row_sum && grad_out,
                 "out / row_max / row_sum / grad_out must not be NULL");
    const BwdLayout L = bwd_layout(num_rows, num_cols, num_e, D, k, H, chunk_edges);
    MAXK_REQUIRE(!L.wide, "num_cols: the fused attention backward takes tables below 2^24 columns "
                 "and 4 GiB of records (%lld columns of %d bytes)", (long long)num_cols, L.RS);
    if (int rc = check_workspace(workspace, workspace_bytes, L.total)) return rc;
    MAXK_REQUIRE(((uintptr_t)cbsr_val & 3) == 0 && ((uintptr_t)s_dst & 3) == 0 &&
                     ((uintptr_t)s_src & 3) == 0 && ((uintptr_t)out & 3) == 0 &&
                     ((uintptr_t)row_max & 3) == 0 && ((uintptr_t)row_sum & 3) == 0 &&
                     ((uintptr_t)grad_out & 3) == 0 && ((uintptr_t)grad_s_dst & 3) == 0 &&
                     ((uintptr_t)grad_s_src & 3) == 0 && ((uintptr_t)grad_cbsr & 3) == 0,
                 "float buffers must be 4-B aligned");
    return with_heads_mask(L.hp, dm, [&](auto hp_c, const auto &mask) {
        return launch_attention_bwd<decltype(hp_c)::value, is_drop_v<decltype(mask)>>(
            row_ptr, col_idx, col_ptr, csc_eid, s_dst, s_src, negative_slope, cbsr_val, cbsr_idx,
            out, row_max, row_sum, grad_out, grad_s_dst, grad_s_src, grad_cbsr, num_rows, num_cols,
            num_e, D, k, H, chunk_edges, L, workspace, s, mask);
    });
}
}  // namespace

extern "C" int maxk_gat_attention_heads_backward(
    const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr,
    const int32_t *csc_eid, const float *s_dst, const float *s_src, float negative_slope,
    const float *cbsr_val, const uint8_t *cbsr_idx, const float *out, const float *row_max,
    const float *row_sum, const float *grad_out, float *grad_s_dst, float *grad_s_src,
    float *grad_cbsr, int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin,
    int32_t dim_k, int32_t num_heads, int32_t chunk_edges, void *workspace,
    size_t workspace_bytes, void *stream) {
    clear_error();
    return attention_heads_backward(row_ptr, col_idx, col_ptr, csc_eid, s_dst, s_src, negative_slope,
                                    cbsr_val, cbsr_idx, out, row_max, row_sum, grad_out,
                                    grad_s_dst, grad_s_src, grad_cbsr, num_rows, num_cols, num_e,
                                    dim_origin, dim_k, num_heads, chunk_edges, workspace,
                                    workspace_bytes, stream, nullptr);
}

extern "C" size_t maxk_gat_attention_heads_dropout_backward_workspace_size(
    int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
    int32_t num_heads, int32_t chunk_edges) {
    return maxk_gat_attention_heads_backward_workspace_size(num_rows, num_cols, num_e, dim_origin,
                                                            dim_k, num_heads, chunk_edges);
}

extern "C" int maxk_gat_attention_heads_dropout_backward(
    const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr,
    const int32_t *csc_eid, const float *s_dst, const float *s_src, float negative_slope,
    const float *cbsr_val, const uint8_t *cbsr_idx, const float *out, const float *row_max,
    const float *row_sum, const float *grad_out, float *grad_s_dst, float *grad_s_src,
    float *grad_cbsr, int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin,
    int32_t dim_k, int32_t num_heads, int32_t chunk_edges, float p, uint64_t seed,
    void *workspace, size_t workspace_bytes, void *stream) {
    clear_error();
    return with_dropout(p, seed, [&](const DropMask *dm) {
        return attention_heads_backward(row_ptr, col_idx, col_ptr, csc_eid, s_dst, s_src,
                                        negative_slope, cbsr_val, cbsr_idx, out, row_max, row_sum,
                                        grad_out, grad_s_dst, grad_s_src, grad_cbsr, num_rows,
                                        num_cols, num_e, dim_origin, dim_k, num_heads, chunk_edges,
                                        workspace, workspace_bytes, stream, dm);
    });
}
