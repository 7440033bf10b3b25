// Fused multi-head dot-product attention on CBSR keys for gfx950: the scaled dot-product score
// and its edge softmax inside the aggregation walk,
//
//   l_he = scale * sum_l cbsr_val[c, l] * q[h, r, cbsr_idx[c, l]]     e in row r, c = col_idx[e]
//   m_hr = max_e l_he      z_hr = sum_e exp(l_he - m_hr)      alpha_he = exp(l_he - m_hr) / z_hr
//   out[h, r, cbsr_idx[c, l]] += alpha_he * cbsr_val[c, l]
//
// what maxk_edge_weight_grad_heads (grad_out := q), the scale, H edge softmaxes and
// maxk_spgemm_forward_heads compute, without logits or alpha [H, E] ever existing.  The score and
// the aggregation read the same packed record of column c, so the walk gathers it for both.  The
// walk is the hub-row heads walk of heads_walk.h, shared with spgemm_fwd_heads.hip and
// gat_attention_heads.hip (records packed once, token-stream items, one wavefront per item under
// CutHubRows, KG lanes per group, G = 64 / KG LDS copies of the output row, the heads in passes
// of HC, the fix-up of the cut rows; its rules are stated there); the logit is a record's dot
// product with a staged row (piece_walk.h, dot_logit.h: the H rows q[h, r, :] of the piece staged
// side by side in LDS, one fma per slot and a fixed butterfly per logit):
//
//  1. launch_cbsr_pack fills the workspace's records.
//  2. dath_fwd_kernel, per row piece: the H query rows are staged as scale * q (one rounding per
//     element, none when scale is a power of two), so a logit is the plain dot product of the
//     record and the staged row;
//     * sweep 1, one group per edge: the record loaded once, one fma chain and one butterfly per
//       head, the piece's maximum per head by a fixed butterfly over the wave;
//     * sweep 2, per pass of HC heads, group g on (edge g / HC, head g % HC): the record again
//       (the line sweep 1 fetched), the logit of its head by the same device functions as sweep
//       1 -- so the maximum is the exact maximum of the values exponentiated, p <= 1 and
//       z_piece >= 1 -- p = exp(l - m_piece), acc += p * value in the group's LDS copy and the
//       lane's own sum of p.  Nothing in LDS is ever rescaled: an online softmax would rescale
//       G * D floats of LDS per new maximum, and the second logit costs one LDS read and one
//       butterfly on a record that is loaded for the aggregation anyway;
//     * a row inside one item is stored as acc / z with (m, z); a hub row's pieces are stored
//       unnormalised, the owner's into out and the statistics, a continuation's into the item's
//       slab [H, n_items, D] and slab statistics [H, n_items].
//  3. softmax_fixup_kernel (heads_walk.h) merges a hub row's pieces in item order.
// A row whose z is not a positive number (a NaN or +Inf logit: z is NaN; only -Inf logits: z = 0)
// is NaN wherever it has an addend and exactly 0 elsewhere: such rows are walked once more with
// the weight NaN and stored undivided.  A row without edges stores zeros in out and both
// statistics.  A query column no neighbour selects is never read from LDS: a NaN there reaches
// nothing (the pad columns [D, DS) hold zeros and a skipped selector carries the value 0).
// maxk_dot_edge_alpha_heads is a staged-row walk (piece_walk.h: CutAtEnd, no slab) with the
// epilogue w = exp(l - row_max) / row_sum; its logit is sweep 1's.
// No global atomics, no LDS atomics; every sum has an order fixed by (graph, chunk, k, H), so the
// result is bitwise repeatable, and head h's slice is computed from head h's query only.
// LDS per wave: (H + G) * DS floats (16.6 KB at H = 8, G = 8, D = 256; 12.5 KB at k = 16).
// maxk_dot_attention_heads_dropout is the same walk with the attention-dropout mask of
// attn_dropout.h multiplied in (the DROP instantiations): out sums alpha * d * value, the
// statistics stay those of the undropped softmax, p == 0 launches the kernels without a mask.
#include <cmath>

#include "attn_dropout.h"
#include "dot_logit.h"

// Waves per SIMD the masked forward is compiled for (1: whatever its registers allow).
#ifndef MAXK_DATH_DROP_WAVES
#define MAXK_DATH_DROP_WAVES 4
#endif

namespace maxk {
namespace {

// Sweep 1 over the edges [sb, sb + n) (n >= 1) of a piece whose query rows are staged: m[h] = the
// piece's largest logit of head h (-inf for h >= H), wave-uniform.  One group per edge.
template <int KG, int U>
__device__ __forceinline__ void piece_max(const float *qrow, const int32_t *__restrict__ col,
                                          const uint8_t *__restrict__ rec, int RS, int n, int H,
                                          int DS, int k, int trash, int lane, float (&m)[kMaxH]) {
    constexpr int G = kWave / KG;
    const int grp = lane / KG, l0 = lane % KG;
    const auto crs = wave_buffer(col, (uint32_t)n * 4u);
    const auto rrs = wave_buffer(rec, 0xffffffffu);  // offsets < num_cols * RS < 2^32
    for (int base = 0; base < n; base += G * U) {
        int c[U];
#pragma unroll
        for (int u = 0; u < U; ++u)  // past the piece's end the column reads 0 (column 0's record)
            c[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(crs, (base + u * G + grp) * 4, 0, 0);
        if (k <= KG) {  // one slot per lane: the record is loaded once for all heads
            const RecordSlot sl(l0, k);
            const PackedSrc src = sl.src(rrs, k, RS);
            float v[U];
            int s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) src.load(c[u], v[u], s[u]);
#pragma unroll
            for (int h = 0; h < kMaxH; ++h) {
                if (h < H) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const float l = lane_tree<KG, Sum>(
                            dot_term(v[u], s[u], qrow + h * DS, trash, sl.ok, 0.f));
                        m[h] = fmaxf(m[h], base + u * G + grp < n ? l : -INFINITY);
                    }
                }
            }
        } else {
#pragma unroll
            for (int h = 0; h < kMaxH; ++h) {
                if (h < H) {
                    float l[U];
                    record_dots<KG, U>(rrs, RS, c, qrow + h * DS, k, trash, l0, l);
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        m[h] = fmaxf(m[h], base + u * G + grp < n ? l[u] : -INFINITY);
                }
            }
        }
    }
#pragma unroll
    for (int h = 0; h < kMaxH; ++h)
        if (h < H) m[h] = uniform(lane_tree<kWave, Max>(m[h]));
}

// Sweep 2 of one pass over the edges [sb, se) (sb < se): this lane's group adds p * value into
// its copy acc_g for the edges base + u * EP + eg it is given, p = exp(l - shift) with l its
// head's logit against qh; returns the lane's sum of p (the same in every lane of a group).
// active: the group has an edge slot and a head in this pass; else it writes its trash column
// only.  POISON: p = NaN and nothing is summed (the rows whose z is no positive number).
// DROP: the pass mask of attn_dropout.h (PassMask) multiplied into the products; the sum of p
// takes the unmasked weights.
template <int KG, int U, bool POISON, bool DROP>
__device__ __forceinline__ float walk_dot(float *acc_g, const float *qh,
                                          const int32_t *__restrict__ col_idx, float shift,
                                          const uint8_t *__restrict__ rec, int RS, int sb, int se,
                                          int k, int trash, int EP, int eg, bool active, int lane,
                                          const MaskArg<DROP> &dm, const DropPass &dp) {
    static_assert(!(POISON && DROP), "the NaN walk has no mask");
    const int l0 = lane % KG;
    const int n = se - sb;  // wave-uniform, <= 2 * chunk
    const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
    const auto rrs = wave_buffer(rec, 0xffffffffu);
    float ps = 0.f;
    PassMask<DROP> pm(dp, EP * U);
    for (int base = 0; base < n; base += EP * U) {
        int c[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            c[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(crs, (base + u * EP + eg) * 4, 0, 0);
        float keep[DROP ? U : 1];  // DROP: 0 where the group's head of slot u is dropped, else 1
        if constexpr (DROP) {
            pm.refresh(dm, dp, sb + base, lane);
#pragma unroll
            for (int u = 0; u < U; ++u) keep[u] = pm.keep(u * EP + eg);
            pm.next();
        }
        if (k <= KG) {  // the slot's value and selector serve the logit and the product
            const RecordSlot sl(l0, k);
            const PackedSrc src = sl.src(rrs, k, RS);
            float v[U];
            int s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) src.load(c[u], v[u], s[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool live = active && base + u * EP + eg < n;
                float p;
                if constexpr (POISON) {
                    p = live ? NAN : 0.f;
                } else {
                    const float l = lane_tree<KG, Sum>(dot_term(v[u], s[u], qh, trash, sl.ok, 0.f));
                    p = live ? expf(l - shift) : 0.f;
                    ps += p;
                    if constexpr (DROP) p *= keep[u];
                }
                float *a = &acc_g[live && sl.ok ? min(s[u], trash) : trash];
                *a = __builtin_fmaf(p, v[u], *a);
            }
        } else {
            float p[U];
            if constexpr (POISON) {
#pragma unroll
                for (int u = 0; u < U; ++u) p[u] = active && base + u * EP + eg < n ? NAN : 0.f;
            } else {
                float l[U];
                record_dots<KG, U>(rrs, RS, c, qh, k, trash, l0, l);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    p[u] = active && base + u * EP + eg < n ? expf(l[u] - shift) : 0.f;
                    ps += p[u];
                    if constexpr (DROP) p[u] *= keep[u];
                }
            }
            scatter_records<KG, U>(acc_g, rrs, RS, k, trash, l0, c, p, active, base, EP, eg, n);
        }
    }
    return ps;
}

// DROP: held to the four waves per SIMD of the kernel without a mask (128 VGPRs); the Philox
// rounds then spill 28 bytes per lane (84 at KG = 32) around the once-in-S-steps evaluation
// instead of taking 142 to 151 VGPRs and three waves (MAXK_DATH_DROP_WAVES=1;
// profiles/r22/dot_attn_dropout/).
template <int KG, int U, bool DROP>
__global__ __launch_bounds__(kBlock, DROP ? MAXK_DATH_DROP_WAVES : 1) void dath_fwd_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const float *__restrict__ q, float scale, const uint8_t *__restrict__ rec, int RS,
    float *__restrict__ out, float *__restrict__ row_max, float *__restrict__ row_sum,
    float *__restrict__ slab, float *__restrict__ slab_m, float *__restrict__ slab_z,
    int32_t *__restrict__ slab_row, int num_rows, int64_t num_e, int D, int DS, int k, int chunk,
    int n_items, int H, int HC, int flags, MaskArg<DROP> dm) {
    // flags: store_flags (heads_walk.h), and bit 2 16-B query loads (D % 4 == 0, q 16-B aligned)
    constexpr int G = kWave / KG;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = lane_id();
    const int item = wave_item();
    if (item >= n_items) return;  // whole wave; no workgroup barrier below
    float *qrow = lds + (size_t)(threadIdx.x / kWave) * (H + G) * DS;
    float *acc = qrow + H * DS;
    zero_wave_lds(qrow, (H + G) * DS, lane);
    const PassGeom<KG> g(lane, HC, acc, DS);
    const bool vec = flags & 1, nt = flags & 2, qvec = flags & 4;

    // Edges [sb, se) of row r: an owned row's into out and the row statistics, a continuation's
    // into the item's slab and slab statistics.  Every head is stored, an empty piece as zeros.
    walk_hub_item(row_ptr, slab_row, num_rows, num_e, item, chunk, lane,
                  [&](int r, int64_t sb, int64_t se, bool whole, bool to_out) {
        float *__restrict__ dst = to_out ? out + (int64_t)r * D : slab + (int64_t)item * D;
        const int64_t hstride = (int64_t)(to_out ? num_rows : n_items) * D;
        float *__restrict__ st_m = to_out ? row_max + r : slab_m + item;
        float *__restrict__ st_z = to_out ? row_sum + r : slab_z + item;
        const int64_t st_stride = to_out ? num_rows : n_items;
        const int n = (int)(se - sb);
        float m[kMaxH];
#pragma unroll
        for (int h = 0; h < kMaxH; ++h) m[h] = -INFINITY;
        if (n > 0) {
            wave_lds_fence();  // the previous piece's reads of qrow are done
            stage_query(qrow, q, r, num_rows, H, D, DS, scale, qvec, lane);
            wave_lds_fence();
            piece_max<KG, U>(qrow, col_idx + sb, rec, RS, n, H, DS, k, DS - 1, lane, m);
        }
        for (int h0 = 0; h0 < H; h0 += HC) {
            const int head = h0 + g.hh;
            const bool active = g.grp_ok && head < H;
            float mh = -INFINITY;
#pragma unroll
            for (int h = 0; h < kMaxH; ++h)
                if (h == head) mh = m[h];
            const float *qh = qrow + (head < H ? head : H - 1) * DS;
            float ps = 0.f;
            wave_lds_fence();
            if (n > 0)
                ps = walk_dot<KG, U, false, DROP>(
                    g.acc_g, qh, col_idx, shift_of(mh), rec, RS, (int)sb, (int)se, k, DS - 1, g.EP,
                    g.eg, active, lane, dm, drop_pass(h0, HC, H, head));
            const int bad = bad_heads<KG>(ps, g.EP, HC, h0, H);
            if (whole && n > 0 && bad) {  // rare: NaN wherever such a head's row has an addend
                wave_lds_fence();
                walk_dot<KG, U, true, false>(g.acc_g, qh, col_idx, 0.f, rec, RS, (int)sb, (int)se,
                                             k, DS - 1, g.EP, g.eg, active && ((bad >> g.hh) & 1),
                                             lane, NoMask{}, DropPass{0, 1, 0});
            }
            wave_lds_fence();
            for (int j = 0; j < HC && h0 + j < H; ++j) {
                const float zj = pass_z<KG>(ps, j, g.EP, HC);
                const bool ok = !((bad >> j) & 1);
                float mul = 1.f;
                if constexpr (DROP) mul = dm.scale;
                flush_head<DROP>(acc + j * DS, g.EP, HC * DS, dst + (int64_t)(h0 + j) * hstride, D,
                                 zj, whole && ok, vec, nt && to_out, lane, mul);
                // the head's maximum sits in the lanes of group j (edge slot 0, head h0 + j)
                const float mj = uniform(__shfl(mh, j * KG));
                if (lane == 0) {
                    st_m[(int64_t)(h0 + j) * st_stride] = whole && n == 0 ? 0.f : mj;
                    st_z[(int64_t)(h0 + j) * st_stride] = zj;
                }
            }
        }
        wave_lds_fence();
    });
}

// ---- w[h, e] = exp(l_he - row_max[h, r]) / row_sum[h, r] ----------------------------------------
// The staged-row walk of piece_walk.h with the softmax epilogue: one record gather per edge for all
// heads, the logit by sweep 1's functions, a batch's results per head through the wave's 64
// staging floats as one coalesced store in CSR order.  st: the piece's row statistics,
// st[h] = shift_of(row_max[h, r]) and st[kMaxH + h] = row_sum[h, r].
template <int KG, int U>
__device__ __forceinline__ void walk_alpha(const float *qrow, float *stage, const float *st,
                                           const int32_t *__restrict__ col_idx,
                                           const uint8_t *__restrict__ rec, int RS,
                                           float *__restrict__ w, int64_t num_e, int H, int DS,
                                           int sb, int se, int k, int trash, int lane) {
    constexpr int G = kWave / KG;
    const int grp = lane / KG, l0 = lane % KG;
    const int n = se - sb;  // wave-uniform, <= chunk
    const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
    const auto rrs = wave_buffer(rec, 0xffffffffu);
    // head h's finished logits of the batch at `base`: the weights staged in edge order, one store
    auto leave = [&](int h, int base, float (&l)[U]) {
        const float shift = st[h], z = st[kMaxH + h];
        const auto ors = wave_buffer(w + (int64_t)h * num_e + sb, (uint32_t)n * 4u);
        wave_lds_fence();
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (l0 == 0) stage[u * G + grp] = expf(l[u] - shift) / z;
        store_staged<KG, U>(stage, ors, base, lane);
    };
    for (int base = 0; base < n; base += G * U) {
        int c[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            c[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(crs, (base + u * G + grp) * 4, 0, 0);
        if (k <= KG) {
            const RecordSlot sl(l0, k);
            const PackedSrc src = sl.src(rrs, k, RS);
            float v[U];
            int s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) src.load(c[u], v[u], s[u]);
            for (int h = 0; h < H; ++h) {
                float l[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    l[u] = lane_tree<KG, Sum>(
                        dot_term(v[u], s[u], qrow + h * DS, trash, sl.ok, 0.f));
                leave(h, base, l);
            }
        } else {
            for (int h = 0; h < H; ++h) {
                float l[U];
                record_dots<KG, U>(rrs, RS, c, qrow + h * DS, k, trash, l0, l);
                leave(h, base, l);
            }
        }
    }
}

template <int KG, int U>
__global__ __launch_bounds__(kBlock) void dath_alpha_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const uint8_t *__restrict__ rec, int RS, const float *__restrict__ q, float scale,
    const float *__restrict__ row_max, const float *__restrict__ row_sum, float *__restrict__ w,
    int num_rows, int64_t num_e, int D, int DS, int k, int chunk, int n_items, int H, int qvec) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int kExtra = kWave + 2 * kMaxH;  // the store staging and the row statistics
    const int wid = threadIdx.x / kWave;
    const int lane = lane_id();
    const int blk = MAXK_FWD_XCD ? xcd_contiguous_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int item = blk * kWavesPerBlock + wid;
    if (item >= n_items) return;  // whole wave; no workgroup barrier below
    float *qrow = lds + (size_t)wid * (H * DS + kExtra);
    float *stage = qrow + H * DS;
    float *st = stage + kWave;
    // the pad columns [D, DS) of every head's row are never staged over: zeroed once
    for (int h = 0; h < H; ++h)
        if (lane < DS - D) qrow[h * DS + D + lane] = 0.f;

    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);
    int r = it.r - 1;
    RowPiece p{0, 0, false};
    if (it.r > 0) p = cont_piece(CutAtEnd{}, it.p_lo, it.d1, it.r, row_ptr[it.r]);
    for (;;) {
        const int64_t sb = p.sb, se = p.se;
        if (r >= 0 && sb < se) {
            wave_lds_fence();  // the previous piece's reads of qrow and st are done
            stage_query(qrow, q, r, num_rows, H, D, DS, scale, qvec != 0, lane);
            if (lane < H) {
                st[lane] = shift_of(row_max[(int64_t)lane * num_rows + r]);
                st[kMaxH + lane] = row_sum[(int64_t)lane * num_rows + r];
            }
            wave_lds_fence();
            walk_alpha<KG, U>(qrow, stage, st, col_idx, rec, RS, w, num_e, H, DS, (int)sb,
                              (int)se, k, DS - 1, lane);
        }
        ++r;
        if (r >= num_rows) break;
        const int64_t rb = row_ptr[r];
        if (!row_owned(it.d1, r, rb)) break;  // row r's token belongs to a later item
        p = row_piece(CutAtEnd{}, it.d1, r, rb, row_ptr[r + 1]);
    }
}

// Waves per SIMD the kernels' VGPRs allow (the kernel-resource-usage remarks).
constexpr int kDotFwdWaves = 4;
constexpr int kDotAlphaWaves = 6;

// The items are sized for the waves a CU holds (walk_chunk): by VGPRs, fewer when the H query
// rows and G accumulator copies per wave fill the CU's LDS first (8 waves at H = 8, k <= 8,
// D = 256).
struct DotLayout {
    int chunk, n_items, hc;
    size_t lds, total;  // lds: per workgroup
    RecordGeom R;
    SlabLayout S;
};

DotLayout dot_fwd_layout(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k, int H,
                         int chunk) {
    DotLayout L{};
    L.R = record_geom(num_cols, D, k);
    L.hc = heads_per_pass(H, L.R.kg);
    L.lds = (size_t)kWavesPerBlock * (H + kWave / L.R.kg) * L.R.DS * sizeof(float);
    L.chunk = walk_chunk(num_rows, num_e, chunk, L.lds, kDotFwdWaves * 4);
    L.n_items = token_items(num_rows, num_e, L.chunk);
    L.S = slab_layout(item_cap(num_rows + num_e, chunk, L.n_items), H, D,
                      al256((size_t)num_cols * L.R.RS), true);
    L.total = L.S.end;
    return L;
}

DotLayout dot_alpha_layout(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k, int H,
                           int chunk) {
    DotLayout L{};
    L.R = record_geom(num_cols, D, k);
    L.lds = (size_t)kWavesPerBlock * (H * L.R.DS + kWave + 2 * kMaxH) * sizeof(float);
    L.chunk = walk_chunk(num_rows, num_e, chunk, L.lds, kDotAlphaWaves * 4);
    L.n_items = token_items(num_rows, num_e, L.chunk);
    L.total = al256((size_t)num_cols * L.R.RS);
    if (L.total == 0) L.total = 256;  // never empty: one query serves any num_cols
    return L;
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" size_t maxk_dot_attention_heads_workspace_size(int64_t num_rows, int64_t num_cols,
                                                          int64_t num_e, int32_t dim_origin,
                                                          int32_t dim_k, int32_t num_heads,
                                                          int32_t chunk_edges) {
    if (!dot_shape_ok(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads, chunk_edges))
        return 0;
    return dot_fwd_layout(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads, chunk_edges)
        .total;
}

namespace {
// The walk and the fix-up of both forward entries, with or without a mask.
template <bool DROP>
int launch_dot_fwd(const int32_t *row_ptr, const int32_t *col_idx, const float *q, float scale,
                   const uint8_t *rec, float *out, float *row_max, float *row_sum, float *slab,
                   float *slab_m, float *slab_z, int32_t *slab_row, int64_t num_rows,
                   int64_t num_e, int D, int k, int H, const DotLayout &L, hipStream_t s,
                   const MaskArg<DROP> &dm) {
    const RecordGeom &R = L.R;
    constexpr int U = MAXK_FWD_U;
    const int flags =
        store_flags(out, H, num_rows, D) | (D % 4 == 0 && ((uintptr_t)q & 15) == 0 ? 4 : 0);
    const bool ok = with_const<8, 16, 32, 64>(R.kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        hipLaunchKernelGGL((dath_fwd_kernel<KG, U, DROP>), item_grid(L.n_items), dim3(kBlock),
                           L.lds, s, row_ptr, col_idx, q, scale, rec, R.RS, out, row_max, row_sum,
                           slab, slab_m, slab_z, slab_row, (int)num_rows, num_e, D, R.DS, k,
                           L.chunk, L.n_items, H, L.hc, flags, dm);
    });
    if (!ok) return bad_lanes(R.kg);
    MAXK_LAUNCHED("dath_fwd_kernel");
    float mul = 1.f;
    if constexpr (DROP) mul = dm.scale;
    return launch_softmax_fixup<DROP>(row_ptr, col_idx, rec, R.RS, k, slab, slab_m, slab_z,
                                      slab_row, out, row_max, row_sum, num_rows, D, L.n_items, H,
                                      mul, s);
}

// Both forward entries; dm: the dropout entry's mask, null for none.
int dot_attention_heads(const int32_t *row_ptr, const int32_t *col_idx, const float *q,
                        float scale, const float *cbsr_val, const uint8_t *cbsr_idx, float *out,
                        float *row_max, float *row_sum, int64_t num_rows, int64_t num_cols,
                        int64_t num_e, int32_t dim_origin, int32_t dim_k, int32_t num_heads,
                        int32_t chunk_edges, void *workspace, size_t workspace_bytes,
                        void *stream, const DropMask *dm) {
    if (int rc = check_dot(num_rows, num_cols, num_e, scale, dim_origin, dim_k, num_heads,
                           chunk_edges))
        return rc;
    if (num_rows == 0) return MAXK_OK;
    MAXK_REQUIRE(row_ptr && out && row_max && row_sum,
                 "row_ptr / out / row_max / row_sum must not be NULL");
    const int D = dim_origin, k = dim_k, H = num_heads;
    hipStream_t s = as_stream(stream);
    if (num_e == 0) return zero_heads_out(out, row_max, row_sum, H, num_rows, D, s);
    MAXK_REQUIRE(col_idx && q && cbsr_val && cbsr_idx,
                 "col_idx / q / cbsr_val / cbsr_idx must not be NULL");
    MAXK_REQUIRE(num_cols > 0, "edges present but num_cols == 0");
    const DotLayout L = dot_fwd_layout(num_rows, num_cols, num_e, D, k, H, chunk_edges);
    const RecordGeom &R = L.R;
    MAXK_REQUIRE(!R.wide, "num_cols: the fused dot-product attention takes tables below 2^24 "
                 "columns and 4 GiB of records (%lld columns of %d bytes)", (long long)num_cols,
                 R.RS);
    if (int rc = check_workspace(workspace, workspace_bytes, L.total)) return rc;
    MAXK_REQUIRE(((uintptr_t)cbsr_val & 3) == 0 && ((uintptr_t)q & 3) == 0 &&
                     ((uintptr_t)out & 3) == 0 && ((uintptr_t)row_max & 3) == 0 &&
                     ((uintptr_t)row_sum & 3) == 0,
                 "float buffers must be 4-B aligned");
    char *ws = reinterpret_cast<char *>(workspace);
    uint8_t *rec = reinterpret_cast<uint8_t *>(ws);
    float *slab = reinterpret_cast<float *>(ws + L.S.slab_off);
    float *slab_m = reinterpret_cast<float *>(ws + L.S.m_off);
    float *slab_z = reinterpret_cast<float *>(ws + L.S.z_off);
    int32_t *slab_row = reinterpret_cast<int32_t *>(ws + L.S.row_off);
    if (int rc = launch_cbsr_pack(cbsr_val, cbsr_idx, rec, num_cols, k, R.RS, D, R.DS - 1, s))
        return rc;
    if (dm)
        return launch_dot_fwd<true>(row_ptr, col_idx, q, scale, rec, out, row_max, row_sum, slab,
                                    slab_m, slab_z, slab_row, num_rows, num_e, D, k, H, L, s, *dm);
    return launch_dot_fwd<false>(row_ptr, col_idx, q, scale, rec, out, row_max, row_sum, slab,
                                 slab_m, slab_z, slab_row, num_rows, num_e, D, k, H, L, s,
                                 NoMask{});
}
}  // namespace

extern "C" int maxk_dot_attention_heads(const int32_t *row_ptr, const int32_t *col_idx,
                                        const float *q, float scale, const float *cbsr_val,
                                        const uint8_t *cbsr_idx, float *out, float *row_max,
                                        float *row_sum, int64_t num_rows, int64_t num_cols,
                                        int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                        int32_t num_heads, int32_t chunk_edges, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    clear_error();
    return dot_attention_heads(row_ptr, col_idx, q, scale, cbsr_val, cbsr_idx, out, row_max,
                               row_sum, num_rows, num_cols, num_e, dim_origin, dim_k, num_heads,
                               chunk_edges, workspace, workspace_bytes, stream, nullptr);
}

extern "C" size_t maxk_dot_attention_heads_dropout_workspace_size(
    int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
    int32_t num_heads, int32_t chunk_edges) {
    return maxk_dot_attention_heads_workspace_size(num_rows, num_cols, num_e, dim_origin, dim_k,
                                                   num_heads, chunk_edges);
}

extern "C" int maxk_dot_attention_heads_dropout(
    const int32_t *row_ptr, const int32_t *col_idx, const float *q, float scale,
    const float *cbsr_val, const uint8_t *cbsr_idx, float *out, float *row_max, float *row_sum,
    int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
    int32_t num_heads, int32_t chunk_edges, float p, uint64_t seed, void *workspace,
    size_t workspace_bytes, void *stream) {
    clear_error();
    return with_dropout(p, seed, [&](const DropMask *dm) {
        return dot_attention_heads(row_ptr, col_idx, q, scale, cbsr_val, cbsr_idx, out, row_max,
                                   row_sum, num_rows, num_cols, num_e, dim_origin, dim_k,
                                   num_heads, chunk_edges, workspace, workspace_bytes, stream, dm);
    });
}

extern "C" size_t maxk_dot_edge_alpha_heads_workspace_size(int64_t num_rows, int64_t num_cols,
                                                           int64_t num_e, int32_t dim_origin,
                                                           int32_t dim_k, int32_t num_heads,
                                                           int32_t chunk_edges) {
    if (!dot_shape_ok(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads, chunk_edges))
        return 0;
    return dot_alpha_layout(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads, chunk_edges)
        .total;
}

extern "C" int maxk_dot_edge_alpha_heads(const int32_t *row_ptr, const int32_t *col_idx,
                                         const float *q, float scale, const float *cbsr_val,
                                         const uint8_t *cbsr_idx, const float *row_max,
                                         const float *row_sum, float *w, int64_t num_rows,
                                         int64_t num_cols, int64_t num_e, int32_t dim_origin,
                                         int32_t dim_k, int32_t num_heads, int32_t chunk_edges,
                                         void *workspace, size_t workspace_bytes, void *stream) {
    clear_error();
    if (int rc = check_dot(num_rows, num_cols, num_e, scale, dim_origin, dim_k, num_heads,
                           chunk_edges))
        return rc;
    if (num_e == 0) return MAXK_OK;  // no edge, nothing to write
    MAXK_REQUIRE(num_rows > 0 && num_cols > 0, "edges present but num_rows or num_cols == 0");
    MAXK_REQUIRE(row_ptr && col_idx && q && cbsr_val && cbsr_idx && row_max && row_sum && w,
                 "row_ptr / col_idx / q / cbsr_val / cbsr_idx / row_max / row_sum / w must not "
                 "be NULL");
    const int D = dim_origin, k = dim_k, H = num_heads;
    const DotLayout L = dot_alpha_layout(num_rows, num_cols, num_e, D, k, H, chunk_edges);
    const RecordGeom &R = L.R;
    MAXK_REQUIRE(!R.wide, "num_cols: the dot-product alpha takes tables below 2^24 columns and "
                 "4 GiB of records (%lld columns of %d bytes)", (long long)num_cols, R.RS);
    if (int rc = check_workspace(workspace, workspace_bytes, L.total)) return rc;
    MAXK_REQUIRE(((uintptr_t)cbsr_val & 3) == 0 && ((uintptr_t)q & 3) == 0 &&
                     ((uintptr_t)row_max & 3) == 0 && ((uintptr_t)row_sum & 3) == 0 &&
                     ((uintptr_t)w & 3) == 0,
                 "float buffers must be 4-B aligned");
    hipStream_t s = as_stream(stream);
    uint8_t *rec = reinterpret_cast<uint8_t *>(workspace);
    if (int rc = launch_cbsr_pack(cbsr_val, cbsr_idx, rec, num_cols, k, R.RS, D, R.DS - 1, s))
        return rc;
    constexpr int U = MAXK_FWD_U;
    const int qvec = D % 4 == 0 && ((uintptr_t)q & 15) == 0;
    const bool ok = with_const<8, 16, 32, 64>(R.kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        hipLaunchKernelGGL((dath_alpha_kernel<KG, U>), item_grid(L.n_items), dim3(kBlock), L.lds,
                           s, row_ptr, col_idx, rec, R.RS, q, scale, row_max, row_sum, w,
                           (int)num_rows, num_e, D, R.DS, k, L.chunk, L.n_items, H, qvec);
    });
    if (!ok) return bad_lanes(R.kg);
    MAXK_LAUNCHED("dath_alpha_kernel");
    return MAXK_OK;
}
