// The hub-row heads walk, stated once for the three multi-head forwards that run it:
// spgemm_fwd_heads.hip (weights from edge_val), gat_attention_heads.hip (the GAT softmax of
// interleaved scores) and dot_attention_heads.hip (the softmax of dot-product logits).  Each of
// them computes its own weights; everything around the weights is here.  The grad_q aggregation
// of dot_attention_heads_bwd.hip runs it too, with the edge-major gl [E, HP] as the weights.
//
// One wavefront per item of the token stream (token_items.h) under the hub-row cut rule
// (CutHubRows).  With KG = pow2ceil(k) lanes per group (>= 8, <= 64) a wave has G = 64 / KG lane
// groups and G LDS copies of the output row, DS floats each (D padded to 16 B plus one 16-B group
// whose last float is the trash column).  The H heads are walked in passes of HC heads
// (heads_per_pass); in a pass group g works on (edge g / HC, head g % HC): EP = G / HC edges per
// wave step, the HC groups of an edge issue the same record addresses in one load instruction
// (one line fetched, not HC).
// The rules every walk keeps:
//  * copy g belongs to head g % HC.  Within a step the lanes of a group hit distinct columns (the
//    pack folds repeated selectors) and different groups hit different copies, so accumulation is
//    plain ds_read / fma / ds_write: no LDS atomics, no global atomics.  A lane without an
//    addend -- a group past EP * HC (G % HC != 0), a slot l >= k, an edge past the piece's end, a
//    folded or out-of-range selector -- writes its copy's trash column only (scatter_records);
//  * the copies are zero when a pass starts: the prologue zeroes them once and flush_head zeroes
//    what it reads.  After a pass head hh is the sum of copies hh, HC + hh, ... in that order,
//    divided once (flush_head);
//  * a row whose tokens all lie in the item goes to out; only a hub row (longer than an item)
//    is cut, its owner's piece going to out and each continuation to the item's slab
//    [H, n_items, D].  slab_row[item] names the row an item holds a continuation of, -1 for none,
//    and is written by that item's wave alone (walk_hub_item).  Every row of every head is
//    stored, an edgeless row as zeros: out needs no initialising;
//  * softmax rows (bad_heads, softmax_fixup_kernel): a row inside one item is stored as
//    acc / z with its (m, z); a hub row's pieces are stored unnormalised with their own (m, z)
//    and merged in item order: m = max m_i, each piece scaled by exp(m_i - m), one division by
//    z = sum z_i exp(m_i - m).  A row whose z is not a positive number (a NaN or +Inf logit: z is
//    NaN; only -Inf logits: z = 0) is NaN wherever it has an addend, as the IEEE evaluation of
//    alpha * value gives, and exactly 0 elsewhere: dividing by such a z would turn the columns
//    without addends into NaN too, so the row is walked once more with the weight NaN and stored
//    undivided.  A row without edges stores zeros in out and both statistics.
// Every sum has an order fixed by (graph, chunk, k, H): the results are bitwise repeatable.
// Device code in an anonymous namespace (each translation unit instantiates what it launches,
// as slab_fixup_kernel in common.h), host code plain inline.
#pragma once

#include <cmath>

#include "cbsr_pack.h"
#include "common.h"

namespace maxk {
namespace {

// ---- device: the wave's place in a pass -------------------------------------------------------

template <int KG>
struct PassGeom {
    static constexpr int G = kWave / KG;  // lane groups = LDS copies per wave
    int grp;       // this lane's group
    float *acc_g;  // its copy of the output row: copy grp of the wave's G copies at acc
    int EP;        // edges per wave step (HC <= G)
    int eg, hh;    // the group's edge slot and head of the pass
    bool grp_ok;   // the group has both
    __device__ __forceinline__ PassGeom(int lane, int HC, float *acc, int DS)
        : grp(lane / KG), acc_g(acc + grp * DS), EP(G / HC), eg(grp / HC), hh(grp % HC),
          grp_ok(grp < EP * HC) {}
};

// p[0:n] = 0 (n a multiple of 4, p 16-B aligned).  One wave.
__device__ __forceinline__ void zero_wave_lds(float *p, int n, int lane) {
    for (int j = lane * 4; j < n; j += kWave * 4)
        *reinterpret_cast<float4 *>(&p[j]) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// One wave step's products: slot u of the step is the piece's edge base + u * EP + eg, of column
// c[u] and weight w[u], and this lane's group adds w[u] * value into acc_g[selector] over the
// record's slots l0, l0 + KG, ... (one pass unless k > 64), one rounding each.  A slot past the
// piece's n edges, a group that is not active (no edge slot or no head in this pass) and a lane
// l >= k have no addend: the trash column takes theirs.
template <int KG, int U>
__device__ __forceinline__ void scatter_records(float *acc_g, const __amdgpu_buffer_rsrc_t rrs,
                                                int RS, int k, int trash, int l0,
                                                const int (&c)[U], const float (&w)[U],
                                                bool active, int base, int EP, int eg, int n) {
    for (int lb = 0; lb < k; lb += KG) {
        const RecordSlot sl(lb + l0, k);
        const PackedSrc src = sl.src(rrs, k, RS);
        float v[U];
        int s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) src.load(c[u], v[u], s[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool live = sl.ok && active && base + u * EP + eg < n;
            float *a = &acc_g[live ? min(s[u], trash) : trash];
            *a = __builtin_fmaf(w[u], v[u], *a);
        }
    }
}

// dst[0:D] = (acc[0:D] + acc[stride + 0:D] + ... over nc copies) / div; the copies read are
// zeroed.  One wave.  MUL: the quotient times mul (the dropout mask's scale).
template <bool MUL>
__device__ __forceinline__ void flush_head(float *acc, int nc, int stride, float *__restrict__ dst,
                                           int D, float div, bool scale, bool vec, bool nt,
                                           int lane, float mul) {
    if (vec) {
        for (int j = lane * 4; j < D; j += kWave * 4) {
            float4 a = *reinterpret_cast<float4 *>(&acc[j]);
            *reinterpret_cast<float4 *>(&acc[j]) = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int g = 1; g < nc; ++g) {
                float4 *pg = reinterpret_cast<float4 *>(&acc[g * stride + j]);
                const float4 b = *pg;
                a.x += b.x;
                a.y += b.y;
                a.z += b.z;
                a.w += b.w;
                *pg = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            if (scale) {
                a.x = a.x / div;
                a.y = a.y / div;
                a.z = a.z / div;
                a.w = a.w / div;
                if constexpr (MUL) {
                    a.x *= mul;
                    a.y *= mul;
                    a.z *= mul;
                    a.w *= mul;
                }
            }
            if (nt)  // output rows streamed past the caches (the record lines stay)
                __builtin_nontemporal_store(__builtin_bit_cast(f32x4, a),
                                            reinterpret_cast<f32x4 *>(&dst[j]));
            else
                *reinterpret_cast<float4 *>(&dst[j]) = a;
        }
    } else {
        for (int j = lane; j < D; j += kWave) {
            float a = acc[j];
            acc[j] = 0.f;
            for (int g = 1; g < nc; ++g) {
                a += acc[g * stride + j];
                acc[g * stride + j] = 0.f;
            }
            if (scale) a = MUL ? a / div * mul : a / div;
            dst[j] = a;
        }
    }
}

// The end of a softmax pass over the heads h0 .. h0 + HC of a piece of n edges.  ps is the
// lane's sum of p from the walk (the same in every lane of a group); z of head h0 + j is its EP
// groups' sums added in group order.
template <int KG>
__device__ __forceinline__ float pass_z(float ps, int j, int EP, int HC) {
    float z = 0.f;
    for (int e = 0; e < EP; ++e) z += __shfl(ps, (e * HC + j) * KG);
    return uniform(z);
}
// Bit j: z of head h0 + j is no positive number.  Where the piece is a whole row (and has
// edges), the caller walks those heads once more with the weight NaN, behind a wave_lds_fence,
// and flushes them undivided.
template <int KG>
__device__ __forceinline__ int bad_heads(float ps, int EP, int HC, int h0, int H) {
    int bad = 0;
    for (int j = 0; j < HC && h0 + j < H; ++j)
        if (!(pass_z<KG>(ps, j, EP, HC) > 0.f)) bad |= 1 << j;
    return bad;
}

// The item driver: piece(row, sb, se, whole, owned) for the edges [sb, se) of every row the item
// walks.  First the continuation of row r - 1 (its token precedes the item): only a hub row
// leaves one (owned = false: it goes to the item's slab), and slab_row[item] names it for the
// fix-up.  Then the rows whose token lies in the item (owned = true: they go to out), whole
// unless the row is a hub row cut at the item's end.
template <class Piece>
__device__ __forceinline__ void walk_hub_item(const int32_t *__restrict__ row_ptr,
                                              int32_t *__restrict__ slab_row, int num_rows,
                                              int64_t num_e, int item, int chunk, int lane,
                                              Piece &&piece) {
    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);
    int r = it.r;
    int cont = -1;
    if (r > 0) {
        const RowPiece p =
            cont_piece(CutHubRows{}, it.p_lo, it.d1, r, row_ptr[r - 1], row_ptr[r], chunk);
        if (p.sb < p.se && p.hub) {
            piece(r - 1, p.sb, p.se, false, false);
            cont = r - 1;
        }
    }
    if (lane == 0) slab_row[item] = cont;
    while (r < num_rows) {
        const int64_t rb = row_ptr[r];
        if (!row_owned(it.d1, r, rb)) break;
        const RowPiece p = row_piece(CutHubRows{}, it.d1, r, rb, row_ptr[r + 1], chunk);
        piece(r, rb, p.se, !p.hub, true);
        ++r;
    }
}

// The merge of a hub row's softmax pieces, one head per blockIdx.y, 16 lanes per item as
// slab_fixup_kernel: the thread group of the first item holding a slab of the row merges the
// owner's piece (in out and the statistics) and the row's slabs in item order.  Every hub row
// has a slab: it is longer than an item.  MUL: the merged quotient times mul.
template <bool MUL>
__global__ __launch_bounds__(kBlock) void softmax_fixup_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const uint8_t *__restrict__ rec, int RS, int k, const float *__restrict__ slab_all,
    const float *__restrict__ slab_m_all, const float *__restrict__ slab_z_all,
    const int32_t *__restrict__ slab_row, float *__restrict__ out_all,
    float *__restrict__ row_max_all, float *__restrict__ row_sum_all, int64_t num_rows, int D,
    int n_items, float mul) {
    const int item = (int)((blockIdx.x * (int64_t)kBlock + threadIdx.x) / 16);
    const int g = threadIdx.x % 16;
    if (item >= n_items) return;
    const int row = slab_row[item];
    if (row < 0 || (item > 0 && slab_row[item - 1] == row)) return;
    const int64_t h = blockIdx.y;
    const float *sm = slab_m_all + h * n_items + item;
    const float *sz = slab_z_all + h * n_items + item;
    const float *sl = slab_all + (h * n_items + item) * D;
    float *o = out_all + (h * num_rows + row) * D;
    float *rm = row_max_all + h * num_rows + row;
    float *rs = row_sum_all + h * num_rows + row;
    int n = 1;
    while (item + n < n_items && slab_row[item + n] == row) ++n;
    const float m0 = *rm, z0 = *rs;
    float m = m0;
    for (int i = 0; i < n; ++i) m = fmaxf(m, sm[i]);
    // a piece of nothing but -inf has sum 0 (or NaN) and scale exp(-inf) = 0
    const float shift = m == -INFINITY ? 0.f : m;
    const float c0 = expf(m0 - shift);
    float z = z0 * c0;
    for (int i = 0; i < n; ++i) z += sz[i] * expf(sm[i] - shift);
    if (z > 0.f) {
        for (int j = g; j < D; j += 16) {
            float a = o[j] * c0;
            for (int i = 0; i < n; ++i) a += sl[(int64_t)i * D + j] * expf(sm[i] - shift);
            o[j] = MUL ? a / z * mul : a / z;
        }
    } else {  // rare: NaN wherever the row has an addend, 0 elsewhere
        for (int j = g; j < D; j += 16) o[j] = 0.f;
        __threadfence();  // the zeros land before the NaNs of other lanes (one wave, in order)
        const int64_t rb = row_ptr[row], re = row_ptr[row + 1];
        for (int64_t e = rb; e < re; ++e) {
            const uint8_t *p = rec + (int64_t)col_idx[e] * RS + 4 * k;
            for (int l = g; l < k; l += 16) {
                const int s = reinterpret_cast<const uint16_t *>(p)[l];
                if (s < D) o[s] = NAN;  // a folded or out-of-range selector is >= 0x100
            }
        }
    }
    if (g == 0) {
        *rm = m;
        *rs = z;
    }
}

}  // namespace

// ---- host ---------------------------------------------------------------------------------------

// The records and lane groups of a walk that gathers one packed record per edge.  wide: the
// table is past what 24-bit column multiplies and 32-bit record offsets address.
struct RecordGeom {
    int RS, DS, kg;
    bool wide;
};
inline RecordGeom record_geom(int64_t num_cols, int D, int k) {
    RecordGeom R{};
    R.RS = record_stride(k, num_cols);
    R.DS = copy_stride(D);
    const int g = lanes_per_edge(k);
    R.kg = g < 8 ? 8 : g;
    R.wide = !(num_cols < (1 << 24) && (uint64_t)num_cols * (uint64_t)R.RS < (1ull << 32));
    return R;
}

// Heads per pass: NP = ceil(H / G) passes of HC = ceil(H / NP) heads (one pass whenever H <= G;
// H = 8 at k = 16, G = 4: two passes of four heads).
inline int heads_per_pass(int H, int kg) {
    const int G = kWave / kg;
    const int np = (H + G - 1) / G;
    return (H + np - 1) / np;
}

// The item size of a walk whose workgroups take lds_per_block bytes: sized for the waves a CU
// holds, by_regs by VGPRs, fewer when the LDS fills the CU first; at most cap tokens.
inline int walk_chunk(int64_t num_rows, int64_t num_e, int chunk, size_t lds_per_block,
                      int by_regs, int cap = kMaxChunk) {
    const int by_lds = (int)(kPullLdsBytes / lds_per_block) * kWavesPerBlock;
    const int c = fwd_chunk(num_rows, num_e, chunk, by_lds < by_regs ? by_lds : by_regs);
    return c > cap ? cap : c;
}

// The per-item parts of a workspace from `base` on, for `cap` items: the slabs [H, cap, D], with
// `stats` the slab statistics m and z [H, cap], and slab_row [cap].
struct SlabLayout {
    size_t slab_off, m_off, z_off, row_off, end;
};
inline SlabLayout slab_layout(int64_t cap, int H, int D, size_t base, bool stats) {
    const size_t stat = stats ? al256((size_t)cap * H * sizeof(float)) : 0;
    SlabLayout S{};
    S.slab_off = base;
    S.m_off = S.slab_off + al256((size_t)cap * H * D * sizeof(float));
    S.z_off = S.m_off + stat;
    S.row_off = S.z_off + stat;
    S.end = S.row_off + al256((size_t)cap * sizeof(int32_t));
    return S;
}

// The kernels' store flags: bit 0 16-B row stores (D % 4 == 0, out 16-B aligned), bit 1
// non-temporal out rows -- rows past the Infinity Cache's size are streamed, as the single-head
// forward stores them (MAXK_FWD_OUT_NT).
inline int store_flags(const float *out, int H, int64_t num_rows, int D) {
    const bool big = (double)H * num_rows * D * 4 > (double)kInfinityCacheBytes;
    return (D % 4 == 0 && ((uintptr_t)out & 15) == 0 ? 1 : 0) |
           ((MAXK_FWD_OUT_NT == 1 || (MAXK_FWD_OUT_NT == 2 && big)) ? 2 : 0);
}

inline int check_cbsr_dims(int32_t dim_origin, int32_t dim_k, int64_t num_cols) {
    MAXK_REQUIRE(dim_origin >= 1 && dim_origin <= kMaxDim, "dim_origin must be in [1,256], got %d",
                 dim_origin);
    MAXK_REQUIRE(dim_k >= 1 && dim_k <= dim_origin, "dim_k must be in [1,dim_origin], got %d",
                 dim_k);
    MAXK_REQUIRE(num_cols * (int64_t)dim_k < (1LL << 31), "num_cols*k too large");
    return MAXK_OK;
}

// num_e == 0, nothing to walk: zero rows, and zero statistics where the entry has them.
inline int zero_heads_out(float *out, float *row_max, float *row_sum, int H, int64_t num_rows,
                          int D, hipStream_t s) {
    if (int rc = zero_words(out, (int64_t)H * num_rows * D, s)) return rc;
    if (!row_max) return MAXK_OK;
    if (int rc = zero_words(row_max, (int64_t)H * num_rows, s)) return rc;
    return zero_words(row_sum, (int64_t)H * num_rows, s);
}

template <bool MUL>
inline int launch_softmax_fixup(const int32_t *row_ptr, const int32_t *col_idx, const uint8_t *rec,
                                int RS, int k, const float *slab, const float *slab_m,
                                const float *slab_z, const int32_t *slab_row, float *out,
                                float *row_max, float *row_sum, int64_t num_rows, int D,
                                int n_items, int H, float mul, hipStream_t s) {
    hipLaunchKernelGGL(softmax_fixup_kernel<MUL>,
                       dim3((unsigned)ceil_div(n_items, kBlock / 16), (unsigned)H), dim3(kBlock),
                       0, s, row_ptr, col_idx, rec, RS, k, slab, slab_m, slab_z, slab_row, out,
                       row_max, row_sum, num_rows, D, n_items, mul);
    MAXK_LAUNCHED("softmax_fixup_kernel");
    return MAXK_OK;
}

}  // namespace maxk
