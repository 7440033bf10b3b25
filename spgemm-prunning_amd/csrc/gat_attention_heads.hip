// Fused multi-head GAT attention for gfx950: the edge softmax inside the aggregation walk,
//
//   out[h, r, cbsr_idx[c, l]] += alpha[h, e] * cbsr_val[c, l]       e in row r, c = col_idx[e]
//   alpha[h, e] = exp(l_he - m_hr) / z_hr          l_he = leaky_relu(s_dst[h, r] + s_src[h, c])
//   m_hr = max_e l_he                              z_hr = sum_e exp(l_he - m_hr)
//
// what maxk_gat_edge_softmax_heads followed by maxk_spgemm_forward_heads compute, without alpha
// [H, E] ever existing: not in an output, not in the workspace.  The row statistics
// row_max = m and row_sum = z are outputs, and maxk_gat_edge_alpha_heads rebuilds alpha from
// them for the backward.  The pieces are those of spgemm_fwd_heads.hip (records packed once,
// token-stream items, one wavefront per item under CutHubRows, KG lanes per group, G = 64 / KG
// LDS copies of the output row, the heads in passes of HC) and of edge_softmax_heads.hip (the
// scores interleaved to ss_t [num_cols, HP], one aligned vector per column):
//
//  1. launch_cbsr_pack and gath_interleave_kernel fill the workspace's records and ss_t.
//  2. gath_fwd_kernel, per row piece:
//     * sweep 1, one lane per edge: the ss_t vector of col_idx[e], the logits of every head,
//       the piece's maximum per head by a fixed butterfly;
//     * sweep 2, per pass of HC heads, group g on (edge g / HC, head g % HC): per wave step of
//       G * U (slot, group) pairs each p = exp(l - m_piece) is computed once, by lane
//       slot * G + group (the head's score is one 4-B load inside the sector sweep 1 fetched),
//       and fetched by its group with a shuffle; then the record gather shared by the HC
//       groups of the edge, acc += p * value in the group's LDS copy and the lane's own sum
//       of p.  The maximum is known before the first product, so nothing in LDS is ever
//       rescaled;
//     * z_piece of a head: the sums of its EP groups added in group order.  A row inside one
//       item (every row of at most `chunk` edges) is stored as acc / z with its (m, z); a hub
//       row's pieces are stored unnormalised, the owner's into out and the statistics, a
//       continuation's into the item's slab [H, n_items, D] and slab statistics [H, n_items].
//  3. gath_fixup_kernel merges a hub row's pieces in item order: m = max m_i, each piece scaled
//     by exp(m_i - m), one division by z = sum z_i exp(m_i - m).
// A row whose z is not a positive number (a NaN or +Inf logit: z is NaN; only -Inf logits:
// z = 0) is all NaN wherever it has an addend, as the IEEE evaluation of alpha * value gives,
// and exactly 0 elsewhere: dividing by such a z would turn the columns without addends into
// NaN too, so those rows are walked once more with the weight NaN and stored undivided.  A row
// without edges stores zeros in out and both statistics.
// No global atomics, no LDS atomics; every sum has an order fixed by (graph, chunk, k, H), so
// the result is bitwise repeatable, and head h's slice is computed from head h's scores only.
// LDS per wave as the multi-head forward (G * DS floats); 87 to 96 VGPRs at HP = 2 and 4 (five
// waves per SIMD), 108 or 109 at HP = 8 (four); no scratch.
// maxk_gat_attention_heads_dropout is the same walk with the attention-dropout mask of
// attn_dropout.h multiplied in (the DROP instantiations): out sums alpha * d * value, the
// statistics stay those of the undropped softmax, p == 0 launches the kernels without a mask.
#include <cmath>

#include "attn_dropout.h"
#include "cbsr_pack.h"
#include "edge_softmax.h"

namespace maxk {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float uniform(float x) {
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x)));
}

template <int HP>
__global__ __launch_bounds__(kBlock) void gath_interleave_kernel(
    const float *__restrict__ s_src, VecF<HP> *__restrict__ ss_t, int H, int64_t num_cols) {
    const int64_t c = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (c >= num_cols) return;
    VecF<HP> x;
#pragma unroll
    for (int h = 0; h < HP; ++h) x.v[h] = h < H ? s_src[h * num_cols + c] : 0.f;
    ss_t[c] = x;
}

// Sweep 1 over the edges [sb, sb + n) (n >= 1): m[h] = the piece's largest logit of head h
// (-inf for a pad head), wave-uniform.
template <int HP>
__device__ __forceinline__ void piece_max(const VecF<HP> *__restrict__ ss_t,
                                          const int32_t *__restrict__ col, int n, int H,
                                          const float (&sd)[HP], float slope, int lane,
                                          float (&m)[HP]) {
    constexpr int MU = HP == 8 ? 2 : kU;  // vector gathers in flight: 16 registers of scores
    for (int base = 0; base < n; base += kWave * MU) {
        VecF<HP> x[MU];
#pragma unroll
        for (int u = 0; u < MU; ++u) {
            const int i = base + u * kWave + lane;
            if (i < n) x[u] = ss_t[(uint32_t)col[i]];
        }
#pragma unroll
        for (int h = 0; h < HP; ++h) {
            if (h < H) {
#pragma unroll
                for (int u = 0; u < MU; ++u) {
                    const int i = base + u * kWave + lane;
                    const float l = i < n ? leaky(sd[h] + x[u].v[h], slope) : -INFINITY;
                    m[h] = fmaxf(m[h], l);
                }
            }
        }
    }
#pragma unroll
    for (int h = 0; h < HP; ++h)
        if (h < H) m[h] = uniform(lane_tree<kWave, Max>(m[h]));
}

// Which (edge slot, head) of a wave step lane t computes the weight of: the step's G * U
// (unroll slot u, group) pairs are laid over the lanes t = u * G + group, so every weight of a
// step is computed once, by one lane, and the lanes of its group fetch it with one shuffle.
struct WeightLane {
    int u, eg, head;  // unroll slot, edge slot of the group, the group's head (0 when !on)
    bool on;          // the group has an edge slot and a head in this pass
    float sdh, shift;
};

// Sweep 2 of one pass over the edges [sb, se) (sb < se): this lane's group adds p * value into
// its copy acc_g for the edges base + u * EP + eg it is given, p = exp(l - shift) from its
// head's score ss[c * HP + head]; returns the lane's sum of p (the same in every lane of a
// group).  active: the group has an edge slot and a head in this pass; else it writes its trash
// column only.  POISON: p = NaN and nothing is summed (the rows whose z is no positive number).
// DROP (attn_dropout.h): a wave step holds EP * U edges and the pass's heads lie in dp.qp <= 2
// quads, so one Philox evaluation per lane -- lane t on the edge at offset t % span of the next
// S = 64 / (EP * U * qp) steps (span = S * EP * U; its CSR position is sb + its index in the
// piece) and the quad dp.q0 + t / span -- serves S steps: four ballots, one per head of a quad,
// carry the bits, and each group keeps its head's 64 (`mine`).  The sum of p takes the unmasked
// weights and the products p * (0 or 1): a dropped NaN or Inf stays NaN.
struct DropPass {
    int q0, qp, head;  // the pass's first quad of heads and their number; the group's head
};
template <int KG, int HP, int U, bool POISON, bool DROP>
__device__ __forceinline__ float walk_attn(float *acc_g, const int32_t *__restrict__ col_idx,
                                           const float *__restrict__ ss, const WeightLane &wl,
                                           float slope, const uint8_t *__restrict__ rec, int RS,
                                           int sb, int se, int k, int trash, int EP, int eg,
                                           bool active, int lane, const MaskArg<DROP> &dm,
                                           const DropPass &dp) {
    constexpr int G = kWave / KG;
    const int l0 = lane % KG, grp = lane / KG;
    const int n = se - sb;  // wave-uniform, <= 2 * chunk
    const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
    const auto rrs = wave_buffer(rec, 0xffffffffu);  // offsets < num_cols * RS < 2^32
    float ps = 0.f;
    const int EU = EP * U;
    int S = 1, span_log = 0, js = 0, qsel = 0;
    uint64_t mine = 0;
    if constexpr (DROP) {
        S = kWave / (EU * dp.qp);  // powers of two, EU * qp <= 64
        span_log = 31 - __clz(S * EU);
        qsel = min(max((dp.head >> 2) - dp.q0, 0), dp.qp - 1);
    }
    for (int base = 0; base < n; base += EP * U) {
        int c[U];
        float w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = base + u * EP + eg;
            // past the piece's end the column reads 0 (column 0's record and scores)
            c[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(crs, i * 4, 0, 0);
        }
        if constexpr (POISON) {
#pragma unroll
            for (int u = 0; u < U; ++u) w[u] = active && base + u * EP + eg < n ? NAN : 0.f;
        } else {
            // this lane's own weight of the step, then the group's U weights by shuffle
            const int it = base + wl.u * EP + wl.eg;
            const int ct = (int)__builtin_amdgcn_raw_buffer_load_b32(crs, it * 4, 0, 0);
            const float x = ss[(uint32_t)ct * (uint32_t)HP + (uint32_t)wl.head];
            const float pt = wl.on && it < n ? expf(leaky(wl.sdh + x, slope) - wl.shift) : 0.f;
            if constexpr (DROP) {
                if (js == 0) {  // wave-uniform: the masks of this and the next S - 1 steps
                    const uint32_t bits =
                        drop_bits(dm, (uint32_t)(sb + base + (lane & ((1 << span_log) - 1))),
                                  (uint32_t)(dp.q0 + (lane >> span_log)));
                    const uint64_t b0 = __ballot(bits & 1u), b1 = __ballot(bits & 2u),
                                   b2 = __ballot(bits & 4u), b3 = __ballot(bits & 8u);
                    const int hb = dp.head & 3;
                    mine = (hb == 0 ? b0 : hb == 1 ? b1 : hb == 2 ? b2 : b3) >> (qsel << span_log);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                w[u] = __shfl(pt, u * G + grp);
                ps += w[u];
                if constexpr (DROP) w[u] *= (mine >> (js * EU + u * EP + eg)) & 1 ? 0.f : 1.f;
            }
            if constexpr (DROP) js = js + 1 == S ? 0 : js + 1;
        }
        for (int lb = 0; lb < k; lb += KG) {  // one pass unless k > 64
            const int l = lb + l0;
            const bool lok = l < k;
            const uint32_t lc = (uint32_t)(lok ? l : k - 1);
            const PackedSrc src{rrs, 4u * lc, 4u * (uint32_t)k + 2u * lc, (uint32_t)RS};
            float v[U];
            int s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) src.load(c[u], v[u], s[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool live = lok && active && base + u * EP + eg < n;
                float *a = &acc_g[live ? min(s[u], trash) : trash];
                *a = __builtin_fmaf(w[u], v[u], *a);
            }
        }
    }
    return ps;
}

// dst[0:D] = (acc[0:D] + acc[stride + 0:D] + ... over nc copies) / div; the copies read are
// zeroed.  One wave.  DROP: the quotient times mul, the mask's scale.
template <bool DROP>
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
                if constexpr (DROP) {
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
            if (scale) a = DROP ? a / div * mul : a / div;
            dst[j] = a;
        }
    }
}

// Five waves per SIMD where the registers allow it without scratch (HP = 2, 4: at most 96
// VGPRs); HP = 8 takes 108 or 109 and runs four.  DROP keeps the same waves: at HP = 2 and 4 the
// Philox rounds then spill 12 to 60 bytes per lane around the once-in-S-steps evaluation, which
// measured faster than four waves without scratch (the forward's cost of the mask 1.09 to 1.13
// against 1.23 to 1.30 Reddit-sized; profiles/r17/attn_dropout/); HP = 8 takes 124 or 125.
template <int KG, int HP, int U, bool DROP>
__global__ __launch_bounds__(kBlock, HP == 8 ? 4 : 5) void gath_fwd_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const VecF<HP> *__restrict__ ss_t, const float *__restrict__ s_dst, float slope,
    const uint8_t *__restrict__ rec, int RS, float *__restrict__ out,
    float *__restrict__ row_max, float *__restrict__ row_sum, float *__restrict__ slab,
    float *__restrict__ slab_m, float *__restrict__ slab_z, int32_t *__restrict__ slab_row,
    int num_rows, int64_t num_e, int D, int DS, int k, int chunk, int n_items, int H, int HC,
    int flags, MaskArg<DROP> dm) {
    // flags: bit 0 16-B row stores (D % 4 == 0, out 16-B aligned), bit 1 non-temporal out rows
    constexpr int G = kWave / KG;  // lane groups = LDS copies per wave
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wid = threadIdx.x / kWave;
    const int lane = lane_id();
    const int blk = MAXK_FWD_XCD ? xcd_contiguous_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int item = blk * kWavesPerBlock + wid;
    if (item >= n_items) return;  // whole wave; no workgroup barrier below
    float *acc = lds + (size_t)wid * G * DS;
    for (int j = lane * 4; j < G * DS; j += kWave * 4)
        *reinterpret_cast<float4 *>(&acc[j]) = make_float4(0.f, 0.f, 0.f, 0.f);
    const int grp = lane / KG;
    float *acc_g = acc + grp * DS;
    const int EP = G / HC;  // edges per wave step (HC <= G)
    const int eg = grp / HC, hh = grp % HC;
    const bool grp_ok = grp < EP * HC;
    const bool vec = flags & 1, nt = flags & 2;
    const float *ss = reinterpret_cast<const float *>(ss_t);
    // the weight this lane computes in a wave step (WeightLane): lane = slot * G + group
    const int wu = lane / G, wg = lane % G;
    const int weg = wg / HC, whh = wg % HC;
    const bool w_ok = wu < U && wg < EP * HC;

    // Edges [sb, se) of row q into dst rows of stride hstride per head, the statistics into
    // st_m / st_z [h * st_stride].  whole: the piece is the row, stored normalised; else it is
    // a hub row's piece, stored as it is.  Every head is stored, an empty piece as zeros.
    auto row_heads = [&](int q, int64_t sb, int64_t se, float *__restrict__ dst, int64_t hstride,
                         float *__restrict__ st_m, float *__restrict__ st_z, int64_t st_stride,
                         bool whole, bool to_out) {
        const int n = (int)(se - sb);
        float sd[HP], m[HP];
#pragma unroll
        for (int h = 0; h < HP; ++h) {
            sd[h] = h < H ? uniform(s_dst[h * (int64_t)num_rows + q]) : 0.f;
            m[h] = -INFINITY;
        }
        if (n > 0) piece_max<HP>(ss_t, col_idx + sb, n, H, sd, slope, lane, m);
        for (int h0 = 0; h0 < H; h0 += HC) {
            const int head = h0 + hh;
            const bool active = grp_ok && head < H;
            float mh = -INFINITY;
            WeightLane wl{wu, weg, 0, false, 0.f, 0.f};
#pragma unroll
            for (int h = 0; h < HP; ++h) {
                if (h == head) mh = m[h];
                if (h == h0 + whh && h < H && w_ok) {
                    wl.head = h;
                    wl.on = true;
                    wl.sdh = sd[h];
                    wl.shift = shift_of(m[h]);
                }
            }
            float ps = 0.f;
            wave_lds_fence();
            if (n > 0)
                ps = walk_attn<KG, HP, U, false, DROP>(
                    acc_g, col_idx, ss, wl, slope, rec, RS, (int)sb, (int)se, k, DS - 1, EP, eg,
                    active, lane, dm,
                    DropPass{h0 >> 2, ((min(h0 + HC, H) - 1) >> 2) - (h0 >> 2) + 1, head});
            // z of head h0 + j: its EP groups' sums in group order
            auto z_of = [&](int j) {
                float z = 0.f;
                for (int e = 0; e < EP; ++e) z += __shfl(ps, (e * HC + j) * KG);
                return uniform(z);
            };
            int bad = 0;
            for (int j = 0; j < HC && h0 + j < H; ++j)
                if (!(z_of(j) > 0.f)) bad |= 1 << j;
            if (whole && n > 0 && bad) {  // rare: NaN wherever such a head's row has an addend
                wave_lds_fence();
                walk_attn<KG, HP, U, true, false>(acc_g, col_idx, ss, wl, slope, rec, RS, (int)sb,
                                                  (int)se, k, DS - 1, EP, eg,
                                                  active && ((bad >> hh) & 1), lane, NoMask{},
                                                  DropPass{0, 1, 0});
            }
            wave_lds_fence();
            for (int j = 0; j < HC && h0 + j < H; ++j) {
                const float zj = z_of(j);
                const bool ok = !((bad >> j) & 1);
                float mul = 1.f;
                if constexpr (DROP) mul = dm.scale;
                flush_head<DROP>(acc + j * DS, EP, HC * DS, dst + (int64_t)(h0 + j) * hstride, D,
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
    };

    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);
    int r = it.r;

    // Continuation of row r - 1 (its token precedes d0): only a hub row leaves one, and a slab
    // per head for the fixup.
    int cont = -1;
    if (r > 0) {
        const RowPiece p =
            cont_piece(CutHubRows{}, it.p_lo, it.d1, r, row_ptr[r - 1], row_ptr[r], chunk);
        if (p.sb < p.se && p.hub) {
            row_heads(r - 1, p.sb, p.se, slab + (int64_t)item * D, (int64_t)n_items * D,
                      slab_m + item, slab_z + item, n_items, false, false);
            cont = r - 1;
        }
    }
    if (lane == 0) slab_row[item] = cont;

    // Rows whose token lies in [d0, d1): this item owns them.
    while (r < num_rows) {
        const int64_t rb = row_ptr[r];
        if (!row_owned(it.d1, r, rb)) break;
        const RowPiece p = row_piece(CutHubRows{}, it.d1, r, rb, row_ptr[r + 1], chunk);
        row_heads(r, rb, p.se, out + (int64_t)r * D, (int64_t)num_rows * D, row_max + r,
                  row_sum + r, num_rows, !p.hub, true);
        ++r;
    }
}

// The merge of a hub row's pieces, one head per blockIdx.y, 16 lanes per item as
// slab_fixup_kernel: the thread group of the first item holding a slab of the row merges the
// owner's piece (in out and the statistics) and the row's slabs in item order.  Every hub row
// has a slab: it is longer than an item.  DROP: the merged quotient times mul, the mask's scale.
template <bool DROP>
__global__ __launch_bounds__(kBlock) void gath_fixup_kernel(
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
    const float shift = shift_of(m);
    const float c0 = expf(m0 - shift);
    float z = z0 * c0;
    for (int i = 0; i < n; ++i) z += sz[i] * expf(sm[i] - shift);
    if (z > 0.f) {
        for (int j = g; j < D; j += 16) {
            float a = o[j] * c0;
            for (int i = 0; i < n; ++i) a += sl[(int64_t)i * D + j] * expf(sm[i] - shift);
            o[j] = DROP ? a / z * mul : a / z;
        }
    } else {  // rare: NaN wherever the row has an addend, 0 elsewhere
        for (int j = g; j < D; j += 16) o[j] = 0.f;
        __threadfence();  // the zeros land before the NaNs of other lanes
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

// w[h, e] = exp(l_he - row_max[h, r]) / row_sum[h, r]: one thread per edge, blocks of
// kAlphaPer * kBlock consecutive edges; a thread finds its row between the rows of the block's
// first and last edge.
constexpr int kAlphaPer = 4;

// the last row r in [lo, hi] with row_ptr[r] <= e (row_ptr[lo] <= e < row_ptr[hi + 1])
__device__ __forceinline__ int row_of_edge(const int32_t *__restrict__ row_ptr, int lo, int hi,
                                           int64_t e) {
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (row_ptr[mid] <= e)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

template <int HP>
__global__ __launch_bounds__(kBlock) void gath_alpha_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const VecF<HP> *__restrict__ ss_t, const float *__restrict__ s_dst, float slope,
    const float *__restrict__ row_max, const float *__restrict__ row_sum, float *__restrict__ w,
    int H, int num_rows, int64_t num_e) {
    const int64_t eb = blockIdx.x * (int64_t)(kAlphaPer * kBlock);
    if (eb >= num_e) return;
    const int64_t ee = eb + kAlphaPer * kBlock < num_e ? eb + kAlphaPer * kBlock : num_e;
    const int r_lo = row_of_edge(row_ptr, 0, num_rows - 1, eb);
    const int r_hi = row_of_edge(row_ptr, r_lo, num_rows - 1, ee - 1);
#pragma unroll
    for (int u = 0; u < kAlphaPer; ++u) {
        const int64_t e = eb + u * kBlock + threadIdx.x;
        if (e >= ee) break;
        const int64_t r = row_of_edge(row_ptr, r_lo, r_hi, e);
        const VecF<HP> x = ss_t[(uint32_t)col_idx[e]];
#pragma unroll
        for (int h = 0; h < HP; ++h) {
            if (h < H) {
                const float l = leaky(s_dst[h * (int64_t)num_rows + r] + x.v[h], slope);
                const float p = expf(l - shift_of(row_max[h * (int64_t)num_rows + r]));
                w[h * num_e + e] = p / row_sum[h * (int64_t)num_rows + r];
            }
        }
    }
}

// A piece is addressed through a descriptor of 4 * n bytes with 32-bit offsets.
constexpr int kAttnMaxChunk = 1 << 24;

struct AttnLayout {
    int chunk, n_items, RS, DS, kg, hc, hp;
    bool wide;
    size_t ss_off, slab_off, m_off, z_off, row_off, total;
};

AttnLayout attn_layout(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k, int H,
                       int chunk) {
    AttnLayout L{};
    L.RS = record_stride(k, num_cols);
    L.DS = copy_stride(D);
    L.hp = hp_of(H);
    const int g = lanes_per_edge(k);
    L.kg = g < 8 ? 8 : g;
    const int G = kWave / L.kg;
    const int np = (H + G - 1) / G;
    L.hc = (H + np - 1) / np;
    L.wide = !(num_cols < (1 << 24) && (uint64_t)num_cols * (uint64_t)L.RS < (1ull << 32));
    // resident waves per CU: 4 or 5 per SIMD by VGPRs, fewer when the LDS copies fill the CU first
    const size_t per_block = (size_t)kWavesPerBlock * G * L.DS * sizeof(float);
    const int by_lds = (int)(kPullLdsBytes / per_block) * kWavesPerBlock;
    const int by_regs = L.hp == 8 ? 16 : 20;
    L.chunk = fwd_chunk(num_rows, num_e, chunk, by_lds < by_regs ? by_lds : by_regs);
    if (L.chunk > kAttnMaxChunk) L.chunk = kAttnMaxChunk;
    L.n_items = token_items(num_rows, num_e, L.chunk);
    const int64_t cap = item_cap(num_rows + num_e, chunk, L.n_items);
    const size_t stat = al256((size_t)cap * H * sizeof(float));
    L.ss_off = al256((size_t)num_cols * L.RS);
    L.slab_off = L.ss_off + al256((size_t)num_cols * L.hp * sizeof(float));
    L.m_off = L.slab_off + al256((size_t)cap * H * D * sizeof(float));
    L.z_off = L.m_off + stat;
    L.row_off = L.z_off + stat;
    L.total = L.row_off + al256((size_t)cap * sizeof(int32_t));
    return L;
}

template <int HP>
int launch_interleave(const float *s_src, void *ss_t, int H, int64_t num_cols, hipStream_t s) {
    hipLaunchKernelGGL(gath_interleave_kernel<HP>, dim3((unsigned)ceil_div(num_cols, kBlock)),
                       dim3(kBlock), 0, s, s_src, reinterpret_cast<VecF<HP> *>(ss_t), H, num_cols);
    MAXK_LAUNCHED("gath_interleave_kernel");
    return MAXK_OK;
}

template <int HP, bool DROP>
int launch_attention(const int32_t *row_ptr, const int32_t *col_idx, const float *s_dst,
                     const float *s_src, float slope, const float *cbsr_val,
                     const uint8_t *cbsr_idx, float *out, float *row_max, float *row_sum,
                     int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k, int H,
                     const AttnLayout &L, void *workspace, hipStream_t s,
                     const MaskArg<DROP> &dm) {
    char *ws = reinterpret_cast<char *>(workspace);
    uint8_t *rec = reinterpret_cast<uint8_t *>(ws);
    VecF<HP> *ss_t = reinterpret_cast<VecF<HP> *>(ws + L.ss_off);
    float *slab = reinterpret_cast<float *>(ws + L.slab_off);
    float *slab_m = reinterpret_cast<float *>(ws + L.m_off);
    float *slab_z = reinterpret_cast<float *>(ws + L.z_off);
    int32_t *slab_row = reinterpret_cast<int32_t *>(ws + L.row_off);
    if (int rc = launch_cbsr_pack(cbsr_val, cbsr_idx, rec, num_cols, k, L.RS, D, L.DS - 1, s))
        return rc;
    if (int rc = launch_interleave<HP>(s_src, ss_t, H, num_cols, s)) return rc;
    constexpr int U = MAXK_FWD_U;
    const int G = kWave / L.kg;
    const size_t lds = (size_t)kWavesPerBlock * G * L.DS * sizeof(float);
    const dim3 grid = item_grid(L.n_items);
    const bool big = (double)H * num_rows * D * 4 > (double)kInfinityCacheBytes;
    const int flags = (D % 4 == 0 && ((uintptr_t)out & 15) == 0 ? 1 : 0) |
                      ((MAXK_FWD_OUT_NT == 1 || (MAXK_FWD_OUT_NT == 2 && big)) ? 2 : 0);
    const bool ok = with_const<8, 16, 32, 64>(L.kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        hipLaunchKernelGGL((gath_fwd_kernel<KG, HP, U, DROP>), grid, dim3(kBlock), lds, s, row_ptr,
                           col_idx, ss_t, s_dst, slope, rec, L.RS, out, row_max, row_sum, slab,
                           slab_m, slab_z, slab_row, (int)num_rows, num_e, D, L.DS, k, L.chunk,
                           L.n_items, H, L.hc, flags, dm);
    });
    if (!ok) return bad_lanes(L.kg);
    MAXK_LAUNCHED("gath_fwd_kernel");
    float mul = 1.f;
    if constexpr (DROP) mul = dm.scale;
    hipLaunchKernelGGL(gath_fixup_kernel<DROP>,
                       dim3((unsigned)ceil_div(L.n_items, kBlock / 16), (unsigned)H), dim3(kBlock),
                       0, s, row_ptr, col_idx, rec, L.RS, k, slab, slab_m, slab_z, slab_row, out,
                       row_max, row_sum, num_rows, D, L.n_items, mul);
    MAXK_LAUNCHED("gath_fixup_kernel");
    return MAXK_OK;
}

template <int HP>
int launch_alpha(const int32_t *row_ptr, const int32_t *col_idx, const float *s_dst,
                 const float *s_src, float slope, const float *row_max, const float *row_sum,
                 float *w, int H, int64_t num_rows, int64_t num_cols, int64_t num_e,
                 void *workspace, hipStream_t s) {
    if (int rc = launch_interleave<HP>(s_src, workspace, H, num_cols, s)) return rc;
    hipLaunchKernelGGL(gath_alpha_kernel<HP>,
                       dim3((unsigned)ceil_div(num_e, (int64_t)kAlphaPer * kBlock)), dim3(kBlock),
                       0, s, row_ptr, col_idx, reinterpret_cast<const VecF<HP> *>(workspace),
                       s_dst, slope, row_max, row_sum, w, H, (int)num_rows, num_e);
    MAXK_LAUNCHED("gath_alpha_kernel");
    return MAXK_OK;
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" size_t maxk_gat_attention_heads_workspace_size(int64_t num_rows, int64_t num_cols,
                                                          int64_t num_e, int32_t dim_origin,
                                                          int32_t dim_k, int32_t num_heads,
                                                          int32_t chunk_edges) {
    if (num_rows < 0 || num_cols < 0 || num_e < 0 || dim_origin <= 0 || dim_k <= 0 ||
        chunk_edges < 0 || num_heads < 1 || num_heads > MAXK_MAX_HEADS)
        return 0;
    return attn_layout(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads, chunk_edges).total;
}

namespace {
// Both attention entries; dm: the dropout entry's mask, null for none.
int attention_heads(const int32_t *row_ptr, const int32_t *col_idx, const float *s_dst,
                    const float *s_src, float negative_slope, const float *cbsr_val,
                    const uint8_t *cbsr_idx, float *out, float *row_max, float *row_sum,
                    int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin,
                    int32_t dim_k, int32_t num_heads, int32_t chunk_edges, void *workspace,
                    size_t workspace_bytes, void *stream, const DropMask *dm) {
    if (int rc = check_heads(num_heads)) return rc;
    if (int rc = check_sizes(num_rows, num_cols, num_e, chunk_edges)) return rc;
    if (int rc = check_slope(negative_slope)) return rc;
    MAXK_REQUIRE(dim_origin >= 1 && dim_origin <= kMaxDim, "dim_origin must be in [1,256], got %d",
                 dim_origin);
    MAXK_REQUIRE(dim_k >= 1 && dim_k <= dim_origin, "dim_k must be in [1,dim_origin], got %d",
                 dim_k);
    MAXK_REQUIRE(num_cols * (int64_t)dim_k < (1LL << 31), "num_cols*k too large");
    if (num_rows == 0) return MAXK_OK;
    MAXK_REQUIRE(row_ptr && out && row_max && row_sum,
                 "row_ptr / out / row_max / row_sum must not be NULL");
    const int D = dim_origin, k = dim_k, H = num_heads;
    hipStream_t s = as_stream(stream);
    if (num_e == 0) {  // nothing to walk: zero rows and statistics
        if (int rc = zero_words(out, (int64_t)H * num_rows * D, s)) return rc;
        if (int rc = zero_words(row_max, (int64_t)H * num_rows, s)) return rc;
        return zero_words(row_sum, (int64_t)H * num_rows, s);
    }
    MAXK_REQUIRE(col_idx && s_dst && s_src && cbsr_val && cbsr_idx,
                 "col_idx / s_dst / s_src / cbsr_val / cbsr_idx must not be NULL");
    MAXK_REQUIRE(num_cols > 0, "edges present but num_cols == 0");
    const AttnLayout L = attn_layout(num_rows, num_cols, num_e, D, k, H, chunk_edges);
    MAXK_REQUIRE(!L.wide, "num_cols: the fused attention takes tables below 2^24 columns and "
                 "4 GiB of records (%lld columns of %d bytes)", (long long)num_cols, L.RS);
    if (int rc = check_workspace(workspace, workspace_bytes, L.total)) return rc;
    MAXK_REQUIRE(((uintptr_t)cbsr_val & 3) == 0 && ((uintptr_t)s_dst & 3) == 0 &&
                     ((uintptr_t)s_src & 3) == 0 && ((uintptr_t)out & 3) == 0 &&
                     ((uintptr_t)row_max & 3) == 0 && ((uintptr_t)row_sum & 3) == 0,
                 "float buffers must be 4-B aligned");
#define MAXK_GATH_FWD(HP, DROP, DM)                                                             \
    launch_attention<HP, DROP>(row_ptr, col_idx, s_dst, s_src, negative_slope, cbsr_val,        \
                               cbsr_idx, out, row_max, row_sum, num_rows, num_cols, num_e, D, k, \
                               H, L, workspace, s, DM)
    if (dm) {
        switch (L.hp) {
            case 2: return MAXK_GATH_FWD(2, true, *dm);
            case 4: return MAXK_GATH_FWD(4, true, *dm);
            default: return MAXK_GATH_FWD(8, true, *dm);
        }
    }
    switch (L.hp) {
        case 2: return MAXK_GATH_FWD(2, false, NoMask{});
        case 4: return MAXK_GATH_FWD(4, false, NoMask{});
        default: return MAXK_GATH_FWD(8, false, NoMask{});
    }
#undef MAXK_GATH_FWD
}
}  // namespace

extern "C" int maxk_gat_attention_heads(const int32_t *row_ptr, const int32_t *col_idx,
                                        const float *s_dst, const float *s_src,
                                        float negative_slope, const float *cbsr_val,
                                        const uint8_t *cbsr_idx, float *out, float *row_max,
                                        float *row_sum, int64_t num_rows, int64_t num_cols,
                                        int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                        int32_t num_heads, int32_t chunk_edges, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    clear_error();
    return attention_heads(row_ptr, col_idx, s_dst, s_src, negative_slope, cbsr_val, cbsr_idx, out,
                           row_max, row_sum, num_rows, num_cols, num_e, dim_origin, dim_k,
                           num_heads, chunk_edges, workspace, workspace_bytes, stream, nullptr);
}

extern "C" size_t maxk_gat_attention_heads_dropout_workspace_size(
    int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
    int32_t num_heads, int32_t chunk_edges) {
    return maxk_gat_attention_heads_workspace_size(num_rows, num_cols, num_e, dim_origin, dim_k,
                                                   num_heads, chunk_edges);
}

extern "C" int maxk_gat_attention_heads_dropout(
    const int32_t *row_ptr, const int32_t *col_idx, const float *s_dst, const float *s_src,
    float negative_slope, const float *cbsr_val, const uint8_t *cbsr_idx, float *out,
    float *row_max, float *row_sum, int64_t num_rows, int64_t num_cols, int64_t num_e,
    int32_t dim_origin, int32_t dim_k, int32_t num_heads, int32_t chunk_edges, float p,
    uint64_t seed, void *workspace, size_t workspace_bytes, void *stream) {
    clear_error();
    if (int rc = check_dropout(p)) return rc;
    // p == 0 drops nothing and scales by 1: the kernels of the entry without dropout
    const DropMask dm = drop_mask(p, seed);
    return attention_heads(row_ptr, col_idx, s_dst, s_src, negative_slope, cbsr_val, cbsr_idx, out,
                           row_max, row_sum, num_rows, num_cols, num_e, dim_origin, dim_k,
                           num_heads, chunk_edges, workspace, workspace_bytes, stream,
                           p > 0.f ? &dm : nullptr);
}

extern "C" size_t maxk_gat_edge_alpha_heads_workspace_size(int32_t num_heads, int64_t num_rows,
                                                           int64_t num_cols, int64_t num_e) {
    if (!sizes_ok(num_rows, num_cols, num_e) || num_heads < 1 || num_heads > MAXK_MAX_HEADS)
        return 0;
    return al256((size_t)num_cols * hp_of(num_heads) * sizeof(float));
}

extern "C" int maxk_gat_edge_alpha_heads(const int32_t *row_ptr, const int32_t *col_idx,
                                         const float *s_dst, const float *s_src,
                                         float negative_slope, const float *row_max,
                                         const float *row_sum, float *w, int32_t num_heads,
                                         int64_t num_rows, int64_t num_cols, int64_t num_e,
                                         void *workspace, size_t workspace_bytes, void *stream) {
    clear_error();
    if (int rc = check_heads(num_heads)) return rc;
    if (int rc = check_sizes(num_rows, num_cols, num_e, 0)) return rc;
    if (int rc = check_slope(negative_slope)) return rc;
    if (num_e == 0) return MAXK_OK;  // no edge, nothing to write
    MAXK_REQUIRE(num_rows > 0 && num_cols > 0, "edges present but num_rows or num_cols == 0");
    MAXK_REQUIRE(row_ptr && col_idx && s_dst && s_src && row_max && row_sum && w,
                 "row_ptr / col_idx / s_dst / s_src / row_max / row_sum / w must not be NULL");
    const size_t need = al256((size_t)num_cols * hp_of(num_heads) * sizeof(float));
    if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    hipStream_t s = as_stream(stream);
#define MAXK_GATH_ALPHA(HP)                                                                     \
    launch_alpha<HP>(row_ptr, col_idx, s_dst, s_src, negative_slope, row_max, row_sum, w,      \
                     num_heads, num_rows, num_cols, num_e, workspace, s)
    switch (hp_of(num_heads)) {
        case 2: return MAXK_GATH_ALPHA(2);
        case 4: return MAXK_GATH_ALPHA(4);
        default: return MAXK_GATH_ALPHA(8);
    }
#undef MAXK_GATH_ALPHA
}
