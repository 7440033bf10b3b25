// Fused multi-head GAT attention for gfx950: the edge softmax inside the aggregation walk,
//
//   out[h, r, cbsr_idx[c, l]] += alpha[h, e] * cbsr_val[c, l]       e in row r, c = col_idx[e]
//   alpha[h, e] = exp(l_he - m_hr) / z_hr          l_he = leaky_relu(s_dst[h, r] + s_src[h, c])
//   m_hr = max_e l_he                              z_hr = sum_e exp(l_he - m_hr)
//
// what maxk_gat_edge_softmax_heads followed by maxk_spgemm_forward_heads compute, without alpha
// [H, E] ever existing: not in an output, not in the workspace.  The row statistics
// row_max = m and row_sum = z are outputs, and maxk_gat_edge_alpha_heads rebuilds alpha from
// them for the backward.  The walk is the hub-row heads walk of heads_walk.h, shared with
// spgemm_fwd_heads.hip and dot_attention_heads.hip (records packed once, token-stream items, one
// wavefront per item under CutHubRows, KG lanes per group, G = 64 / KG LDS copies of the output
// row, the heads in passes of HC; its rules of the copies, the trash column, the slabs and the
// softmax rows are stated there), with edge_softmax_heads.hip's scores (interleaved to ss_t
// [num_cols, HP], one aligned vector per column):
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
//  3. softmax_fixup_kernel (heads_walk.h) merges a hub row's pieces in item order.
// A row whose z is not a positive number is NaN wherever it has an addend and exactly 0
// elsewhere (heads_walk.h): those rows are walked once more with the weight NaN (POISON) and
// stored undivided.  A row without edges stores zeros in out and both statistics.
// No global atomics, no LDS atomics; every sum has an order fixed by (graph, chunk, k, H), so
// the result is bitwise repeatable, and head h's slice is computed from head h's scores only.
// LDS per wave as the multi-head forward (G * DS floats); 87 to 96 VGPRs at HP = 2 and 4 (five
// waves per SIMD), 108 or 109 at HP = 8 (four); no scratch.
// maxk_gat_attention_heads_dropout is the same walk with the attention-dropout mask of
// attn_dropout.h multiplied in (the DROP instantiations): out sums alpha * d * value, the
// statistics stay those of the undropped softmax, p == 0 launches the kernels without a mask.
#include <cmath>

#include "attn_dropout.h"
#include "edge_softmax.h"
#include "heads_walk.h"

namespace maxk {
namespace {

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
// DROP: the pass mask of attn_dropout.h (PassMask) multiplied into the products; the sum of p
// takes the unmasked weights.
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
    PassMask<DROP> pm(dp, EP * U);
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
            pm.refresh(dm, dp, sb + base, lane);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                w[u] = __shfl(pt, u * G + grp);
                ps += w[u];
                if constexpr (DROP) w[u] *= pm.keep(u * EP + eg);
            }
            pm.next();
        }
        scatter_records<KG, U>(acc_g, rrs, RS, k, trash, l0, c, w, active, base, EP, eg, n);
    }
    return ps;
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
    // flags: store_flags (heads_walk.h)
    constexpr int G = kWave / KG;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = lane_id();
    const int item = wave_item();
    if (item >= n_items) return;  // whole wave; no workgroup barrier below
    float *acc = lds + (size_t)(threadIdx.x / kWave) * G * DS;
    zero_wave_lds(acc, G * DS, lane);
    const PassGeom<KG> g(lane, HC, acc, DS);
    const bool vec = flags & 1, nt = flags & 2;
    const float *ss = reinterpret_cast<const float *>(ss_t);
    // the weight this lane computes in a wave step (WeightLane): lane = slot * G + group
    const int wu = lane / G, wg = lane % G;
    const int weg = wg / HC, whh = wg % HC;
    const bool w_ok = wu < U && wg < g.EP * HC;

    // Edges [sb, se) of row q: an owned row's into out and the row statistics, a continuation's
    // into the item's slab and slab statistics.  Every head is stored, an empty piece as zeros.
    walk_hub_item(row_ptr, slab_row, num_rows, num_e, item, chunk, lane,
                  [&](int q, int64_t sb, int64_t se, bool whole, bool to_out) {
        float *__restrict__ dst = to_out ? out + (int64_t)q * D : slab + (int64_t)item * D;
        const int64_t hstride = (int64_t)(to_out ? num_rows : n_items) * D;
        float *__restrict__ st_m = to_out ? row_max + q : slab_m + item;
        float *__restrict__ st_z = to_out ? row_sum + q : slab_z + item;
        const int64_t st_stride = to_out ? num_rows : n_items;
        const int n = (int)(se - sb);
        float sd[HP], m[HP];
#pragma unroll
        for (int h = 0; h < HP; ++h) {
            sd[h] = h < H ? uniform(s_dst[h * (int64_t)num_rows + q]) : 0.f;
            m[h] = -INFINITY;
        }
        if (n > 0) piece_max<HP>(ss_t, col_idx + sb, n, H, sd, slope, lane, m);
        for (int h0 = 0; h0 < H; h0 += HC) {
            const int head = h0 + g.hh;
            const bool active = g.grp_ok && head < H;
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
                    g.acc_g, col_idx, ss, wl, slope, rec, RS, (int)sb, (int)se, k, DS - 1, g.EP,
                    g.eg, active, lane, dm, drop_pass(h0, HC, H, head));
            const int bad = bad_heads<KG>(ps, g.EP, HC, h0, H);
            if (whole && n > 0 && bad) {  // rare: NaN wherever such a head's row has an addend
                wave_lds_fence();
                walk_attn<KG, HP, U, true, false>(g.acc_g, col_idx, ss, wl, slope, rec, RS,
                                                  (int)sb, (int)se, k, DS - 1, g.EP, g.eg,
                                                  active && ((bad >> g.hh) & 1), lane, NoMask{},
                                                  DropPass{0, 1, 0});
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

struct AttnLayout {
    int chunk, n_items, hc, hp;
    size_t lds, ss_off;  // lds: per workgroup
    RecordGeom R;
    SlabLayout S;
};

AttnLayout attn_layout(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k, int H,
                       int chunk) {
    AttnLayout L{};
    L.R = record_geom(num_cols, D, k);
    L.hp = hp_of(H);
    L.hc = heads_per_pass(H, L.R.kg);
    // resident waves per CU: 4 or 5 per SIMD by VGPRs, fewer when the LDS copies fill the CU first
    L.lds = (size_t)kWavesPerBlock * (kWave / L.R.kg) * L.R.DS * sizeof(float);
    L.chunk = walk_chunk(num_rows, num_e, chunk, L.lds, L.hp == 8 ? 16 : 20);
    L.n_items = token_items(num_rows, num_e, L.chunk);
    L.ss_off = al256((size_t)num_cols * L.R.RS);
    L.S = slab_layout(item_cap(num_rows + num_e, chunk, L.n_items), H, D,
                      L.ss_off + al256((size_t)num_cols * L.hp * sizeof(float)), true);
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
    float *slab = reinterpret_cast<float *>(ws + L.S.slab_off);
    float *slab_m = reinterpret_cast<float *>(ws + L.S.m_off);
    float *slab_z = reinterpret_cast<float *>(ws + L.S.z_off);
    int32_t *slab_row = reinterpret_cast<int32_t *>(ws + L.S.row_off);
    const RecordGeom &R = L.R;
    if (int rc = launch_cbsr_pack(cbsr_val, cbsr_idx, rec, num_cols, k, R.RS, D, R.DS - 1, s))
        return rc;
    if (int rc = launch_interleave<HP>(s_src, ss_t, H, num_cols, s)) return rc;
    constexpr int U = MAXK_FWD_U;
    const int flags = store_flags(out, H, num_rows, D);
    const bool ok = with_const<8, 16, 32, 64>(R.kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        hipLaunchKernelGGL((gath_fwd_kernel<KG, HP, U, DROP>), item_grid(L.n_items), dim3(kBlock),
                           L.lds, s, row_ptr, col_idx, ss_t, s_dst, slope, rec, R.RS, out, row_max,
                           row_sum, slab, slab_m, slab_z, slab_row, (int)num_rows, num_e, D, R.DS,
                           k, L.chunk, L.n_items, H, L.hc, flags, dm);
    });
    if (!ok) return bad_lanes(R.kg);
    MAXK_LAUNCHED("gath_fwd_kernel");
    float mul = 1.f;
    if constexpr (DROP) mul = dm.scale;
    return launch_softmax_fixup<DROP>(row_ptr, col_idx, rec, R.RS, k, slab, slab_m, slab_z,
                                      slab_row, out, row_max, row_sum, num_rows, D, L.n_items, H,
                                      mul, s);
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
    return attn_layout(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads, chunk_edges)
        .S.end;
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
    if (int rc = check_cbsr_dims(dim_origin, dim_k, num_cols)) return rc;
    if (num_rows == 0) return MAXK_OK;
    MAXK_REQUIRE(row_ptr && out && row_max && row_sum,
                 "row_ptr / out / row_max / row_sum must not be NULL");
    const int D = dim_origin, k = dim_k, H = num_heads;
    hipStream_t s = as_stream(stream);
    if (num_e == 0) return zero_heads_out(out, row_max, row_sum, H, num_rows, D, s);
    MAXK_REQUIRE(col_idx && s_dst && s_src && cbsr_val && cbsr_idx,
                 "col_idx / s_dst / s_src / cbsr_val / cbsr_idx must not be NULL");
    MAXK_REQUIRE(num_cols > 0, "edges present but num_cols == 0");
    const AttnLayout L = attn_layout(num_rows, num_cols, num_e, D, k, H, chunk_edges);
    MAXK_REQUIRE(!L.R.wide, "num_cols: the fused attention takes tables below 2^24 columns and "
                 "4 GiB of records (%lld columns of %d bytes)", (long long)num_cols, L.R.RS);
    if (int rc = check_workspace(workspace, workspace_bytes, L.S.end)) return rc;
    MAXK_REQUIRE(((uintptr_t)cbsr_val & 3) == 0 && ((uintptr_t)s_dst & 3) == 0 &&
                     ((uintptr_t)s_src & 3) == 0 && ((uintptr_t)out & 3) == 0 &&
                     ((uintptr_t)row_max & 3) == 0 && ((uintptr_t)row_sum & 3) == 0,
                 "float buffers must be 4-B aligned");
    return with_heads_mask(L.hp, dm, [&](auto hp_c, const auto &mask) {
        return launch_attention<decltype(hp_c)::value, is_drop_v<decltype(mask)>>(
            row_ptr, col_idx, s_dst, s_src, negative_slope, cbsr_val, cbsr_idx, out, row_max,
            row_sum, num_rows, num_cols, num_e, D, k, H, L, workspace, s, mask);
    });
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
    return with_dropout(p, seed, [&](const DropMask *dm) {
        return attention_heads(row_ptr, col_idx, s_dst, s_src, negative_slope, cbsr_val, cbsr_idx,
                               out, row_max, row_sum, num_rows, num_cols, num_e, dim_origin, dim_k,
                               num_heads, chunk_edges, workspace, workspace_bytes, stream, dm);
    });
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
