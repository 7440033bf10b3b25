// Fused backward of the multi-head dot-product attention on CBSR keys (dot_attention_heads.hip)
// for gfx950: the coefficients, their gradient, the softmax backward and both feature
// contributions of every edge in one walk of the graph, without alpha [H, E], grad_alpha [H, E]
// or the logits' gradient head-major [H, E] ever existing.
//
//   l_he     = scale * sum_l cbsr_val[c, l] * q[h, r, s]          e in row r, c = col_idx[e],
//   alpha_he = exp(l_he - row_max[h, r]) / row_sum[h, r]          s = cbsr_idx[c, l]
//   ga_he    = sum_l cbsr_val[c, l] * grad_out[h, r, s]
//   t_hr     = sum_{j : out[h, r, j] != 0} out[h, r, j] * grad_out[h, r, j]
//   gl_he    = alpha_he * (ga_he - t_hr)
//   grad_q[h, r, j]  = scale * sum_{e in r} gl_he * x_c[j]        x_c the scattered CBSR row
//   grad_cbsr[c, l]  = sum_h sum_{e -> c} (alpha_he * grad_out[h, r, s] + scale * gl_he * q[h, r, s])
//
// t is the softmax backward's sum_e alpha_he * ga_he, which equals the dot product of the two
// dense rows out[h, r, :] and grad_out[h, r, :] (stage_dot, piece_walk.h): every item
// computes it for itself before it touches an edge, so a row cut over items needs no second walk.
//
//  1. launch_cbsr_pack fills the workspace's records.
//  2. datb_walk_kernel (walk A), a staged-row walk (piece_walk.h): one wavefront per item of
//     `chunk` tokens cut at the item's end (CutAtEnd), KG = pow2ceil(k) lanes per edge (8 .. 64),
//     G = 64 / KG edges per wave step, U steps in flight.
//     * per row piece: the H rows grad_out[h, r, :] and the H rows scale * q[h, r, :] staged side
//       by side in the wave's LDS (2 * H * DS floats, the pad columns [D, DS) zero), out[h, r, :]
//       streamed beside them, t_h reduced by the fixed 64-lane butterfly: the same number in
//       every item holding a piece of the row.  Lane h < H of every group keeps row_max, row_sum
//       and t of head h.
//     * per edge: one col_idx load and one packed record.  Per head the group forms the logit by
//       the device functions of dot_logit.h -- the forward's and the alpha entry's, on the same
//       staged row, so exp(l - row_max) <= 1 exactly as there -- and ga_h by the group's
//       butterfly over value * g_h[selector] (a folded or skipped selector adds nothing); lane h
//       keeps both and forms alpha_h (one expf, one division) and gl_h.
//     * T[e, l] = sum_h (alpha_h * g_h[s] + gl_h * sq_h[s]) in head order, a product first and
//       one fma per further term, sq the staged scale * q.  The record's low selector byte is the
//       caller's selector, so a repeated selector's slot receives the column's gradient although
//       the pack folded its value; a selector >= D reads the zero pad.
//     * the group's HP lanes store glT[e, 0:HP] (pad heads 0), all lanes the row T[e, 0:k].
//       k > 64: the logit and ga in passes over l per head, then T in passes over l, the record
//       reloaded from the caches.
//  3. datb_gq_kernel (aggregation B): the hub-row heads walk of heads_walk.h under CutHubRows
//     with the weights read from glT[e * HP + h]; the flush multiplies by scale.  gl is final, so
//     a hub row's pieces are added by slab_fixup_kernel in item order.  Every row of every head
//     is stored, an edgeless row as zeros.
//  4. csc_sum_rows: grad_cbsr from T through the CSC, in slot order (the csc phase 2).
// No global atomics, no LDS atomics; every sum has an order fixed by (graph, chunk, k, H).  Head
// h's slice of grad_q is computed from head h's q, statistics, out and grad_out alone.
// LDS per wave: walk A 2 * H * DS floats (16.6 KB at H = 8, D = 256: 8 waves per CU), B G * DS.
// maxk_dot_attention_heads_dropout_backward is the same sequence with the attention-dropout mask
// of attn_dropout.h in walk A (the DROP instantiations): gl = alpha * (d * ga - t) and
// T = sum_h (alpha * d * g + gl * sq), t from the dropped out; B, glT and the CSC sum are
// unchanged; p == 0 launches the kernels without a mask.
#include <cmath>

#include "attn_dropout.h"
#include "dot_logit.h"
#include "sspmm_bwd.h"

// Wave steps of record loads in flight in walk A.
#ifndef MAXK_DATB_U
#define MAXK_DATB_U 4
#endif

namespace maxk {
namespace {

// What lane h of a group holds of head h for the row being walked (pad heads: 0, 1, 0).
struct HeadLane {
    float shift, sum, t;
};

// The edges [sb, se) (sb < se) of one row whose grad_out rows are staged in grow and whose scaled
// query rows are staged in qrow: stores their T rows and glT vectors.  DROP: lane h takes its
// head's bits of the step from step_gone (attn_dropout.h) and keeps alpha * d beside alpha:
// T gains alpha * d * g and gl = alpha * (d * ga - t), t from the dropped out.
template <int KG, int HP, int U, bool DROP>
__device__ __forceinline__ void walk_piece_bwd(const float *grow, const float *qrow, int DS,
                                               const int32_t *__restrict__ col_idx,
                                               const uint8_t *__restrict__ rec, int RS,
                                               float *__restrict__ T, float *__restrict__ glT,
                                               int H, int D, int sb, int se, int k,
                                               const HeadLane &hd, int lane,
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
    const auto zrs = wave_buffer(glT + (size_t)(uint32_t)sb * HP, (uint32_t)n * HP * 4u);
    for (int base = 0; base < n; base += G * U) {
        int c[U];
#pragma unroll
        for (int u = 0; u < U; ++u)  // past the piece's end the column reads 0 (column 0)
            c[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(crs, (base + u * G + grp) * 4, 0, 0);
        // lane h of the group: head h's logit and ga of each of the group's U edges
        float lg[U], ga[U];
#pragma unroll
        for (int u = 0; u < U; ++u) lg[u] = ga[u] = 0.f;
        // DROP, lane h: bit u, head h of the group's edge u is dropped
        const uint32_t gone = step_gone<KG, HP, U, DROP>(dm, sb + base, grp, l0, lane0);
        // lane h: alpha and gl from them; al is the coefficient of the feature gradient, alpha,
        // under DROP alpha * d
        auto finish = [&](float (&al)[U], float (&gl)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) al[u] = gl[u] = 0.f;
            if (hl) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float p = expf(lg[u] - hd.shift);
                    al[u] = hon ? p / hd.sum : 0.f;
                    if constexpr (DROP) {
                        const float d = (gone >> u) & 1u ? 0.f : dm.scale;
                        gl[u] = al[u] * (d * ga[u] - hd.t);
                        al[u] *= d;
                    } else {
                        gl[u] = al[u] * (ga[u] - hd.t);  // a pad head: 0 * (0 - 0)
                    }
                }
            }
        };
        float al[U], gl[U];
        if (k <= KG) {  // one slot per lane: the record is loaded once for all heads
            const RecordSlot sl(l0, k);
            const PackedSrc src = sl.src(rrs, k, RS);
            float v[U];
            int s[U], sr[U];
#pragma unroll
            for (int u = 0; u < U; ++u) src.load(c[u], v[u], s[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) sr[u] = s[u];  // s stays for the logit
            const uint32_t keep = caller_columns(sr, sl.ok, D, trash);
#pragma unroll
            for (int h = 0; h < HP; ++h) {
                if (h < H) {
                    const float *gh = grow + h * DS, *qh = qrow + h * DS;
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const float l =
                            lane_tree<KG, Sum>(dot_term(v[u], s[u], qh, trash, sl.ok, 0.f));
                        // a slot without a kept value adds nothing, whatever x is
                        const float x = gh[sr[u]];
                        const float d = lane_tree<KG, Sum>((keep >> u) & 1u ? v[u] * x : 0.f);
                        lg[u] = l0 == h ? l : lg[u];
                        ga[u] = l0 == h ? d : ga[u];
                    }
                }
            }
            finish(al, gl);
            float tc[U];
#pragma unroll
            for (int h = 0; h < HP; ++h) {
                if (h < H) {
                    const float *gh = grow + h * DS, *qh = qrow + h * DS;
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const float a = __shfl(al[u], lane0 + h), b = __shfl(gl[u], lane0 + h);
                        tc[u] = h == 0 ? a * gh[sr[u]] : __builtin_fmaf(a, gh[sr[u]], tc[u]);
                        tc[u] = __builtin_fmaf(b, qh[sr[u]], tc[u]);
                    }
                }
            }
            store_t_rows<KG, U>(trs, tc, sl.ok, base, grp, k, l0);
        } else {  // k > 64 (KG == 64, one edge per wave step): passes over l
#pragma unroll
            for (int h = 0; h < HP; ++h) {
                if (h < H) {
                    const float *gh = grow + h * DS;
                    float l[U], acc[U];
                    record_dots<KG, U>(rrs, RS, c, qrow + h * DS, k, trash, l0, l);
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
                        lg[u] = l0 == h ? l[u] : lg[u];
                        ga[u] = l0 == h ? d : ga[u];
                    }
                }
            }
            finish(al, gl);
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
                        const float *gh = grow + h * DS, *qh = qrow + h * DS;
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const float a = __shfl(al[u], lane0 + h);
                            const float b = __shfl(gl[u], lane0 + h);
                            tc[u] = h == 0 ? a * gh[s[u]] : __builtin_fmaf(a, gh[s[u]], tc[u]);
                            tc[u] = __builtin_fmaf(b, qh[s[u]], tc[u]);
                        }
                    }
                }
                store_t_rows<KG, U>(trs, tc, sl.ok, base, grp, k, lb + l0);
            }
        }
        // one gl vector per edge from the group's HP lanes
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = base + u * G + grp;
            __builtin_amdgcn_raw_buffer_store_b32(
                __float_as_uint(gl[u]), zrs, hl && i < n ? (i * HP + l0) * 4 : (int)0x80000000, 0,
                0);
        }
    }
}

template <int KG, int HP, int U, bool DROP>
__global__ __launch_bounds__(kBlock) void datb_walk_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const float *__restrict__ q, float scale, const uint8_t *__restrict__ rec, int RS,
    const float *__restrict__ out, const float *__restrict__ row_max,
    const float *__restrict__ row_sum, const float *__restrict__ grad_out, float *__restrict__ T,
    float *__restrict__ glT, int num_rows, int64_t num_e, int D, int DS, int k, int chunk,
    int n_items, int H, int flags, MaskArg<DROP> dm) {
    // flags: bit 0 16-B loads of grad_out and out, bit 1 of q (D % 4 == 0, 16-B aligned)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wid = threadIdx.x / kWave;
    const int lane = lane_id();
    const int item = item_of_wave(n_items);
    if (item < 0) return;  // whole wave; no workgroup barrier below
    float *grow = lds + (size_t)wid * 2 * H * DS;
    float *qrow = grow + H * DS;
    // the pad columns [D, DS) of every staged row are never staged over: zeroed once
    for (int h = 0; h < 2 * H; ++h)
        if (lane < DS - D) grow[h * DS + D + lane] = 0.f;
    const int l0 = lane % KG;
    const bool gvec = flags & 1, qvec = flags & 2;

    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);
    // Rows r = it.r - 1 (the continuation: its token precedes the item), it.r, it.r + 1, ...:
    // each one's piece under CutAtEnd, through one walk site, so t is formed by the same
    // instructions in every item that holds a piece of a row.
    int r = it.r - 1;
    RowPiece p{0, 0, false};
    if (it.r > 0) p = cont_piece(CutAtEnd{}, it.p_lo, it.d1, it.r, row_ptr[it.r]);
    for (;;) {
        if (r >= 0 && p.sb < p.se) {
            HeadLane hd{0.f, 1.f, 0.f};
            if (l0 < H) {
                const int64_t o = (int64_t)l0 * num_rows + r;
                hd.shift = shift_of(row_max[o]);
                hd.sum = row_sum[o];
            }
            wave_lds_fence();  // the previous piece's reads of the staged rows are done
            for (int h = 0; h < H; ++h) {
                const int64_t o = ((int64_t)h * num_rows + r) * D;
                const float th = lane_tree<kWave, Sum>(
                    stage_dot(grow + h * DS, grad_out + o, out + o, D, gvec, lane));
                hd.t = l0 == h ? th : hd.t;
            }
            stage_query(qrow, q, r, num_rows, H, D, DS, scale, qvec, lane);
            wave_lds_fence();
            walk_piece_bwd<KG, HP, U, DROP>(grow, qrow, DS, col_idx, rec, RS, T, glT, H, D,
                                            (int)p.sb, (int)p.se, k, hd, lane, dm);
        }
        ++r;
        if (r >= num_rows) break;
        const int64_t rb = row_ptr[r];
        if (!row_owned(it.d1, r, rb)) break;  // row r's token belongs to a later item
        p = row_piece(CutAtEnd{}, it.d1, r, rb, row_ptr[r + 1]);
    }
}

// ---- aggregation B: grad_q[h, r, :] = scale * sum_{e in r} glT[e, h] * x_c -----------------------

// One pass over the edges [sb, se) (sb < se) of a row piece: this lane's group adds
// glT[e, head] * value into its copy acc_g for the edges base + u * EP + eg it is given (active:
// the group has an edge slot and a head in this pass; else it writes its trash column only).
template <int KG, int U>
__device__ __forceinline__ void walk_gl(float *acc_g, const int32_t *__restrict__ col_idx,
                                        const float *__restrict__ glh, int HP,
                                        const uint8_t *__restrict__ rec, int RS, int sb, int se,
                                        int k, int trash, int EP, int eg, bool active, int lane) {
    const int l0 = lane % KG;
    const int n = se - sb;  // wave-uniform, <= 2 * chunk
    const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
    const auto rrs = wave_buffer(rec, 0xffffffffu);  // offsets < num_cols * RS < 2^32
    for (int base = 0; base < n; base += EP * U) {
        int c[U];
        float w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = base + u * EP + eg;
            // past the piece's end the column reads 0 (column 0's record) and the weight is 0
            c[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(crs, i * 4, 0, 0);
            w[u] = active && i < n ? glh[((int64_t)sb + i) * HP] : 0.f;
        }
        scatter_records<KG, U>(acc_g, rrs, RS, k, trash, l0, c, w, active, base, EP, eg, n);
    }
}

// dst[0:D] = (acc[0:D] + acc[stride + 0:D] + ... over nc copies) * mul; the copies read are
// zeroed.  One wave.  (flush_head with a product in the place of the division.)
__device__ __forceinline__ void flush_scaled(float *acc, int nc, int stride,
                                             float *__restrict__ dst, int D, float mul, bool vec,
                                             bool nt, int lane) {
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
            a.x *= mul;
            a.y *= mul;
            a.z *= mul;
            a.w *= mul;
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
            dst[j] = a * mul;
        }
    }
}

template <int KG, int U>
__global__ __launch_bounds__(kBlock) void datb_gq_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const float *__restrict__ glT, int HP, const uint8_t *__restrict__ rec, int RS, float scale,
    float *__restrict__ grad_q, float *__restrict__ slab, int32_t *__restrict__ slab_row,
    int num_rows, int64_t num_e, int D, int DS, int k, int chunk, int n_items, int H, int HC,
    int flags) {
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

    // edges [sb, se) of row r, an owned row's into grad_q, a continuation's into the item's slab:
    // every head is stored, an empty piece as zeros
    walk_hub_item(row_ptr, slab_row, num_rows, num_e, item, chunk, lane,
                  [&](int r, int64_t sb, int64_t se, bool, bool owned) {
        float *__restrict__ dst = owned ? grad_q + (int64_t)r * D : slab + (int64_t)item * D;
        const int64_t hstride = (int64_t)(owned ? num_rows : n_items) * D;
        for (int h0 = 0; h0 < H; h0 += HC) {
            const int head = h0 + g.hh;
            const bool active = g.grp_ok && head < H;
            wave_lds_fence();
            if (sb < se)
                walk_gl<KG, U>(g.acc_g, col_idx, glT + (active ? head : 0), HP, rec, RS, (int)sb,
                               (int)se, k, DS - 1, g.EP, g.eg, active, lane);
            wave_lds_fence();
            for (int j = 0; j < HC && h0 + j < H; ++j)
                flush_scaled(acc + j * DS, g.EP, HC * DS, dst + (int64_t)(h0 + j) * hstride, D,
                             scale, vec, nt && owned, lane);
        }
        wave_lds_fence();
    });
}

// ---- host ---------------------------------------------------------------------------------------

// Resident waves per CU the items are sized for: walk A four per SIMD by VGPRs, B seven (the
// multi-head forward's), fewer where the staged rows or the copies fill the LDS first.
constexpr int kWalkResident = 16;
constexpr int kGqResident = 28;

// Workspace: [T (num_e + 1 rows) and the phase-2 slabs | records | glT | B's slabs | slab_row].
struct DotBwdLayout {
    RecordGeom R;
    int hp, chunk, n_items;    // walk A
    int hc, bchunk, bn_items;  // aggregation B
    size_t lds_a, lds_b;       // per workgroup
    size_t rec_off, gl_off, total;
    SlabLayout S;
};

DotBwdLayout bwd_layout(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k, int H,
                        int chunk) {
    DotBwdLayout L{};
    L.R = record_geom(num_cols, D, k);
    L.hp = hp_of(H);
    L.lds_a = (size_t)kWavesPerBlock * 2 * H * L.R.DS * sizeof(float);
    L.chunk = walk_chunk(num_rows, num_e, chunk, L.lds_a, kWalkResident, kBwdMaxChunk);
    L.n_items = token_items(num_rows, num_e, L.chunk);
    L.hc = heads_per_pass(H, L.R.kg);
    L.lds_b = (size_t)kWavesPerBlock * (kWave / L.R.kg) * L.R.DS * sizeof(float);
    L.bchunk = walk_chunk(num_rows, num_e, chunk, L.lds_b, kGqResident);
    L.bn_items = token_items(num_rows, num_e, L.bchunk);
    L.rec_off = csc_sum_workspace_size(num_cols, num_e, k, chunk);
    L.gl_off = L.rec_off + al256((size_t)num_cols * L.R.RS);
    L.S = slab_layout(item_cap(num_rows + num_e, chunk, L.bn_items), H, D,
                      L.gl_off + al256((size_t)num_e * L.hp * sizeof(float)), false);
    L.total = L.S.end;
    return L;
}

template <int HP, bool DROP>
int launch_dot_bwd(const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr,
                   const int32_t *csc_eid, const float *q, float scale, const float *cbsr_val,
                   const uint8_t *cbsr_idx, const float *out, const float *row_max,
                   const float *row_sum, const float *grad_out, float *grad_q, float *grad_cbsr,
                   int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k, int H,
                   int chunk_edges, const DotBwdLayout &L, void *workspace, hipStream_t s,
                   const MaskArg<DROP> &dm) {
    const RecordGeom &R = L.R;
    char *ws = reinterpret_cast<char *>(workspace);
    float *T = reinterpret_cast<float *>(ws);
    uint8_t *rec = reinterpret_cast<uint8_t *>(ws + L.rec_off);
    float *glT = reinterpret_cast<float *>(ws + L.gl_off);
    float *slab = reinterpret_cast<float *>(ws + L.S.slab_off);
    int32_t *slab_row = reinterpret_cast<int32_t *>(ws + L.S.row_off);
    if (int rc = launch_cbsr_pack(cbsr_val, cbsr_idx, rec, num_cols, k, R.RS, D, R.DS - 1, s))
        return rc;
    const int aflags =
        (D % 4 == 0 && ((uintptr_t)grad_out & 15) == 0 && ((uintptr_t)out & 15) == 0 ? 1 : 0) |
        (D % 4 == 0 && ((uintptr_t)q & 15) == 0 ? 2 : 0);
    bool ok = with_const<8, 16, 32, 64>(R.kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        hipLaunchKernelGGL((datb_walk_kernel<KG, HP, MAXK_DATB_U, DROP>), item_grid(L.n_items),
                           dim3(kBlock), L.lds_a, s, row_ptr, col_idx, q, scale, rec, R.RS, out,
                           row_max, row_sum, grad_out, T, glT, (int)num_rows, num_e, D, R.DS, k,
                           L.chunk, L.n_items, H, aflags, dm);
    });
    if (!ok) return bad_lanes(R.kg);
    MAXK_LAUNCHED("datb_walk_kernel");
    const int bflags = store_flags(grad_q, H, num_rows, D);
    ok = with_const<8, 16, 32, 64>(R.kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        hipLaunchKernelGGL((datb_gq_kernel<KG, MAXK_FWD_U>), item_grid(L.bn_items), dim3(kBlock),
                           L.lds_b, s, row_ptr, col_idx, glT, HP, rec, R.RS, scale, grad_q, slab,
                           slab_row, (int)num_rows, num_e, D, R.DS, k, L.bchunk, L.bn_items, H,
                           L.hc, bflags);
    });
    if (!ok) return bad_lanes(R.kg);
    MAXK_LAUNCHED("datb_gq_kernel");
    for (int h = 0; h < H; ++h)  // gl is final: a hub row's pieces are added in item order
        if (int rc = launch_slab_fixup<0>(slab + (size_t)h * L.bn_items * D, slab_row,
                                          grad_q + (size_t)h * num_rows * D, D, L.bn_items, s))
            return rc;
    return csc_sum_rows(s, col_ptr, csc_eid, ws, grad_cbsr, num_cols, num_e, k, chunk_edges);
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" size_t maxk_dot_attention_heads_backward_workspace_size(
    int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
    int32_t num_heads, int32_t chunk_edges) {
    if (!dot_shape_ok(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads, chunk_edges))
        return 0;
    return bwd_layout(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads, chunk_edges).total;
}

namespace {
// Both backward entries; dm: the dropout entry's mask, null for none.
int dot_attention_heads_backward(
    const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr, const int32_t *csc_eid,
    const float *q, float scale, const float *cbsr_val, const uint8_t *cbsr_idx, const float *out,
    const float *row_max, const float *row_sum, const float *grad_out, float *grad_q,
    float *grad_cbsr, int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin,
    int32_t dim_k, int32_t num_heads, int32_t chunk_edges, void *workspace,
    size_t workspace_bytes, void *stream, const DropMask *dm) {
    if (int rc = check_dot(num_rows, num_cols, num_e, scale, dim_origin, dim_k, num_heads,
                           chunk_edges))
        return rc;
    MAXK_REQUIRE((grad_q || num_rows == 0) && (grad_cbsr || num_cols == 0),
                 "grad_q / grad_cbsr must not be NULL");
    const int D = dim_origin, k = dim_k, H = num_heads;
    hipStream_t s = as_stream(stream);
    if (num_e == 0) {  // nothing to walk: both gradients are zeros
        if (num_rows > 0)
            if (int rc = zero_words(grad_q, (int64_t)H * num_rows * D, s)) return rc;
        return num_cols > 0 ? zero_words(grad_cbsr, num_cols * k, s) : MAXK_OK;
    }
    MAXK_REQUIRE(num_rows > 0 && num_cols > 0, "edges present but num_rows or num_cols == 0");
    MAXK_REQUIRE(row_ptr && col_idx && col_ptr && csc_eid,
                 "row_ptr / col_idx / col_ptr / csc_eid must not be NULL");
    MAXK_REQUIRE(q && cbsr_val && cbsr_idx, "q / cbsr_val / cbsr_idx must not be NULL");
    MAXK_REQUIRE(out && row_max && row_sum && grad_out,
                 "out / row_max / row_sum / grad_out must not be NULL");
    const DotBwdLayout L = bwd_layout(num_rows, num_cols, num_e, D, k, H, chunk_edges);
    MAXK_REQUIRE(!L.R.wide, "num_cols: the fused dot-product attention backward takes tables below "
                 "2^24 columns and 4 GiB of records (%lld columns of %d bytes)",
                 (long long)num_cols, L.R.RS);
    if (int rc = check_workspace(workspace, workspace_bytes, L.total)) return rc;
    MAXK_REQUIRE(((uintptr_t)cbsr_val & 3) == 0 && ((uintptr_t)q & 3) == 0 &&
                     ((uintptr_t)out & 3) == 0 && ((uintptr_t)row_max & 3) == 0 &&
                     ((uintptr_t)row_sum & 3) == 0 && ((uintptr_t)grad_out & 3) == 0 &&
                     ((uintptr_t)grad_q & 3) == 0 && ((uintptr_t)grad_cbsr & 3) == 0,
                 "float buffers must be 4-B aligned");
    return with_heads_mask(L.hp, dm, [&](auto hp_c, const auto &mask) {
        return launch_dot_bwd<decltype(hp_c)::value, is_drop_v<decltype(mask)>>(
            row_ptr, col_idx, col_ptr, csc_eid, q, scale, cbsr_val, cbsr_idx, out, row_max, row_sum,
            grad_out, grad_q, grad_cbsr, num_rows, num_cols, num_e, D, k, H, chunk_edges, L,
            workspace, s, mask);
    });
}
}  // namespace

extern "C" int maxk_dot_attention_heads_backward(
    const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr, const int32_t *csc_eid,
    const float *q, float scale, const float *cbsr_val, const uint8_t *cbsr_idx, const float *out,
    const float *row_max, const float *row_sum, const float *grad_out, float *grad_q,
    float *grad_cbsr, int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin,
    int32_t dim_k, int32_t num_heads, int32_t chunk_edges, void *workspace,
    size_t workspace_bytes, void *stream) {
    clear_error();
    return dot_attention_heads_backward(row_ptr, col_idx, col_ptr, csc_eid, q, scale, cbsr_val,
                                        cbsr_idx, out, row_max, row_sum, grad_out, grad_q,
                                        grad_cbsr, num_rows, num_cols, num_e, dim_origin, dim_k,
                                        num_heads, chunk_edges, workspace, workspace_bytes, stream,
                                        nullptr);
}

extern "C" size_t maxk_dot_attention_heads_dropout_backward_workspace_size(
    int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
    int32_t num_heads, int32_t chunk_edges) {
    return maxk_dot_attention_heads_backward_workspace_size(num_rows, num_cols, num_e, dim_origin,
                                                            dim_k, num_heads, chunk_edges);
}

extern "C" int maxk_dot_attention_heads_dropout_backward(
    const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr, const int32_t *csc_eid,
    const float *q, float scale, const float *cbsr_val, const uint8_t *cbsr_idx, const float *out,
    const float *row_max, const float *row_sum, const float *grad_out, float *grad_q,
    float *grad_cbsr, int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin,
    int32_t dim_k, int32_t num_heads, int32_t chunk_edges, float p, uint64_t seed,
    void *workspace, size_t workspace_bytes, void *stream) {
    clear_error();
    return with_dropout(p, seed, [&](const DropMask *dm) {
        return dot_attention_heads_backward(row_ptr, col_idx, col_ptr, csc_eid, q, scale, cbsr_val,
                                            cbsr_idx, out, row_max, row_sum, grad_out, grad_q,
                                            grad_cbsr, num_rows, num_cols, num_e, dim_origin,
                                            dim_k, num_heads, chunk_edges, workspace,
                                            workspace_bytes, stream, dm);
    });
}
