// The staged-row walks, stated once for the units that run them: the
// edge-weight gradient (edge_grad.hip), the alpha entry of the dot-product attention
// (dot_attention_heads.hip, through dot_logit.h) and the two fused attention backwards
// (gat_attention_heads_bwd.hip, dot_attention_heads_bwd.hip).
//
// One wavefront per item of the token stream under CutAtEnd (token_items.h; walk_cut_item is the
// item driver, and the kernels that spill scalar registers keep its loop written out): every
// edge's result is independent of the other edges of its row, so a row cut over items needs no
// slab -- each item stages the row again.  Per row piece the dense rows the edges are multiplied
// with (grad_out, the scaled query; H of them side by side for H heads) are staged in the wave's
// LDS, DS floats each, the pad columns [D, DS) zero, so a skipped selector reads 0 even beside a
// NaN.  Per edge KG = pow2ceil(k) lanes (>= 8, <= 64) read one packed record (RecordSlot,
// cbsr_pack.h), G = 64 / KG edges per wave step, U steps in flight; past the piece's end col_idx
// reads 0 (column 0's record) and nothing is stored.  k > 64: a lane takes its slots l0,
// l0 + KG, ... in l order, the record reloaded from the caches.  Every sum over a group is the
// fixed butterfly lane_tree: the same order every run, the same bits in every lane of the group.
// Here: stage_row / stage_dot (the staging), dot_term / record_dots (a record's dot product with
// a staged row), store_staged (a batch's results as one coalesced store), caller_columns (the
// caller's selectors and the keep bits), store_t_rows (the contribution rows) and kBwdMaxChunk.
// What each unit multiplies and sums between these steps is its own.
// Device code in an anonymous namespace (each translation unit instantiates what it launches),
// host code plain inline.
#pragma once

#include "cbsr_pack.h"
#include "edge_softmax.h"  // lane_tree
#include "heads_walk.h"    // walk_chunk

namespace maxk {
namespace {

// grow[0:D] = g[0:D] (grow's pad columns [D, DS) already hold zeros).  One wave.
__device__ __forceinline__ void stage_row(float *grow, const float *__restrict__ g, int D, bool vec,
                                          int lane) {
    if (vec) {
        for (int j = lane * 4; j < D; j += kWave * 4)
            *reinterpret_cast<float4 *>(&grow[j]) = *reinterpret_cast<const float4 *>(&g[j]);
    } else {
        for (int j = lane; j < D; j += kWave) grow[j] = g[j];
    }
}

// grow[0:D] = g[0:D]; returns this lane's part of sum_{j : o[j] != 0} o[j] * g[j].  One wave.
__device__ __forceinline__ float stage_dot(float *grow, const float *__restrict__ g,
                                           const float *__restrict__ o, int D, bool vec,
                                           int lane) {
    float t = 0.f;
    if (vec) {
        for (int j = lane * 4; j < D; j += kWave * 4) {
            const float4 gv = *reinterpret_cast<const float4 *>(&g[j]);
            const float4 ov = *reinterpret_cast<const float4 *>(&o[j]);
            *reinterpret_cast<float4 *>(&grow[j]) = gv;
            t = ov.x != 0.f ? __builtin_fmaf(ov.x, gv.x, t) : t;
            t = ov.y != 0.f ? __builtin_fmaf(ov.y, gv.y, t) : t;
            t = ov.z != 0.f ? __builtin_fmaf(ov.z, gv.z, t) : t;
            t = ov.w != 0.f ? __builtin_fmaf(ov.w, gv.w, t) : t;
        }
    } else {
        for (int j = lane; j < D; j += kWave) {
            const float gv = g[j], ov = o[j];
            grow[j] = gv;
            t = ov != 0.f ? __builtin_fmaf(ov, gv, t) : t;
        }
    }
    return t;
}

// One slot of an edge's dot product against a staged row: an idle lane's clamped slot (!ok)
// contributes nothing.  A folded or skipped selector carries the value 0 and reads a zero pad.
__device__ __forceinline__ float dot_term(float v, int s, const float *row, int trash, bool ok,
                                          float acc) {
    const float t = __builtin_fmaf(v, row[min(s, trash)], acc);
    return ok ? t : acc;
}
// k > KG (k > 64): d[u] = the dot product of column c[u]'s record and the staged row; a lane takes
// its slots l0, l0 + KG, ... in l order, the group's lanes are summed by lane_tree.
template <int KG, int U>
__device__ __forceinline__ void record_dots(const __amdgpu_buffer_rsrc_t rrs, int RS,
                                            const int (&c)[U], const float *row, int k, int trash,
                                            int l0, float (&d)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) d[u] = 0.f;
    for (int lb = 0; lb < k; lb += KG) {
        const RecordSlot sl(lb + l0, k);
        const PackedSrc src = sl.src(rrs, k, RS);
        float v[U];
        int s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) src.load(c[u], v[u], s[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) d[u] = dot_term(v[u], s[u], row, trash, sl.ok, d[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) d[u] = lane_tree<KG, Sum>(d[u]);
}

// A batch's G * U results leave through the wave's 64 staging floats as one coalesced store in
// edge order: behind a wave_lds_fence the first lane of group grp has written the result of its
// edge base + u * G + grp to stage[u * G + grp]; ors: the piece's results.  Past the piece's end
// (and from the lanes past the batch) the offset is out of the descriptor's range: dropped.
template <int KG, int U>
__device__ __forceinline__ void store_staged(const float *stage, const __amdgpu_buffer_rsrc_t ors,
                                             int base, int lane) {
    constexpr int G = kWave / KG;
    wave_lds_fence();
    const int e = base + lane;
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(stage[lane % (G * U)]), ors,
                                          lane < G * U ? e * 4 : (int)0x80000000, 0, 0);
}

// The record's low selector byte is the caller's selector, so a repeated selector's slot receives
// its gradient although the pack folded its value.  Turns the loaded selectors s[u] into the
// caller's staged columns, the trash column (a zero pad) for a selector >= D.  Returns bit u:
// slot u carries a (folded) value under a selector < D (ok: the record has the slot).
template <int U>
__device__ __forceinline__ uint32_t caller_columns(int (&s)[U], bool ok, int D, int trash) {
    uint32_t keep = 0u;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        keep |= (ok && s[u] < 0x100 ? 1u : 0u) << u;
        const int raw = s[u] & 255;
        s[u] = raw < D ? raw : trash;
    }
    return keep;
}

// Slot l of the contribution rows T[e, 0:k] of the group's U edges base + u * G + grp; trs: the
// piece's rows.  Idle lanes (!ok) and edges past the piece's end: the offset is out of the
// descriptor's range, dropped.
template <int KG, int U>
__device__ __forceinline__ void store_t_rows(const __amdgpu_buffer_rsrc_t trs, const float (&tc)[U],
                                             bool ok, int base, int grp, int k, int l) {
    constexpr int G = kWave / KG;
#pragma unroll
    for (int u = 0; u < U; ++u)
        __builtin_amdgcn_raw_buffer_store_b32(
            __float_as_uint(tc[u]), trs,
            ok ? ((base + u * G + grp) * k + l) * 4 : (int)0x80000000, 0, MAXK_T_AUX);
}

}  // namespace

// ---- host ---------------------------------------------------------------------------------------

// A backward piece's T rows are addressed through a descriptor of 4 * k * n bytes with 32-bit
// offsets: the cap of walk_chunk for the walks that store them.
constexpr int kBwdMaxChunk = 1 << 20;

}  // namespace maxk
