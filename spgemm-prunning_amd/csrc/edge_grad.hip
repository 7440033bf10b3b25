// Gradient of the aggregation with respect to the edge weights, for gfx950: an SDDMM sampled
// by the CBSR,
//
//   grad_edge[e] = ( sum_l cbsr_val[c, l] * G[r, cbsr_idx[c, l]] ) / row_div[r]
//                  r = the CSR row holding e, c = col_idx[e]
//
// the adjoint of out = diag(1/row_div) . A . scatter(cbsr) in A's values.  It shares the
// forward's gather -- one packed record [k f32 | k u16 | pad] per edge (cbsr_pack.h), so an edge
// costs one line -- and its token-stream partition (token_items.h), and nothing else:
//
//  1. launch_cbsr_pack writes this call's records into the workspace.  The pack folds repeated
//     selectors into their first occurrence and sends selectors >= D to the trash column with
//     value 0, so every term of an edge's dot product is either a kept (value, column < D) pair
//     or exactly 0 * 0.
//  2. edge_grad_kernel, one wavefront per item of `chunk` tokens, cut at the item's end
//     (CutAtEnd): every edge's result is independent, so a hub row cut over items needs no
//     slab and no fix-up -- each item stages the row again.
//     * per row piece: G[r, :] staged once into the wave's LDS row (16-B loads where D % 4 == 0
//       and grad_out is 16-B aligned, else scalar); the pad columns [D, DS) hold zeros, so a
//       skipped selector reads 0 even beside a NaN in G;
//     * per edge: KG = pow2ceil(k) lanes (>= 8, <= 64), G = 64 / KG edges per wave step, U steps
//       in flight; lane l loads its value and selector through a buffer descriptor
//       (unconditional: past the piece's end col_idx reads 0, column 0's record, and the result
//       is not stored), reads G[sel] from LDS and multiplies; for k > 64 a lane accumulates its
//       slots l, l + 64, ... in l order with one fma each; idle lanes (l >= k) contribute 0;
//     * a fixed cross-lane tree (DPP quad permutes and mirrors within 16 lanes, ds_swizzle for
//       the 32-lane step, v_permlane32_swap for the last) sums the group: same order every run;
//     * the finished dot product is divided by row_div[r] once; a batch's G * U results go
//       through 64 floats of LDS per wave and leave as one coalesced store in CSR order.
//       (Lane 0 of each group storing its own result, G consecutive floats per instruction and
//       U instructions per batch, measured 1.752 against 1.653 ms Reddit-sized at k = 16 and
//       5.06 against 5.00 ms products-sized at k = 32, the latter inside the run-to-run
//       spread: MAXK_EGRAD_LDS_STORE=0, profiles/r07/edge_grad/.)
// No atomics, no allocation, copy or synchronisation: the launch can be captured.
// The item driver is token_items.h's walk_cut_item; the staging, the group sum (lane_tree) and the
// staged store are piece_walk.h's, shared with the attention backwards and the dot-product alpha.
#include "piece_walk.h"

#ifndef MAXK_EGRAD_U  // edge-gradient: wave steps of record loads in flight
#define MAXK_EGRAD_U 8
#endif
#ifndef MAXK_EGRAD_LDS_STORE  // 1: a batch's results staged in LDS and stored as one coalesced
#define MAXK_EGRAD_LDS_STORE 1  // run; 0: lane 0 of each group stores its own
#endif

namespace maxk {
namespace {

// grad_edge[e] = dot(record of col_idx[e], grow) / div over e in [sb, se), sb < se: a piece of
// one row whose G row is staged in grow.  WIDE (tables past 2^24 columns or 4 GiB): 64-bit
// record addresses and clamped loads instead of the buffer descriptors.
template <int KG, int U, bool WIDE>
__device__ __forceinline__ void walk_piece(const float *grow, float *stage,
                                           const int32_t *__restrict__ col_idx,
                                           const uint8_t *__restrict__ rec, int RS,
                                           float *__restrict__ grad_edge, int sb, int se, int k,
                                           int trash, float div, bool scale, int lane) {
    constexpr int G = kWave / KG;
    const int grp = lane / KG, l0 = lane % KG;
    const int n = se - sb;  // wave-uniform, <= chunk
    const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
    const auto ors = wave_buffer(grad_edge + sb, (uint32_t)n * 4u);
    const auto rrs = wave_buffer(rec, WIDE ? 0u : 0xffffffffu);
    for (int base = 0; base < n; base += G * U) {
        int c[U];
        float acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            c[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(crs, (base + u * G + grp) * 4, 0, 0);
            acc[u] = 0.f;
        }
        for (int lb = 0; lb < k; lb += KG) {  // one pass unless k > 64
            const RecordSlot sl(lb + l0, k);
            float v[U];
            int s[U];
            if constexpr (!WIDE) {
                const PackedSrc src = sl.src(rrs, k, RS);
#pragma unroll
                for (int u = 0; u < U; ++u) src.load(c[u], v[u], s[u]);
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint8_t *p = rec + (size_t)(uint32_t)c[u] * RS;
                    v[u] = reinterpret_cast<const float *>(p)[sl.lc];
                    s[u] = reinterpret_cast<const uint16_t *>(p + 4 * k)[sl.lc];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float t = __builtin_fmaf(v[u], grow[min(s[u], trash)], acc[u]);
                acc[u] = sl.ok ? t : acc[u];  // an idle lane's clamped slot contributes nothing
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float x = lane_tree<KG, Sum>(acc[u]);
            acc[u] = scale ? x / div : x;
        }
        if constexpr (MAXK_EGRAD_LDS_STORE) {
            // the batch's G * U results in edge order, one coalesced store of the run
            wave_lds_fence();
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (l0 == 0) stage[u * G + grp] = acc[u];
            store_staged<KG, U>(stage, ors, base, lane);
        } else {
            // lane 0 of each group: G consecutive floats per instruction; past the piece's end
            // (and from the other lanes) the offset is out of the descriptor's range: dropped
#pragma unroll
            for (int u = 0; u < U; ++u)
                __builtin_amdgcn_raw_buffer_store_b32(
                    __float_as_uint(acc[u]), ors,
                    l0 == 0 ? (base + u * G + grp) * 4 : (int)0x80000000, 0, 0);
        }
    }
}

template <int KG, int U, bool WIDE>
__global__ __launch_bounds__(kBlock) void edge_grad_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const uint8_t *__restrict__ rec, int RS, const float *__restrict__ grad_out,
    const float *__restrict__ row_div, float *__restrict__ grad_edge, int num_rows, int64_t num_e,
    int D, int DS, int k, int chunk, int n_items, int vec) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int kStage = MAXK_EGRAD_LDS_STORE ? kWave : 0;
    const int wid = threadIdx.x / kWave;
    const int lane = lane_id();
    const int blk = MAXK_FWD_XCD ? xcd_contiguous_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int item = blk * kWavesPerBlock + wid;
    if (item >= n_items) return;  // whole wave; no workgroup barrier below
    float *grow = lds + (size_t)wid * (DS + kStage);
    float *stage = grow + DS;
    // the pad columns [D, DS) are never staged over: zeroed once (DS - D <= 7)
    if (lane < DS - D) grow[D + lane] = 0.f;

    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);

    // the edges whose tokens lie in [d0, d1), row piece by row piece
    walk_cut_item(row_ptr, num_rows, it, [&](int q, int64_t sb, int64_t se, int64_t, bool) {
        if (sb >= se) return;
        const float div = row_div ? row_div[q] : 1.f;  // loaded before the walk
        wave_lds_fence();  // the previous piece's reads of grow are done
        stage_row(grow, grad_out + (int64_t)q * D, D, vec != 0, lane);
        wave_lds_fence();
        walk_piece<KG, U, WIDE>(grow, stage, col_idx, rec, RS, grad_edge, (int)sb, (int)se, k,
                                DS - 1, div, row_div != nullptr, lane);
    });
}

// ---- H heads (maxk_edge_weight_grad_heads): grad_out [H, num_rows, D], grad_edge [H, num_e] ----
// The walk above with one record load per edge serving every head: per row piece the H rows
// G[h, r, :] are staged side by side (grow[h * DS + j]: H * DS floats per wave, 8.3 KB at H = 8,
// D = 256); per edge the lane's value and selector are loaded once and each head takes one fma
// against its staged row and the same fixed-shape lane_tree, so head h's result is, bitwise,
// what the single-head kernel gives for G[h] (H = 1: the same kernel in effect).  For k > 64
// (several slots per lane) the passes over l run per head and the record is loaded again from
// the caches.  A batch's results leave per head through the wave's 64 staging floats as one
// coalesced store.
template <int KG, int U>
__device__ __forceinline__ void walk_piece_heads(const float *grow, float *stage,
                                                 const int32_t *__restrict__ col_idx,
                                                 const uint8_t *__restrict__ rec, int RS,
                                                 float *__restrict__ grad_edge, int64_t num_e,
                                                 int H, int DS, int sb, int se, int k, int trash,
                                                 float div, bool scale, int lane) {
    constexpr int G = kWave / KG;
    const int grp = lane / KG, l0 = lane % KG;
    const int n = se - sb;  // wave-uniform, <= chunk
    const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
    const auto rrs = wave_buffer(rec, 0xffffffffu);
    // head h's sums of the batch at `base`: scaled, staged in edge order, one store
    auto leave = [&](int h, int base, float (&x)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = scale ? x[u] / div : x[u];
        const auto ors = wave_buffer(grad_edge + (int64_t)h * num_e + sb, (uint32_t)n * 4u);
        wave_lds_fence();
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (l0 == 0) stage[u * G + grp] = x[u];
        store_staged<KG, U>(stage, ors, base, lane);
    };
    for (int base = 0; base < n; base += G * U) {
        int c[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            c[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(crs, (base + u * G + grp) * 4, 0, 0);
        if (k <= KG) {  // one slot per lane: the record is loaded once for all heads
            const RecordSlot sl(l0, k);
            const PackedSrc src = sl.src(rrs, k, RS);
            float v[U];
            int s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                src.load(c[u], v[u], s[u]);
                s[u] = min(s[u], trash);
            }
            for (int h = 0; h < H; ++h) {
                const float *gh = grow + h * DS;
                float acc[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float t = __builtin_fmaf(v[u], gh[s[u]], 0.f);
                    // an idle lane's clamped slot contributes nothing
                    acc[u] = lane_tree<KG, Sum>(sl.ok ? t : 0.f);
                }
                leave(h, base, acc);
            }
        } else {
            for (int h = 0; h < H; ++h) {
                float acc[U];
                record_dots<KG, U>(rrs, RS, c, grow + h * DS, k, trash, l0, acc);
                leave(h, base, acc);
            }
        }
    }
}

template <int KG, int U>
__global__ __launch_bounds__(kBlock) void edge_grad_heads_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const uint8_t *__restrict__ rec, int RS, const float *__restrict__ grad_out,
    const float *__restrict__ row_div, float *__restrict__ grad_edge, int num_rows, int64_t num_e,
    int D, int DS, int k, int chunk, int n_items, int H, int vec) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wid = threadIdx.x / kWave;
    const int lane = lane_id();
    const int blk = MAXK_FWD_XCD ? xcd_contiguous_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int item = blk * kWavesPerBlock + wid;
    if (item >= n_items) return;  // whole wave; no workgroup barrier below
    float *grow = lds + (size_t)wid * (H * DS + kWave);
    float *stage = grow + H * DS;
    // the pad columns [D, DS) of every head's row are never staged over: zeroed once
    for (int h = 0; h < H; ++h)
        if (lane < DS - D) grow[h * DS + D + lane] = 0.f;

    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);
    walk_cut_item(row_ptr, num_rows, it, [&](int q, int64_t sb, int64_t se, int64_t, bool) {
        if (sb >= se) return;
        const float div = row_div ? row_div[q] : 1.f;  // loaded before the walk
        wave_lds_fence();  // the previous piece's reads of grow are done
        for (int h = 0; h < H; ++h)
            stage_row(grow + h * DS, grad_out + ((int64_t)h * num_rows + q) * D, D, vec != 0,
                      lane);
        wave_lds_fence();
        walk_piece_heads<KG, U>(grow, stage, col_idx, rec, RS, grad_edge, num_e, H, DS, (int)sb,
                                (int)se, k, DS - 1, div, row_div != nullptr, lane);
    });
}

// Waves one CU holds at once: 8 per SIMD by VGPRs (at most 64, the kernel-resource-usage
// remarks); the LDS row per wave (about 1 KB) is far from the CU's 160 KB.
constexpr int kEdgeGradResident = 32;

struct EdgeGradLayout : RecordGeom {
    int chunk, n_items;
    size_t total;
};

EdgeGradLayout edge_grad_layout(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k,
                                int chunk) {
    EdgeGradLayout L{record_geom(num_cols, D, k)};
    L.chunk = fwd_chunk(num_rows, num_e, chunk, kEdgeGradResident);
    if (L.chunk > kMaxChunk) L.chunk = kMaxChunk;
    L.n_items = token_items(num_rows, num_e, L.chunk);
    L.total = al256((size_t)num_cols * L.RS);
    return L;
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" size_t maxk_edge_weight_grad_workspace_size(int64_t num_rows, int64_t num_cols,
                                                       int64_t num_e, int32_t dim_origin,
                                                       int32_t dim_k, int32_t chunk_edges) {
    if (num_rows < 0 || num_cols < 0 || num_e < 0 || dim_origin <= 0 || dim_k <= 0) return 0;
    const size_t n =
        edge_grad_layout(num_rows, num_cols, num_e, dim_origin, dim_k, chunk_edges).total;
    return n ? n : 256;  // never empty: one query serves any num_cols
}

extern "C" int maxk_edge_weight_grad(const int32_t *row_ptr, const int32_t *col_idx,
                                     const float *cbsr_val, const uint8_t *cbsr_idx,
                                     const float *grad_out, const float *row_div,
                                     float *grad_edge, int64_t num_rows, int64_t num_cols,
                                     int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                     int32_t chunk_edges, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    clear_error();
    MAXK_REQUIRE(num_rows >= 0 && num_rows < (1LL << 31), "num_rows out of range: %lld",
                 (long long)num_rows);
    MAXK_REQUIRE(num_cols >= 0 && num_cols < (1LL << 31), "num_cols out of range");
    MAXK_REQUIRE(num_e >= 0 && num_e < (1LL << 31), "num_e out of range: %lld", (long long)num_e);
    MAXK_REQUIRE(dim_origin >= 1 && dim_origin <= kMaxDim, "dim_origin must be in [1,256], got %d",
                 dim_origin);
    MAXK_REQUIRE(dim_k >= 1 && dim_k <= dim_origin, "dim_k must be in [1,dim_origin], got %d",
                 dim_k);
    MAXK_REQUIRE(chunk_edges >= 0, "chunk_edges must be >= 0");
    MAXK_REQUIRE(num_cols * (int64_t)dim_k < (1LL << 31), "num_cols*k too large");
    if (num_e == 0) return MAXK_OK;  // no edge, nothing to write
    MAXK_REQUIRE(num_rows > 0 && num_cols > 0, "edges present but num_rows or num_cols == 0");
    MAXK_REQUIRE(row_ptr && col_idx && cbsr_val && cbsr_idx && grad_out && grad_edge,
                 "CSR / CBSR / grad_out / grad_edge pointers must not be NULL");
    const EdgeGradLayout L =
        edge_grad_layout(num_rows, num_cols, num_e, dim_origin, dim_k, chunk_edges);
    MAXK_REQUIRE(workspace && workspace_bytes >= L.total,
                 "workspace too small: need %zu bytes, got %zu", L.total, workspace_bytes);
    MAXK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-B aligned");
    MAXK_REQUIRE(((uintptr_t)cbsr_val & 3) == 0 && ((uintptr_t)grad_out & 3) == 0 &&
                     ((uintptr_t)grad_edge & 3) == 0,
                 "float buffers must be 4-B aligned");

    hipStream_t s = as_stream(stream);
    const int D = dim_origin, k = dim_k;
    uint8_t *rec = reinterpret_cast<uint8_t *>(workspace);
    if (int rc = launch_cbsr_pack(cbsr_val, cbsr_idx, rec, num_cols, k, L.RS, D, L.DS - 1, s))
        return rc;
    constexpr int U = MAXK_EGRAD_U;
    const size_t lds =
        (size_t)kWavesPerBlock * (L.DS + (MAXK_EGRAD_LDS_STORE ? kWave : 0)) * sizeof(float);
    const int64_t blocks = ceil_div(L.n_items, kWavesPerBlock);
    const dim3 grid((unsigned)(MAXK_FWD_XCD ? xcd_grid(blocks) : blocks));
    const int vec = D % 4 == 0 && ((uintptr_t)grad_out & 15) == 0;
    const bool ok = with_const<8, 16, 32, 64>(L.kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        if (L.wide)
            hipLaunchKernelGGL((edge_grad_kernel<KG, U, true>), grid, dim3(kBlock), lds, s, row_ptr,
                               col_idx, rec, L.RS, grad_out, row_div, grad_edge, (int)num_rows,
                               num_e, D, L.DS, k, L.chunk, L.n_items, vec);
        else
            hipLaunchKernelGGL((edge_grad_kernel<KG, U, false>), grid, dim3(kBlock), lds, s,
                               row_ptr, col_idx, rec, L.RS, grad_out, row_div, grad_edge,
                               (int)num_rows, num_e, D, L.DS, k, L.chunk, L.n_items, vec);
    });
    if (!ok) return bad_lanes(L.kg);
    MAXK_LAUNCHED("edge_grad_kernel");
    return MAXK_OK;
}

namespace {
// The heads walk stages H rows per wave: the items are sized for the waves a CU then holds: 7
// per SIMD by VGPRs (69, no scratch: the kernel-resource-usage remarks), fewer where the LDS
// fills first (16 at H = 8, D = 256: four 34-KB workgroups in the 160 KB).
constexpr int kEdgeGradHeadsResident = 28;
EdgeGradLayout edge_grad_heads_layout(int64_t num_rows, int64_t num_cols, int64_t num_e, int D,
                                      int k, int H, int chunk) {
    EdgeGradLayout L = edge_grad_layout(num_rows, num_cols, num_e, D, k, chunk);
    const size_t per_block = (size_t)kWavesPerBlock * (H * L.DS + kWave) * sizeof(float);
    L.chunk = walk_chunk(num_rows, num_e, chunk, per_block, kEdgeGradHeadsResident);
    L.n_items = token_items(num_rows, num_e, L.chunk);
    return L;
}
}  // namespace

extern "C" size_t maxk_edge_weight_grad_heads_workspace_size(int64_t num_rows, int64_t num_cols,
                                                             int64_t num_e, int32_t dim_origin,
                                                             int32_t dim_k, int32_t num_heads,
                                                             int32_t chunk_edges) {
    if (num_rows < 0 || num_cols < 0 || num_e < 0 || dim_origin <= 0 || dim_k <= 0 ||
        num_heads < 1 || num_heads > MAXK_MAX_HEADS)
        return 0;
    const size_t n = edge_grad_heads_layout(num_rows, num_cols, num_e, dim_origin, dim_k,
                                            num_heads, chunk_edges).total;
    return n ? n : 256;  // never empty: one query serves any num_cols
}

extern "C" int maxk_edge_weight_grad_heads(const int32_t *row_ptr, const int32_t *col_idx,
                                           const float *cbsr_val, const uint8_t *cbsr_idx,
                                           const float *grad_out, const float *row_div,
                                           float *grad_edge, int64_t num_rows, int64_t num_cols,
                                           int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                           int32_t num_heads, int32_t chunk_edges, void *workspace,
                                           size_t workspace_bytes, void *stream) {
    clear_error();
    MAXK_REQUIRE(num_rows >= 0 && num_rows < (1LL << 31), "num_rows out of range: %lld",
                 (long long)num_rows);
    MAXK_REQUIRE(num_cols >= 0 && num_cols < (1LL << 31), "num_cols out of range");
    MAXK_REQUIRE(num_e >= 0 && num_e < (1LL << 31), "num_e out of range: %lld", (long long)num_e);
    MAXK_REQUIRE(dim_origin >= 1 && dim_origin <= kMaxDim, "dim_origin must be in [1,256], got %d",
                 dim_origin);
    MAXK_REQUIRE(dim_k >= 1 && dim_k <= dim_origin, "dim_k must be in [1,dim_origin], got %d",
                 dim_k);
    MAXK_REQUIRE(num_heads >= 1 && num_heads <= MAXK_MAX_HEADS,
                 "num_heads must be in [1,%d], got %d", MAXK_MAX_HEADS, num_heads);
    MAXK_REQUIRE(chunk_edges >= 0, "chunk_edges must be >= 0");
    MAXK_REQUIRE(num_cols * (int64_t)dim_k < (1LL << 31), "num_cols*k too large");
    if (num_e == 0) return MAXK_OK;  // no edge, nothing to write
    MAXK_REQUIRE(num_rows > 0 && num_cols > 0, "edges present but num_rows or num_cols == 0");
    MAXK_REQUIRE(row_ptr && col_idx && cbsr_val && cbsr_idx && grad_out && grad_edge,
                 "CSR / CBSR / grad_out / grad_edge pointers must not be NULL");
    const int D = dim_origin, k = dim_k, H = num_heads;
    const EdgeGradLayout L =
        edge_grad_heads_layout(num_rows, num_cols, num_e, D, k, H, chunk_edges);
    MAXK_REQUIRE(!L.wide, "num_cols: the multi-head edge gradient takes tables below 2^24 columns "
                 "and 4 GiB of records (%lld columns of %d bytes)", (long long)num_cols, L.RS);
    MAXK_REQUIRE(workspace && workspace_bytes >= L.total,
                 "workspace too small: need %zu bytes, got %zu", L.total, workspace_bytes);
    MAXK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-B aligned");
    MAXK_REQUIRE(((uintptr_t)cbsr_val & 3) == 0 && ((uintptr_t)grad_out & 3) == 0 &&
                     ((uintptr_t)grad_edge & 3) == 0,
                 "float buffers must be 4-B aligned");

    hipStream_t s = as_stream(stream);
    uint8_t *rec = reinterpret_cast<uint8_t *>(workspace);
    if (int rc = launch_cbsr_pack(cbsr_val, cbsr_idx, rec, num_cols, k, L.RS, D, L.DS - 1, s))
        return rc;
    constexpr int U = MAXK_EGRAD_U;
    const size_t lds = (size_t)kWavesPerBlock * (H * L.DS + kWave) * sizeof(float);
    const int64_t blocks = ceil_div(L.n_items, kWavesPerBlock);
    const dim3 grid((unsigned)(MAXK_FWD_XCD ? xcd_grid(blocks) : blocks));
    const int vec = D % 4 == 0 && ((uintptr_t)grad_out & 15) == 0;
    const bool ok = with_const<8, 16, 32, 64>(L.kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        hipLaunchKernelGGL((edge_grad_heads_kernel<KG, U>), grid, dim3(kBlock), lds, s, row_ptr,
                           col_idx, rec, L.RS, grad_out, row_div, grad_edge, (int)num_rows, num_e,
                           D, L.DS, k, L.chunk, L.n_items, H, vec);
    });
    if (!ok) return bad_lanes(L.kg);
    MAXK_LAUNCHED("edge_grad_heads_kernel");
    return MAXK_OK;
}
