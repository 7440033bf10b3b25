// Backward SSpMM on 16-bit selectors, 1 <= D <= 1024, as the two-phase csc form:
//   grad_cbsr[c, l] = sum_{e=(r->c)} val[e] * G[r, sel[c, l]] / row_div[r]
//
// Phase 1, x16_bwd_kernel<KG, U> (this file): one wave per item of the token stream
// (token_items.h, CutAtEnd, driven by walk_cut_item).  For every row piece the wave stages
// G[r, :] / row_div[r] in LDS with 16-B loads -- D floats, 4 KB at D = 1024, one row per wave --
// and then lane groups of KG = pow2ceil(k) lanes (at most a wave; past 64 slots a lane walks
// l, l + 64, ...) take one edge each, U wave steps in flight: the group reads its destination's
// k contiguous u16 selectors, picks from the LDS row, multiplies by val[e] and stores the
// contribution row T[e, 0..k) coalesced.  A selector >= D contributes 0.
// Phase 2 is csc_sum_rows (sspmm_push.hip, through sspmm_bwd.h) unchanged: it does not depend on
// D.  Bitwise repeatable: no atomics, each destination summed in CSC slot order.
// DESIGN.md 5.20.
#include "sspmm_bwd.h"
#include "x16_pack.h"

namespace maxk {
namespace {

template <int KG, int U>
__global__ __launch_bounds__(kBlock) void x16_bwd_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const float *__restrict__ edge_val, const float *__restrict__ grad,
    const float *__restrict__ row_div, const uint16_t *__restrict__ cbsr_idx, uint32_t idx_bytes,
    float *__restrict__ T, int num_rows, int64_t num_e, int D, int DS, int k, int chunk,
    int n_items, int vec) {
    constexpr int G = kWave / KG;  // edges per wave step
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = lane_id();
    const int item = item_of_wave(n_items);
    if (item < 0) return;  // whole wave; no workgroup barrier below
    float *row = lds + (size_t)(threadIdx.x / kWave) * DS;
    const int grp = lane / KG, l0 = lane % KG;
    // the selector table: a load past it (a column out of range) returns 0
    const auto irs = wave_buffer(cbsr_idx, idx_bytes);
    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);
    walk_cut_item(row_ptr, num_rows, it, [&](int q, int64_t sb, int64_t se, int64_t, bool) {
        if (sb >= se) return;
        // stage G[q, :] / row_div[q]
        const float div = row_div ? row_div[q] : 1.f;
        const float *g = grad + (int64_t)q * D;
        wave_lds_fence();  // the previous piece's picks are done
        if (vec) {
            for (int j = lane * 4; j < D; j += kWave * 4) {
                float4 x = *reinterpret_cast<const float4 *>(g + j);
                if (row_div) {
                    x.x = x.x / div;
                    x.y = x.y / div;
                    x.z = x.z / div;
                    x.w = x.w / div;
                }
                *reinterpret_cast<float4 *>(row + j) = x;
            }
        } else {
            for (int j = lane; j < D; j += kWave) row[j] = row_div ? g[j] / div : g[j];
        }
        wave_lds_fence();
        const int n = (int)(se - sb);  // wave-uniform, at most chunk
        const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
        const auto vrs = wave_buffer(edge_val + sb, (uint32_t)n * 4u);
        float *Tp = T + (size_t)sb * k;
        for (int base = 0; base < n; base += G * U) {
            uint32_t io[U];
            float w[U];
            const int lo = (base + grp) * 4;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                io[u] = __builtin_amdgcn_raw_buffer_load_b32(crs, lo + u * G * 4, 0, 0) *
                        (uint32_t)k * 2u;
                w[u] = __uint_as_float(
                    __builtin_amdgcn_raw_buffer_load_b32(vrs, lo + u * G * 4, 0, 0));
            }
            for (int lb = 0; lb < k; lb += KG) {  // one pass unless k > 64
                const int l = lb + l0;
                const bool lok = l < k;
                const uint32_t so = 2u * (uint32_t)(lok ? l : k - 1);
                int s[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    s[u] = (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(irs, (int)(io[u] + so),
                                                                          0, 0);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int e = base + u * G + grp;
                    const float picked = row[s[u] < D ? s[u] : 0];
                    const float x = w[u] * (s[u] < D ? picked : 0.f);
                    if (lok && e < n)  // contribution rows streamed past the caches
                        __builtin_nontemporal_store(x, Tp + (size_t)e * k + l);
                }
            }
        }
    });
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" size_t maxk_sspmm_backward_x16_workspace_size(int64_t num_rows, int64_t num_cols,
                                                         int64_t num_e, int32_t dim_origin,
                                                         int32_t dim_k, int32_t chunk_edges) {
    if (num_rows < 0 || num_cols < 0 || num_e < 0 || chunk_edges < 0 ||
        !x16_dims_ok(dim_origin, dim_k))
        return 0;
    return csc_sum_workspace_size(num_cols, num_e, dim_k, chunk_edges);
}

extern "C" int maxk_sspmm_backward_x16(const int32_t *row_ptr, const int32_t *col_idx,
                                       const float *edge_val, const float *grad_out,
                                       const uint16_t *cbsr_idx, const float *row_div,
                                       const int32_t *col_ptr, const int32_t *csc_eid,
                                       float *grad_cbsr, int64_t num_rows, int64_t num_cols,
                                       int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                       int32_t chunk_edges, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    clear_error();
    if (int rc = x16_check_dims(dim_origin, dim_k)) return rc;
    MAXK_REQUIRE(num_rows >= 0 && num_rows < (1LL << 31), "num_rows out of range");
    MAXK_REQUIRE(num_cols >= 0 && num_cols < (1LL << 31), "num_cols out of range");
    MAXK_REQUIRE(num_e >= 0 && num_e < (1LL << 31), "num_e out of range");
    MAXK_REQUIRE(chunk_edges >= 0 && chunk_edges <= kMaxChunk, "chunk_edges must be in [0, 2^24]");
    MAXK_REQUIRE(num_cols * (int64_t)dim_k < (1LL << 31), "num_cols*k too large");
    if (num_cols == 0) return MAXK_OK;
    MAXK_REQUIRE(grad_cbsr && col_ptr, "grad_cbsr/col_ptr must not be NULL");
    MAXK_REQUIRE(num_e == 0 || (row_ptr && col_idx && edge_val && grad_out && cbsr_idx && csc_eid),
                 "CSR/grad/selector/transpose pointers must not be NULL");
    const size_t need = csc_sum_workspace_size(num_cols, num_e, dim_k, chunk_edges);
    MAXK_REQUIRE(workspace && workspace_bytes >= need,
                 "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    MAXK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-B aligned");
    MAXK_REQUIRE(((uintptr_t)grad_out & 3) == 0 && ((uintptr_t)cbsr_idx & 1) == 0,
                 "grad_out must be 4-B aligned, cbsr_idx 2-B aligned");
    hipStream_t s = as_stream(stream);
    const int D = dim_origin, k = dim_k;
    if (num_e > 0 && num_rows > 0) {
        const int DS = x16_copy_stride(D);
        const int chunk = x16_chunk(num_rows, num_e, chunk_edges);
        const int n_items = token_items(num_rows, num_e, chunk);
        const int vec = D % 4 == 0 && ((uintptr_t)grad_out & 15) == 0;
        const int kg = x16_lanes(k, 8);
        const bool ok = with_const<8, 16, 32, 64>(kg, [&](auto kg_c) {
            constexpr int KG = decltype(kg_c)::value;
            hipLaunchKernelGGL((x16_bwd_kernel<KG, 4>), item_grid(n_items), dim3(kBlock),
                               (size_t)kWavesPerBlock * DS * sizeof(float), s, row_ptr, col_idx,
                               edge_val, grad_out, row_div, cbsr_idx,
                               (uint32_t)(num_cols * dim_k * 2), reinterpret_cast<float *>(workspace),
                               (int)num_rows, num_e, D, DS, k, chunk, n_items, vec);
        });
        if (!ok) return bad_lanes(kg);
        MAXK_LAUNCHED("x16_bwd_kernel");
    }
    return csc_sum_rows(s, col_ptr, csc_eid, workspace, grad_cbsr, num_cols, num_e, k, chunk_edges);
}
