// Multi-head forward row-wise-product SpGEMM for gfx950: H aggregations over one graph and one
// CBSR that differ only in their edge weights,
//
//   out[h, r, cbsr_idx[c, l]] += edge_val[h, e] * cbsr_val[c, l] / row_div[r]     0 <= h < H
//                                r = the CSR row holding e, c = col_idx[e]
//
// (head-major: edge_val [H, num_e], out [H, num_rows, D]; row_div is shared by the heads).  H
// calls of maxk_spgemm_forward gather the packed record of col_idx[e] H times; here one gather
// per edge serves all heads.  The pieces are the single-head forward's (spgemm_fwd.hip):
//
//  1. launch_cbsr_pack (cbsr_pack.h) writes this call's records, once for all heads.
//  2. spgemm_fwd_heads_kernel: the hub-row heads walk of heads_walk.h, which states the mapping
//     (KG lanes per group, G = 64 / KG LDS copies of the output row, exactly the single-head
//     kernel's LDS; the heads in passes of HC; group g on edge g / HC and head g % HC) and the
//     rules of the copies, the trash column, the flush and the slabs.  What is this file's: each
//     group multiplies by its own head's weight edge_val[h, e], and the flush divides by row_div
//     once.
//     LDS per wave: G * DS floats, DS = D padded to 16 B plus one 16-B group for the trash
//     column: 8.3 KB at D = 256, k <= 8; 4.2 KB at k <= 16; 2.1 KB at k <= 32; 1.0 KB above --
//     whatever H.  Resident waves per CU: 16 at k <= 8 and D = 256 (four 33-KB workgroups in
//     the 160 KB), else the VGPR limit: 68 to 72 VGPRs (the kernel-resource-usage remarks),
//     7 waves per SIMD, 28 per CU; no scratch.
//  3. slab_fixup_kernel<0> (common.h), once per head over the same slab_row, adds the slabs of
//     each split row onto the owner's partial in item order.
// The order of every sum is fixed by (graph, chunk, k, H): bitwise repeatable, and head h's
// slice holds only products with head h's weights, so it does not depend on the other heads'.
// No dense route, selector stream, accumulate or transport-record form; tables past 2^24
// columns or 4 GiB of records are rejected.  No allocation, copy or synchronisation.
#include "heads_walk.h"

namespace maxk {
namespace {

// One pass over the edges [sb, se) (sb < se) of a row piece: this lane's group adds
// wp[e] * value into its copy acc_g for the edges base + u * EP + eg it is given (active:
// the group has an edge slot and a head in this pass; else it writes its trash column only).
template <int KG, int U>
__device__ __forceinline__ void walk_heads(float *acc_g, const int32_t *__restrict__ col_idx,
                                           const float *__restrict__ wp,
                                           const uint8_t *__restrict__ rec, int RS, int sb, int se,
                                           int k, int trash, int EP, int eg, bool active,
                                           int lane) {
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
            w[u] = active && i < n ? wp[(int64_t)sb + i] : 0.f;
        }
        scatter_records<KG, U>(acc_g, rrs, RS, k, trash, l0, c, w, active, base, EP, eg, n);
    }
}

template <int KG, int U>
__global__ __launch_bounds__(kBlock) void spgemm_fwd_heads_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const float *__restrict__ edge_val, const uint8_t *__restrict__ rec, int RS,
    const float *__restrict__ row_div, float *__restrict__ out, float *__restrict__ slab,
    int32_t *__restrict__ slab_row, int num_rows, int64_t num_e, int D, int DS, int k, int chunk,
    int n_items, int H, int HC, int flags) {
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
    const bool scale = row_div != nullptr;

    // edges [sb, se) of row q, an owned row's into out, a continuation's into the item's slab:
    // every head is stored, an empty piece as zeros
    walk_hub_item(row_ptr, slab_row, num_rows, num_e, item, chunk, lane,
                  [&](int q, int64_t sb, int64_t se, bool, bool owned) {
        float *__restrict__ dst = owned ? out + (int64_t)q * D : slab + (int64_t)item * D;
        const int64_t hstride = (int64_t)(owned ? num_rows : n_items) * D;
        const float div = scale ? row_div[q] : 1.f;  // loaded before the walk
        for (int h0 = 0; h0 < H; h0 += HC) {
            const int head = h0 + g.hh;
            const bool active = g.grp_ok && head < H;
            wave_lds_fence();
            if (sb < se)
                walk_heads<KG, U>(g.acc_g, col_idx, edge_val + (active ? (int64_t)head * num_e : 0),
                                  rec, RS, (int)sb, (int)se, k, DS - 1, g.EP, g.eg, active, lane);
            wave_lds_fence();
            for (int j = 0; j < HC && h0 + j < H; ++j)
                flush_head<false>(acc + j * DS, g.EP, HC * DS, dst + (int64_t)(h0 + j) * hstride,
                                  D, div, scale, vec, nt && owned, lane, 1.f);
        }
        wave_lds_fence();
    });
}

struct HeadsLayout {
    int chunk, n_items, hc;
    size_t lds;  // per workgroup
    RecordGeom R;
    SlabLayout S;
};

HeadsLayout heads_layout(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k, int H,
                         int chunk) {
    HeadsLayout L{};
    L.R = record_geom(num_cols, D, k);
    L.hc = heads_per_pass(H, L.R.kg);
    // resident waves per CU: 7 per SIMD by VGPRs, fewer when the LDS copies fill the CU first
    L.lds = (size_t)kWavesPerBlock * (kWave / L.R.kg) * L.R.DS * sizeof(float);
    L.chunk = walk_chunk(num_rows, num_e, chunk, L.lds, 28);
    L.n_items = token_items(num_rows, num_e, L.chunk);
    L.S = slab_layout(L.n_items, H, D, al256((size_t)num_cols * L.R.RS), false);
    return L;
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" size_t maxk_spgemm_forward_heads_workspace_size(int64_t num_rows, int64_t num_cols,
                                                           int64_t num_e, int32_t dim_origin,
                                                           int32_t dim_k, int32_t num_heads,
                                                           int32_t chunk_edges) {
    if (num_rows < 0 || num_cols < 0 || num_e < 0 || dim_origin <= 0 || dim_k <= 0 ||
        num_heads < 1 || num_heads > MAXK_MAX_HEADS)
        return 0;
    return heads_layout(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads, chunk_edges)
        .S.end;
}

extern "C" int maxk_spgemm_forward_heads(const int32_t *row_ptr, const int32_t *col_idx,
                                         const float *edge_val, const float *cbsr_val,
                                         const uint8_t *cbsr_idx, const float *row_div, float *out,
                                         int64_t num_rows, int64_t num_cols, int64_t num_e,
                                         int32_t dim_origin, int32_t dim_k, int32_t num_heads,
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
    MAXK_REQUIRE(num_heads >= 1 && num_heads <= MAXK_MAX_HEADS,
                 "num_heads must be in [1,%d], got %d", MAXK_MAX_HEADS, num_heads);
    MAXK_REQUIRE(chunk_edges >= 0, "chunk_edges must be >= 0");
    MAXK_REQUIRE(num_cols * (int64_t)dim_k < (1LL << 31), "num_cols*k too large");
    if (num_rows == 0) return MAXK_OK;
    MAXK_REQUIRE(row_ptr && out, "row_ptr/out must not be NULL");
    const int D = dim_origin, k = dim_k, H = num_heads;
    hipStream_t s = as_stream(stream);
    if (num_e == 0) return zero_heads_out(out, nullptr, nullptr, H, num_rows, D, s);
    MAXK_REQUIRE(col_idx && edge_val && cbsr_val && cbsr_idx,
                 "CSR/CBSR pointers (col_idx, edge_val, cbsr_val, cbsr_idx) must not be NULL");
    MAXK_REQUIRE(num_cols > 0, "edges present but num_cols == 0");
    const HeadsLayout L = heads_layout(num_rows, num_cols, num_e, D, k, H, chunk_edges);
    const RecordGeom &R = L.R;
    MAXK_REQUIRE(!R.wide, "num_cols: the multi-head forward takes tables below 2^24 columns and "
                 "4 GiB of records (%lld columns of %d bytes)", (long long)num_cols, R.RS);
    MAXK_REQUIRE(workspace && workspace_bytes >= L.S.end,
                 "workspace too small: need %zu bytes, got %zu", L.S.end, workspace_bytes);
    MAXK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-B aligned");
    MAXK_REQUIRE(((uintptr_t)cbsr_val & 3) == 0 && ((uintptr_t)edge_val & 3) == 0 &&
                     ((uintptr_t)out & 3) == 0,
                 "float buffers must be 4-B aligned");

    char *ws = reinterpret_cast<char *>(workspace);
    uint8_t *rec = reinterpret_cast<uint8_t *>(ws);
    float *slab = reinterpret_cast<float *>(ws + L.S.slab_off);
    int32_t *slab_row = reinterpret_cast<int32_t *>(ws + L.S.row_off);
    if (int rc = launch_cbsr_pack(cbsr_val, cbsr_idx, rec, num_cols, k, R.RS, D, R.DS - 1, s))
        return rc;
    constexpr int U = MAXK_FWD_U;
    const int flags = store_flags(out, H, num_rows, D);
    const bool ok = with_const<8, 16, 32, 64>(R.kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        hipLaunchKernelGGL((spgemm_fwd_heads_kernel<KG, U>), item_grid(L.n_items), dim3(kBlock),
                           L.lds, s, row_ptr, col_idx, edge_val, rec, R.RS, row_div, out, slab,
                           slab_row, (int)num_rows, num_e, D, R.DS, k, L.chunk, L.n_items, H, L.hc,
                           flags);
    });
    if (!ok) return bad_lanes(R.kg);
    MAXK_LAUNCHED("spgemm_fwd_heads_kernel");
    for (int h = 0; h < H; ++h)
        if (int rc = launch_slab_fixup<0>(slab + (size_t)h * L.n_items * D, slab_row,
                                          out + (size_t)h * num_rows * D, D, L.n_items, s))
            return rc;
    return MAXK_OK;
}
