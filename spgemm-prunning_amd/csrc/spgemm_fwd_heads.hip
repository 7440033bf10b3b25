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
//  2. spgemm_fwd_heads_kernel, one wavefront per item of the token stream (token_items.h) under
//     the hub-row cut rule (CutHubRows).  Mapping, with KG = pow2ceil(k) lanes per group
//     (>= 8, <= 64) and G = 64 / KG groups and LDS copies of the output row per wave, exactly
//     the single-head kernel's LDS:
//     * the heads are walked in NP = ceil(H / G) passes of HC = ceil(H / NP) heads (one pass
//       whenever H <= G; H = 8 at k = 16, G = 4: two passes of four heads);
//     * in a pass, group g of a wave step works on (edge g / HC, head g % HC): EP = G / HC edges
//       per step, the HC groups of one edge issue the same record addresses in one load
//       instruction (one line fetched, not HC), and each multiplies by its own head's weight;
//     * copy g belongs to head g % HC: within a step the lanes of a group hit distinct columns
//       (the pack folds repeated selectors) and different groups hit different copies, so the
//       accumulation is plain ds_read / fma / ds_write -- no LDS atomics, no global atomics;
//       groups past EP * HC (G % HC != 0: H = 3, 5, 6, 7) and lanes l >= k write only their
//       copy's trash column;
//     * after a pass, head hh of it is the sum of copies hh, HC + hh, ... in that order, divided
//       by row_div once and stored (16-B stores where D % 4 == 0 and out is 16-B aligned): a
//       row whose tokens all lie in the item goes to out, a hub row's continuation to the
//       item's slab [H, n_items, D].  Every row of every head is stored, an edgeless row as
//       zeros: out needs no initialising.
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
#include "cbsr_pack.h"
#include "common.h"

namespace maxk {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

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
                *a = __builtin_fmaf(w[u], v[u], *a);  // one rounding, as in the single-head walk
            }
        }
    }
}

// dst[0:D] = (acc[0:D] + acc[stride + 0:D] + ... over nc copies) / div; the copies read are
// zeroed.  One wave.
__device__ __forceinline__ void flush_head(float *acc, int nc, int stride, float *__restrict__ dst,
                                           int D, float div, bool scale, bool vec, bool nt,
                                           int lane) {
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
            dst[j] = scale ? a / div : a;
        }
    }
}

template <int KG, int U>
__global__ __launch_bounds__(kBlock) void spgemm_fwd_heads_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const float *__restrict__ edge_val, const uint8_t *__restrict__ rec, int RS,
    const float *__restrict__ row_div, float *__restrict__ out, float *__restrict__ slab,
    int32_t *__restrict__ slab_row, int num_rows, int64_t num_e, int D, int DS, int k, int chunk,
    int n_items, int H, int HC, int flags) {
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
    const bool scale = row_div != nullptr;

    // edges [sb, se) of row q into dst rows of stride hstride per head: every head is stored,
    // an empty piece as zeros
    auto row_heads = [&](int q, int64_t sb, int64_t se, float *__restrict__ dst, int64_t hstride,
                         bool to_out) {
        const float div = scale ? row_div[q] : 1.f;  // loaded before the walk
        for (int h0 = 0; h0 < H; h0 += HC) {
            const int head = h0 + hh;
            const bool active = grp_ok && head < H;
            wave_lds_fence();
            if (sb < se)
                walk_heads<KG, U>(acc_g, col_idx, edge_val + (active ? (int64_t)head * num_e : 0),
                                  rec, RS, (int)sb, (int)se, k, DS - 1, EP, eg, active, lane);
            wave_lds_fence();
            for (int j = 0; j < HC && h0 + j < H; ++j)
                flush_head(acc + j * DS, EP, HC * DS, dst + (int64_t)(h0 + j) * hstride, D, div,
                           scale, vec, nt && to_out, lane);
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
            row_heads(r - 1, p.sb, p.se, slab + (int64_t)item * D, (int64_t)n_items * D, false);
            cont = r - 1;
        }
    }
    if (lane == 0) slab_row[item] = cont;

    // Rows whose token lies in [d0, d1): this item owns them.
    while (r < num_rows) {
        const int64_t rb = row_ptr[r];
        if (!row_owned(it.d1, r, rb)) break;
        const int64_t se = row_piece(CutHubRows{}, it.d1, r, rb, row_ptr[r + 1], chunk).se;
        row_heads(r, rb, se, out + (int64_t)r * D, (int64_t)num_rows * D, true);
        ++r;
    }
}

// A piece is addressed through a descriptor of 4 * n bytes with 32-bit offsets.
constexpr int kHeadsMaxChunk = 1 << 24;

struct HeadsLayout {
    int chunk, n_items, RS, DS, kg, hc;
    bool wide;
    size_t rec_bytes, slab_off, slab_bytes, row_off, total;
};

HeadsLayout heads_layout(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k, int H,
                         int chunk) {
    HeadsLayout L{};
    L.RS = record_stride(k, num_cols);
    L.DS = copy_stride(D);
    const int g = lanes_per_edge(k);
    L.kg = g < 8 ? 8 : g;
    const int G = kWave / L.kg;
    const int np = (H + G - 1) / G;
    L.hc = (H + np - 1) / np;
    L.wide = !(num_cols < (1 << 24) && (uint64_t)num_cols * (uint64_t)L.RS < (1ull << 32));
    // resident waves per CU: 7 per SIMD by VGPRs, fewer when the LDS copies fill the CU first
    const size_t per_block = (size_t)kWavesPerBlock * G * L.DS * sizeof(float);
    const int by_lds = (int)(kPullLdsBytes / per_block) * kWavesPerBlock;
    L.chunk = fwd_chunk(num_rows, num_e, chunk, by_lds < 28 ? by_lds : 28);
    if (L.chunk > kHeadsMaxChunk) L.chunk = kHeadsMaxChunk;
    L.n_items = token_items(num_rows, num_e, L.chunk);
    L.rec_bytes = al256((size_t)num_cols * L.RS);
    L.slab_off = L.rec_bytes;
    L.slab_bytes = al256((size_t)L.n_items * H * D * sizeof(float));
    L.row_off = L.slab_off + L.slab_bytes;
    L.total = L.row_off + al256((size_t)L.n_items * sizeof(int32_t));
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
        .total;
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
    if (num_e == 0)  // nothing to walk: zero rows
        return zero_words(out, (int64_t)H * num_rows * D, s);
    MAXK_REQUIRE(col_idx && edge_val && cbsr_val && cbsr_idx,
                 "CSR/CBSR pointers (col_idx, edge_val, cbsr_val, cbsr_idx) must not be NULL");
    MAXK_REQUIRE(num_cols > 0, "edges present but num_cols == 0");
    const HeadsLayout L = heads_layout(num_rows, num_cols, num_e, D, k, H, chunk_edges);
    MAXK_REQUIRE(!L.wide, "num_cols: the multi-head forward takes tables below 2^24 columns and "
                 "4 GiB of records (%lld columns of %d bytes)", (long long)num_cols, L.RS);
    MAXK_REQUIRE(workspace && workspace_bytes >= L.total,
                 "workspace too small: need %zu bytes, got %zu", L.total, workspace_bytes);
    MAXK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-B aligned");
    MAXK_REQUIRE(((uintptr_t)cbsr_val & 3) == 0 && ((uintptr_t)edge_val & 3) == 0 &&
                     ((uintptr_t)out & 3) == 0,
                 "float buffers must be 4-B aligned");

    char *ws = reinterpret_cast<char *>(workspace);
    uint8_t *rec = reinterpret_cast<uint8_t *>(ws);
    float *slab = reinterpret_cast<float *>(ws + L.slab_off);
    int32_t *slab_row = reinterpret_cast<int32_t *>(ws + L.row_off);
    if (int rc = launch_cbsr_pack(cbsr_val, cbsr_idx, rec, num_cols, k, L.RS, D, L.DS - 1, s))
        return rc;
    constexpr int U = MAXK_FWD_U;
    const int G = kWave / L.kg;
    const size_t lds = (size_t)kWavesPerBlock * G * L.DS * sizeof(float);
    const int64_t blocks = ceil_div(L.n_items, kWavesPerBlock);
    const dim3 grid((unsigned)(MAXK_FWD_XCD ? xcd_grid(blocks) : blocks));
    // rows past the Infinity Cache's size are stored non-temporally, as the single-head forward
    // stores them (MAXK_FWD_OUT_NT)
    const bool big = (double)H * num_rows * D * 4 > (double)kInfinityCacheBytes;
    const int flags = (D % 4 == 0 && ((uintptr_t)out & 15) == 0 ? 1 : 0) |
                      ((MAXK_FWD_OUT_NT == 1 || (MAXK_FWD_OUT_NT == 2 && big)) ? 2 : 0);
    const bool ok = with_const<8, 16, 32, 64>(L.kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        hipLaunchKernelGGL((spgemm_fwd_heads_kernel<KG, U>), grid, dim3(kBlock), lds, s, row_ptr,
                           col_idx, edge_val, rec, L.RS, row_div, out, slab, slab_row,
                           (int)num_rows, num_e, D, L.DS, k, L.chunk, L.n_items, H, L.hc, flags);
    });
    if (!ok) return bad_lanes(L.kg);
    MAXK_LAUNCHED("spgemm_fwd_heads_kernel");
    for (int h = 0; h < H; ++h)
        if (int rc = launch_slab_fixup<0>(slab + (size_t)h * L.n_items * D, slab_row,
                                          out + (size_t)h * num_rows * D, D, L.n_items, s))
            return rc;
    return MAXK_OK;
}
