// Multi-head aggregation on 16-bit selectors, 1 <= D <= 1024, 1 <= k <= min(D, 256),
// 1 <= H <= MAXK_MAX_HEADS: the three kernels the stored attention path of the GAT and transformer
// layers needs past 256 columns.  Head-major like the u8 entries (spgemm_fwd_heads.hip,
// edge_grad.hip, sspmm_push.hip): edge_val, grad_edge [H, E]; out, grad_out [H, R, D]; row_div
// shared by the heads.  DESIGN.md 5.22.
//
//   forward        out[h, r, sel[c,l]] += edge_val[h,e] * val[c,l] / row_div[r]
//   edge gradient  grad_edge[h,e] = (sum_l val[c,l] * grad_out[h, r, sel[c,l]]) / row_div[r]
//   backward       grad_cbsr[c,l] = sum_h sum_{e=(r->c)} edge_val[h,e] * grad_out[h,r,sel[c,l]]
//                                   / row_div[r]
//
// What a D of up to 1024 changes against the u8 kernels is the LDS: a dense row is up to 4 KB, so
// the rows a wave keeps -- output copies in the forward, staged grad_out rows in the other two --
// are set by D and stay in the single-head x16 budget of about 8 KB per wave (33 KB per
// workgroup: four workgroups, 16 waves, per CU of 160 KB).  The heads then go in passes:
//
//  * x16_fwd_heads_kernel<KG, U>: one wave per item of the token stream under CutHubRows
//    (heads_walk.h's walk_hub_item).  NC = 64 / KG copies of DS = pad4(D) + 4 floats, KG as in
//    x16_fwd.hip (NC = 4 up to D = 508, 2 up to D = 1024, 1 when k > 32).  A pass takes
//    HC = min(heads left, NC) heads; lane group g works on head g % HC and edge g / HC, so the HC
//    groups of an edge read the same record lines in the same load instruction and a pass gathers
//    a record once for its heads.  A copy belongs to one head within a pass: plain ds_read / fma /
//    ds_write.  Heads are flushed in head order, row_div applied once; a hub row's continuation
//    goes to the item's slab of its head, and slab_fixup_kernel<0> runs once per head.
//  * x16_edge_grad_heads_kernel<KG, U>: CutAtEnd items (walk_cut_item).  Per row piece and pass the
//    HP = min(heads left, x16_rows_in_budget(DS)) rows grad_out[h, r, :] are staged side by side;
//    per edge the record (value, column) is gathered once per pass, each head takes one fma per
//    slot against its row and the fixed butterfly lane_tree, and lane 0 of the group stores
//    grad_edge[h, e].  A folded or out-of-range slot names the trash column DS - 1, a pad column
//    that holds 0, with value 0; a column the vertex does not select is never read.
//  * x16_bwd_heads_kernel<KG, U>: phase 1 of the two-phase csc form.  The same staging, of
//    grad_out[h, r, :] / row_div[r]; per edge the destination's selectors are gathered once per
//    pass, the heads of the pass are summed in head order in registers and one contribution row
//    T[e, 0:k] is stored.  With H <= HP (every H up to 4 at D <= 508, up to 2 at D = 1024) that
//    is one gather, one row written and one row read per edge whatever H; a later pass adds onto
//    the row the same lane wrote.  At H = 1 the arithmetic is x16_bwd_kernel's, bit for bit.
//    Phase 2 is csc_sum_rows (sspmm_push.hip) unchanged.
// No global atomics, no LDS float atomics; every sum has an order fixed by (graph, chunk, k, D,
// H): bitwise repeatable.  Inputs are never written.  No allocation, copy or synchronisation.
#include "piece_walk.h"
#include "sspmm_bwd.h"
#include "x16_pack.h"

namespace maxk {
namespace {

constexpr int kX16HeadsU = 4;  // wave steps of edges in flight in the two staged-row walks

// One pass of the forward over the edges [sb, se) (sb < se) of a row piece: this lane's group adds
// wp[e] * value into its copy acc_g for the edges base + u * EP + eg (active: the group has an
// edge slot in this pass; else, like a lane past k and an edge past se, it writes its copy's trash
// column only).  wp: the weights of the group's head.
template <int KG, int U>
__device__ __forceinline__ void x16_walk_heads(float *acc_g, const int32_t *__restrict__ col_idx,
                                               const float *__restrict__ wp,
                                               __amdgpu_buffer_rsrc_t rrs, int RS, int sb, int se,
                                               int k, int trash, int EP, int eg, bool active,
                                               int lane) {
    const int l0 = lane % KG;
    const int n = se - sb;  // wave-uniform, <= 2 * chunk
    const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
    for (int base = 0; base < n; base += EP * U) {
        uint32_t ro[U];
        float w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = base + u * EP + eg;
            // past the piece's end the column reads 0 (column 0's record) and the weight is 0
            ro[u] = __builtin_amdgcn_raw_buffer_load_b32(crs, i * 4, 0, 0) * (uint32_t)RS;
            w[u] = active && i < n ? wp[(int64_t)sb + i] : 0.f;
        }
        for (int lb = 0; lb < k; lb += KG) {  // one pass unless k > 64
            const int l = lb + l0;
            const bool lok = l < k;
            const uint32_t lc = (uint32_t)(lok ? l : k - 1);  // clamped: no load leaves the record
            const uint32_t vo = 4u * lc, so = 4u * (uint32_t)k + 2u * lc;
            float v[U];
            int s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                v[u] = __uint_as_float(
                    __builtin_amdgcn_raw_buffer_load_b32(rrs, (int)(ro[u] + vo), 0, 0));
                s[u] = (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(rrs, (int)(ro[u] + so), 0, 0);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool live = lok && active && base + u * EP + eg < n;
                float *a = &acc_g[live ? min(s[u], trash) : trash];
                *a = __builtin_fmaf(w[u], v[u], *a);  // one rounding, as in x16_fwd.hip
            }
        }
    }
}

template <int KG, int U>
__global__ __launch_bounds__(kBlock) void x16_fwd_heads_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const float *__restrict__ edge_val, const uint8_t *__restrict__ rec, uint32_t rec_bytes, int RS,
    const float *__restrict__ row_div, float *__restrict__ out, float *__restrict__ slab,
    int32_t *__restrict__ slab_row, int num_rows, int64_t num_e, int D, int DS, int k, int chunk,
    int n_items, int H, int vec) {
    constexpr int NC = kWave / KG;  // LDS copies per wave (one per lane group)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = lane_id();
    const int item = item_of_wave(n_items);
    if (item < 0) return;  // whole wave; no workgroup barrier below
    float *acc = lds + (size_t)(threadIdx.x / kWave) * NC * DS;
    zero_wave_lds(acc, NC * DS, lane);
    // the full passes take HC heads; a last pass of fewer heads spreads them over all the copies
    const int HC = H < NC ? H : NC, HT = H % HC;
    const PassGeom<KG> full(lane, HC, acc, DS), last(lane, HT ? HT : HC, acc, DS);
    // the record table: a load past it (a column out of range) returns 0
    const auto rrs = wave_buffer(rec, rec_bytes);
    const bool scale = row_div != nullptr;

    // edges [sb, se) of row q, an owned row's into out, a continuation's into the item's slab:
    // every head is stored, an empty piece as zeros
    walk_hub_item(row_ptr, slab_row, num_rows, num_e, item, chunk, lane,
                  [&](int q, int64_t sb, int64_t se, bool, bool owned) {
        float *__restrict__ dst = owned ? out + (int64_t)q * D : slab + (int64_t)item * D;
        const int64_t hstride = (int64_t)(owned ? num_rows : n_items) * D;
        const float div = scale ? row_div[q] : 1.f;  // loaded before the walk
        for (int h0 = 0; h0 < H; h0 += HC) {
            const bool tail = H - h0 < HC;
            const PassGeom<KG> &g = tail ? last : full;
            const int hc = tail ? HT : HC;
            wave_lds_fence();
            if (sb < se)
                x16_walk_heads<KG, U>(g.acc_g, col_idx,
                                      edge_val + (g.grp_ok ? (int64_t)(h0 + g.hh) * num_e : 0), rrs,
                                      RS, (int)sb, (int)se, k, DS - 1, g.EP, g.eg, g.grp_ok, lane);
            wave_lds_fence();
            for (int j = 0; j < hc; ++j)
                flush_head<false>(acc + j * DS, g.EP, hc * DS, dst + (int64_t)(h0 + j) * hstride,
                                  D, div, scale, vec != 0, false, lane, 1.f);
        }
        wave_lds_fence();
    });
}

// rows[j * DS + 0:D] = grad[h0 + j, q, 0:D] (/ div when SCALED), j < hp.  One wave; the division
// is x16_bwd_kernel's, element by element.
template <bool SCALED>
__device__ __forceinline__ void stage_head_rows(float *rows, int DS, const float *__restrict__ grad,
                                                int64_t num_rows, int q, int D, int h0, int hp,
                                                float div, bool scale, bool vec, int lane) {
    for (int j = 0; j < hp; ++j) {
        const float *g = grad + ((int64_t)(h0 + j) * num_rows + q) * D;
        float *row = rows + j * DS;
        if (!SCALED || !scale) {
            stage_row(row, g, D, vec, lane);
        } else if (vec) {
            for (int c = lane * 4; c < D; c += kWave * 4) {
                float4 x = *reinterpret_cast<const float4 *>(g + c);
                x.x = x.x / div;
                x.y = x.y / div;
                x.z = x.z / div;
                x.w = x.w / div;
                *reinterpret_cast<float4 *>(row + c) = x;
            }
        } else {
            for (int c = lane; c < D; c += kWave) row[c] = g[c] / div;
        }
    }
}

template <int KG, int U>
__global__ __launch_bounds__(kBlock) void x16_edge_grad_heads_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const uint8_t *__restrict__ rec, uint32_t rec_bytes, int RS,
    const float *__restrict__ grad_out, const float *__restrict__ row_div,
    float *__restrict__ grad_edge, int num_rows, int64_t num_e, int D, int DS, int k, int chunk,
    int n_items, int H, int HP, int vec) {
    constexpr int G = kWave / KG;  // edges per wave step
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = lane_id();
    const int item = item_of_wave(n_items);
    if (item < 0) return;  // whole wave; no workgroup barrier below
    float *rows = lds + (size_t)(threadIdx.x / kWave) * HP * DS;
    // the pad columns [D, DS) of every row are never staged over: zeroed once (DS - D <= 7), so
    // the trash column reads 0
    for (int j = 0; j < HP; ++j)
        if (lane < DS - D) rows[j * DS + D + lane] = 0.f;
    const int grp = lane / KG, l0 = lane % KG;
    const int trash = DS - 1;
    const auto rrs = wave_buffer(rec, rec_bytes);
    const bool scale = row_div != nullptr;
    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);
    walk_cut_item(row_ptr, num_rows, it, [&](int q, int64_t sb, int64_t se, int64_t, bool) {
        if (sb >= se) return;
        const float div = scale ? row_div[q] : 1.f;  // loaded before the walk
        const int n = (int)(se - sb);                // wave-uniform, at most chunk
        const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
        for (int h0 = 0; h0 < H; h0 += HP) {
            const int hp = H - h0 < HP ? H - h0 : HP;
            wave_lds_fence();  // the previous pass's reads of the rows are done
            stage_head_rows<false>(rows, DS, grad_out, num_rows, q, D, h0, hp, 1.f, false,
                                   vec != 0, lane);
            wave_lds_fence();
            float *__restrict__ ge = grad_edge + (int64_t)h0 * num_e + sb;
            for (int base = 0; base < n; base += G * U) {
                uint32_t ro[U];
                float acc[MAXK_MAX_HEADS][U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    ro[u] = __builtin_amdgcn_raw_buffer_load_b32(crs, (base + u * G + grp) * 4, 0,
                                                                 0) * (uint32_t)RS;
#pragma unroll
                for (int j = 0; j < MAXK_MAX_HEADS; ++j)
#pragma unroll
                    for (int u = 0; u < U; ++u) acc[j][u] = 0.f;
                for (int lb = 0; lb < k; lb += KG) {  // one pass unless k > 64
                    const int l = lb + l0;
                    const bool lok = l < k;
                    const uint32_t lc = (uint32_t)(lok ? l : k - 1);  // clamped into the record
                    const uint32_t vo = 4u * lc, so = 4u * (uint32_t)k + 2u * lc;
                    float v[U];
                    int s[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        v[u] = __uint_as_float(
                            __builtin_amdgcn_raw_buffer_load_b32(rrs, (int)(ro[u] + vo), 0, 0));
                        s[u] = min((int)(uint16_t)__builtin_amdgcn_raw_buffer_load_b16(
                                       rrs, (int)(ro[u] + so), 0, 0), trash);
                    }
#pragma unroll
                    for (int j = 0; j < MAXK_MAX_HEADS; ++j) {
                        if (j >= hp) break;  // wave-uniform
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const float t = __builtin_fmaf(v[u], rows[j * DS + s[u]], acc[j][u]);
                            acc[j][u] = lok ? t : acc[j][u];  // an idle lane's clamped slot: nothing
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < MAXK_MAX_HEADS; ++j) {
                    if (j >= hp) break;
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const float x = lane_tree<KG, Sum>(acc[j][u]);
                        const int e = base + u * G + grp;
                        if (l0 == 0 && e < n) ge[(int64_t)j * num_e + e] = scale ? x / div : x;
                    }
                }
            }
        }
    });
}

template <int KG, int U>
__global__ __launch_bounds__(kBlock) void x16_bwd_heads_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const float *__restrict__ edge_val, const float *__restrict__ grad,
    const float *__restrict__ row_div, const uint16_t *__restrict__ cbsr_idx, uint32_t idx_bytes,
    float *__restrict__ T, int num_rows, int64_t num_e, int D, int DS, int k, int chunk,
    int n_items, int H, int HP, int vec) {
    constexpr int G = kWave / KG;  // edges per wave step
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = lane_id();
    const int item = item_of_wave(n_items);
    if (item < 0) return;  // whole wave; no workgroup barrier below
    float *rows = lds + (size_t)(threadIdx.x / kWave) * HP * DS;
    const int grp = lane / KG, l0 = lane % KG;
    // the selector table: a load past it (a column out of range) returns 0
    const auto irs = wave_buffer(cbsr_idx, idx_bytes);
    const bool scale = row_div != nullptr;
    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);
    walk_cut_item(row_ptr, num_rows, it, [&](int q, int64_t sb, int64_t se, int64_t, bool) {
        if (sb >= se) return;
        const float div = scale ? row_div[q] : 1.f;
        const int n = (int)(se - sb);  // wave-uniform, at most chunk
        const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
        float *Tp = T + (size_t)sb * k;
        for (int h0 = 0; h0 < H; h0 += HP) {
            const int hp = H - h0 < HP ? H - h0 : HP;
            wave_lds_fence();  // the previous pass's picks are done
            stage_head_rows<true>(rows, DS, grad, num_rows, q, D, h0, hp, div, scale, vec != 0,
                                  lane);
            wave_lds_fence();
            const float *__restrict__ wv = edge_val + (int64_t)h0 * num_e + sb;
            for (int base = 0; base < n; base += G * U) {
                uint32_t io[U];
                float w[MAXK_MAX_HEADS][U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    io[u] = __builtin_amdgcn_raw_buffer_load_b32(crs, (base + u * G + grp) * 4, 0,
                                                                 0) * (uint32_t)k * 2u;
#pragma unroll
                for (int j = 0; j < MAXK_MAX_HEADS; ++j)
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int e = base + u * G + grp;
                        w[j][u] = j < hp && e < n ? wv[(int64_t)j * num_e + e] : 0.f;
                    }
                for (int lb = 0; lb < k; lb += KG) {  // one pass unless k > 64
                    const int l = lb + l0;
                    const bool lok = l < k;
                    const uint32_t so = 2u * (uint32_t)(lok ? l : k - 1);
                    int s[U];
                    float x[U];
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        s[u] = (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(
                            irs, (int)(io[u] + so), 0, 0);
#pragma unroll
                    for (int u = 0; u < U; ++u) {  // the pass's first head: x16_bwd_kernel's product
                        const float picked = rows[s[u] < D ? s[u] : 0];
                        x[u] = w[0][u] * (s[u] < D ? picked : 0.f);
                    }
#pragma unroll
                    for (int j = 1; j < MAXK_MAX_HEADS; ++j) {  // the others, in head order
                        if (j >= hp) break;                      // wave-uniform
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const float picked = rows[j * DS + (s[u] < D ? s[u] : 0)];
                            x[u] = __builtin_fmaf(w[j][u], s[u] < D ? picked : 0.f, x[u]);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int e = base + u * G + grp;
                        if (lok && e < n) {
                            float *t = Tp + (size_t)e * k + l;
                            // a later pass adds onto what this lane stored in the one before
                            if (h0 > 0) x[u] = *t + x[u];
                            __builtin_nontemporal_store(x[u], t);  // streamed past the caches
                        }
                    }
                }
            }
        }
    });
}

// ---- host -----------------------------------------------------------------------------------------

int x16_heads_check(int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t D, int32_t k,
                    int32_t H, int32_t chunk) {
    if (int rc = x16_check_dims(D, k)) return rc;
    MAXK_REQUIRE(H >= 1 && H <= MAXK_MAX_HEADS, "num_heads must be in [1,%d], got %d",
                 MAXK_MAX_HEADS, H);
    MAXK_REQUIRE(num_rows >= 0 && num_rows < (1LL << 31), "num_rows out of range: %lld",
                 (long long)num_rows);
    MAXK_REQUIRE(num_cols >= 0 && num_cols < (1LL << 31), "num_cols out of range");
    MAXK_REQUIRE(num_e >= 0 && num_e < (1LL << 31), "num_e out of range: %lld", (long long)num_e);
    MAXK_REQUIRE(chunk >= 0 && chunk <= kMaxChunk, "chunk_edges must be in [0, 2^24]");
    MAXK_REQUIRE(num_cols * (int64_t)k < (1LL << 31), "num_cols*k too large");
    return MAXK_OK;
}
bool x16_heads_ok(int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t D, int32_t k,
                  int32_t H, int32_t chunk) {
    return num_rows >= 0 && num_cols >= 0 && num_e >= 0 && chunk >= 0 && x16_dims_ok(D, k) &&
           H >= 1 && H <= MAXK_MAX_HEADS;
}

// The items and the record table of a walk; the forward adds its slabs [H, cap, D] and slab_row.
struct X16HeadsLayout {
    int chunk, n_items, RS, DS;
    size_t rec_bytes;
    SlabLayout S;
};
X16HeadsLayout x16_heads_layout(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k,
                                int H, int chunk) {
    X16HeadsLayout L{};
    L.RS = x16_record_stride(k);
    L.DS = x16_copy_stride(D);
    L.chunk = x16_chunk(num_rows, num_e, chunk);
    L.n_items = token_items(num_rows, num_e, L.chunk);
    L.rec_bytes = (size_t)num_cols * L.RS;
    L.S = slab_layout(x16_item_cap(num_rows + num_e, chunk, L.n_items), H, D, al256(L.rec_bytes),
                      false);
    return L;
}

int x16_rec_check(const X16HeadsLayout &L) {
    MAXK_REQUIRE(L.rec_bytes < (1ull << 32),
                 "packed record table of %zu bytes: num_cols * %d must stay below 4 GiB",
                 L.rec_bytes, L.RS);
    return MAXK_OK;
}
int x16_ws_check(const void *workspace, size_t workspace_bytes, size_t need) {
    MAXK_REQUIRE(workspace && workspace_bytes >= need,
                 "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    MAXK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-B aligned");
    return MAXK_OK;
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" size_t maxk_spgemm_forward_heads_x16_workspace_size(int64_t num_rows, int64_t num_cols,
                                                               int64_t num_e, int32_t dim_origin,
                                                               int32_t dim_k, int32_t num_heads,
                                                               int32_t chunk_edges) {
    if (!x16_heads_ok(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads, chunk_edges))
        return 0;
    return x16_heads_layout(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads, chunk_edges)
        .S.end;
}

extern "C" int maxk_spgemm_forward_heads_x16(const int32_t *row_ptr, const int32_t *col_idx,
                                             const float *edge_val, const float *cbsr_val,
                                             const uint16_t *cbsr_idx, const float *row_div,
                                             float *out, int64_t num_rows, int64_t num_cols,
                                             int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                             int32_t num_heads, int32_t chunk_edges,
                                             void *workspace, size_t workspace_bytes,
                                             void *stream) {
    clear_error();
    if (int rc = x16_heads_check(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads,
                                 chunk_edges))
        return rc;
    if (num_rows == 0) return MAXK_OK;
    MAXK_REQUIRE(row_ptr && out, "row_ptr/out must not be NULL");
    const int D = dim_origin, k = dim_k, H = num_heads;
    hipStream_t s = as_stream(stream);
    if (num_e == 0) return zero_heads_out(out, nullptr, nullptr, H, num_rows, D, s);
    MAXK_REQUIRE(col_idx && edge_val && cbsr_val && cbsr_idx,
                 "CSR/CBSR pointers (col_idx, edge_val, cbsr_val, cbsr_idx) must not be NULL");
    MAXK_REQUIRE(num_cols > 0, "edges present but num_cols == 0");
    const X16HeadsLayout L = x16_heads_layout(num_rows, num_cols, num_e, D, k, H, chunk_edges);
    if (int rc = x16_rec_check(L)) return rc;
    if (int rc = x16_ws_check(workspace, workspace_bytes, L.S.end)) return rc;
    MAXK_REQUIRE(((uintptr_t)cbsr_val & 3) == 0 && ((uintptr_t)cbsr_idx & 1) == 0 &&
                     ((uintptr_t)edge_val & 3) == 0 && ((uintptr_t)out & 3) == 0,
                 "float buffers must be 4-B aligned, cbsr_idx 2-B aligned");

    char *ws = reinterpret_cast<char *>(workspace);
    uint8_t *rec = reinterpret_cast<uint8_t *>(ws);
    float *slab = reinterpret_cast<float *>(ws + L.S.slab_off);
    int32_t *slab_row = reinterpret_cast<int32_t *>(ws + L.S.row_off);
    if (int rc = launch_x16_pack(cbsr_val, cbsr_idx, rec, num_cols, k, L.RS, D, L.DS - 1, s))
        return rc;
    const int vec = D % 4 == 0 && ((uintptr_t)out & 15) == 0;
    // KG as x16_fwd.hip: pow2ceil(k), at least 64 / (the copies D allows: 4 up to D = 508, else 2)
    const int kg = x16_lanes(k, L.DS <= 512 ? 16 : 32);
    const bool ok = with_const<16, 32, 64>(kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        const size_t lds = (size_t)kWavesPerBlock * (kWave / KG) * L.DS * sizeof(float);
        hipLaunchKernelGGL((x16_fwd_heads_kernel<KG, 8>), item_grid(L.n_items), dim3(kBlock), lds,
                           s, row_ptr, col_idx, edge_val, rec, (uint32_t)L.rec_bytes, L.RS,
                           row_div, out, slab, slab_row, (int)num_rows, num_e, D, L.DS, k, L.chunk,
                           L.n_items, H, vec);
    });
    if (!ok) return bad_lanes(kg);
    MAXK_LAUNCHED("x16_fwd_heads_kernel");
    for (int h = 0; h < H; ++h)
        if (int rc = launch_slab_fixup<0>(slab + (size_t)h * L.n_items * D, slab_row,
                                          out + (size_t)h * num_rows * D, D, L.n_items, s))
            return rc;
    return MAXK_OK;
}

extern "C" size_t maxk_edge_weight_grad_heads_x16_workspace_size(int64_t num_rows,
                                                                 int64_t num_cols, int64_t num_e,
                                                                 int32_t dim_origin, int32_t dim_k,
                                                                 int32_t num_heads,
                                                                 int32_t chunk_edges) {
    if (!x16_heads_ok(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads, chunk_edges))
        return 0;
    const size_t n = al256((size_t)num_cols * x16_record_stride(dim_k));
    return n ? n : 256;  // never empty: one query serves any num_cols
}

extern "C" int maxk_edge_weight_grad_heads_x16(const int32_t *row_ptr, const int32_t *col_idx,
                                               const float *cbsr_val, const uint16_t *cbsr_idx,
                                               const float *grad_out, const float *row_div,
                                               float *grad_edge, int64_t num_rows,
                                               int64_t num_cols, int64_t num_e, int32_t dim_origin,
                                               int32_t dim_k, int32_t num_heads,
                                               int32_t chunk_edges, void *workspace,
                                               size_t workspace_bytes, void *stream) {
    clear_error();
    if (int rc = x16_heads_check(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads,
                                 chunk_edges))
        return rc;
    if (num_e == 0) return MAXK_OK;  // no edge, nothing to write
    MAXK_REQUIRE(num_rows > 0 && num_cols > 0, "edges present but num_rows or num_cols == 0");
    MAXK_REQUIRE(row_ptr && col_idx && cbsr_val && cbsr_idx && grad_out && grad_edge,
                 "CSR / CBSR / grad_out / grad_edge pointers must not be NULL");
    const int D = dim_origin, k = dim_k, H = num_heads;
    const X16HeadsLayout L = x16_heads_layout(num_rows, num_cols, num_e, D, k, H, chunk_edges);
    if (int rc = x16_rec_check(L)) return rc;
    if (int rc = x16_ws_check(workspace, workspace_bytes, al256(L.rec_bytes))) return rc;
    MAXK_REQUIRE(((uintptr_t)cbsr_val & 3) == 0 && ((uintptr_t)cbsr_idx & 1) == 0 &&
                     ((uintptr_t)grad_out & 3) == 0 && ((uintptr_t)grad_edge & 3) == 0,
                 "float buffers must be 4-B aligned, cbsr_idx 2-B aligned");

    hipStream_t s = as_stream(stream);
    uint8_t *rec = reinterpret_cast<uint8_t *>(workspace);
    if (int rc = launch_x16_pack(cbsr_val, cbsr_idx, rec, num_cols, k, L.RS, D, L.DS - 1, s))
        return rc;
    const int rows = x16_rows_in_budget(L.DS), HP = H < rows ? H : rows;
    const int vec = D % 4 == 0 && ((uintptr_t)grad_out & 15) == 0;
    const int kg = x16_lanes(k, 8);
    const bool ok = with_const<8, 16, 32, 64>(kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        hipLaunchKernelGGL((x16_edge_grad_heads_kernel<KG, kX16HeadsU>), item_grid(L.n_items),
                           dim3(kBlock), (size_t)kWavesPerBlock * HP * L.DS * sizeof(float), s,
                           row_ptr, col_idx, rec, (uint32_t)L.rec_bytes, L.RS, grad_out, row_div,
                           grad_edge, (int)num_rows, num_e, D, L.DS, k, L.chunk, L.n_items, H, HP,
                           vec);
    });
    if (!ok) return bad_lanes(kg);
    MAXK_LAUNCHED("x16_edge_grad_heads_kernel");
    return MAXK_OK;
}

extern "C" size_t maxk_sspmm_backward_heads_x16_workspace_size(int64_t num_rows, int64_t num_cols,
                                                               int64_t num_e, int32_t dim_origin,
                                                               int32_t dim_k, int32_t num_heads,
                                                               int32_t chunk_edges) {
    if (!x16_heads_ok(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads, chunk_edges))
        return 0;
    return csc_sum_workspace_size(num_cols, num_e, dim_k, chunk_edges);
}

extern "C" int maxk_sspmm_backward_heads_x16(const int32_t *row_ptr, const int32_t *col_idx,
                                             const float *edge_val, const float *grad_out,
                                             const float *row_div, const uint16_t *cbsr_idx,
                                             const int32_t *col_ptr, const int32_t *csc_eid,
                                             float *grad_cbsr, int64_t num_rows, int64_t num_cols,
                                             int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                             int32_t num_heads, int32_t chunk_edges,
                                             void *workspace, size_t workspace_bytes,
                                             void *stream) {
    clear_error();
    if (int rc = x16_heads_check(num_rows, num_cols, num_e, dim_origin, dim_k, num_heads,
                                 chunk_edges))
        return rc;
    if (num_cols == 0) return MAXK_OK;
    MAXK_REQUIRE(grad_cbsr && col_ptr, "grad_cbsr/col_ptr must not be NULL");
    MAXK_REQUIRE(num_e == 0 || (row_ptr && col_idx && edge_val && grad_out && cbsr_idx && csc_eid),
                 "CSR/grad/selector/transpose pointers must not be NULL");
    const int D = dim_origin, k = dim_k, H = num_heads;
    if (int rc = x16_ws_check(workspace, workspace_bytes,
                              csc_sum_workspace_size(num_cols, num_e, k, chunk_edges)))
        return rc;
    MAXK_REQUIRE(((uintptr_t)edge_val & 3) == 0 && ((uintptr_t)grad_out & 3) == 0 &&
                     ((uintptr_t)cbsr_idx & 1) == 0,
                 "float buffers must be 4-B aligned, cbsr_idx 2-B aligned");
    hipStream_t s = as_stream(stream);
    if (num_e > 0 && num_rows > 0) {
        const int DS = x16_copy_stride(D);
        const int chunk = x16_chunk(num_rows, num_e, chunk_edges);
        const int n_items = token_items(num_rows, num_e, chunk);
        const int rows = x16_rows_in_budget(DS), HP = H < rows ? H : rows;
        const int vec = D % 4 == 0 && ((uintptr_t)grad_out & 15) == 0;
        const int kg = x16_lanes(k, 8);
        const bool ok = with_const<8, 16, 32, 64>(kg, [&](auto kg_c) {
            constexpr int KG = decltype(kg_c)::value;
            hipLaunchKernelGGL((x16_bwd_heads_kernel<KG, kX16HeadsU>), item_grid(n_items),
                               dim3(kBlock), (size_t)kWavesPerBlock * HP * DS * sizeof(float), s,
                               row_ptr, col_idx, edge_val, grad_out, row_div, cbsr_idx,
                               (uint32_t)(num_cols * k * 2), reinterpret_cast<float *>(workspace),
                               (int)num_rows, num_e, D, DS, k, chunk, n_items, H, HP, vec);
        });
        if (!ok) return bad_lanes(kg);
        MAXK_LAUNCHED("x16_bwd_heads_kernel");
    }
    return csc_sum_rows(s, col_ptr, csc_eid, workspace, grad_cbsr, num_cols, num_e, k, chunk_edges);
}
