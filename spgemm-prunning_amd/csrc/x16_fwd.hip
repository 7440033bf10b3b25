// Forward SpGEMM on 16-bit selectors, 1 <= D <= 1024:  out = diag(1/row_div) . A . scatter(CBSR)
//
// maxk_spgemm_forward's semantics (spgemm_fwd.hip) for rows too wide for its budgets: there a
// wave keeps up to eight LDS copies of a 256-float output row; at D = 1024 a copy is 4 KB, so
// the copies per wave are set by D, not by k.  DESIGN.md 5.20.
//
//  1. x16_pack_kernel: one record [k f32 | k u16 | pad] per source vertex (x16_pack.h), so an
//     edge gathers one run of lines; repeated selectors fold into their first occurrence, and a
//     folded or out-of-range slot names the trash column DS - 1 -- not a bit of the u16, every
//     bit below 1024 being a real column.
//  2. x16_fwd_kernel<KG, U>, one wave per item of the token stream (token_items.h, CutHubRows):
//     * NC = 64 / KG copies of the output row in LDS, DS = pad4(D) + 4 floats each: NC = 4 up
//       to D = 508 (8.3 KB per wave), 2 up to D = 1024 (8.2 KB), and 1 when k > 32 needs the
//       whole wave for one edge.  KG = max(pow2ceil(k), 64 / NC) lanes take one edge -- lanes
//       past k idle, as spgemm_fwd.hip's 16 lanes do at k <= 8 -- and for k > 64 a lane walks
//       slots l, l + 64, ...;
//     * U wave steps of (column, weight) and then of record loads in flight, all through buffer
//       descriptors (past a piece's end: column 0, weight 0, sent to the trash column);
//     * plain ds_read / ds_write accumulation: within a step a group's lanes hit distinct
//       columns (folded selectors) and groups hit different copies -- no LDS float atomics;
//     * a row lying whole in the item is stored once: copies summed in copy order, divided by
//       row_div, 16-B stores.  A hub row's continuation goes to the item's slab.
//  3. slab_fixup_kernel<0> (common.h, D-generic) adds the slabs of each split row in item order.
// No global atomics: bitwise repeatable.
#include "x16_pack.h"

namespace maxk {
namespace {

// One thread per (vertex, l), vpb = min(64, 256 / k) vertices per workgroup pass, grid-stride.
// A 1024-bit column set per vertex (atomicOr returns the bit already set) finds the vertices
// with a repeated selector; only those scan their selectors (rare: top-k output has none).
constexpr int kX16PackBlock = 256;
constexpr int kX16PackMaxV = 64;

__global__ __launch_bounds__(kX16PackBlock) void x16_pack_kernel(
    const float *__restrict__ cbsr_val, const uint16_t *__restrict__ cbsr_idx,
    uint8_t *__restrict__ rec, int num_cols, int k, int RS, int D, int trash) {
    __shared__ uint32_t s_bits[kX16PackMaxV * (kMaxDimX16 / 32)];
    __shared__ int s_dup[kX16PackMaxV];
    const int vpb = kX16PackBlock / k < kX16PackMaxV ? kX16PackBlock / k : kX16PackMaxV;
    const int t = threadIdx.x;
    const int vl = t / k, l = t - vl * k;
    for (int64_t g0 = (int64_t)blockIdx.x * vpb; g0 < num_cols; g0 += (int64_t)gridDim.x * vpb) {
        const int64_t v = g0 + vl;
        const bool act = vl < vpb && v < num_cols;
        for (int i = t; i < vpb * (kMaxDimX16 / 32); i += kX16PackBlock) s_bits[i] = 0u;
        if (t < vpb) s_dup[t] = 0;
        __syncthreads();
        uint32_t s = 0;
        float val = 0.f;
        bool in = false;
        if (act) {
            s = cbsr_idx[v * k + l];
            val = cbsr_val[v * k + l];
            in = s < (uint32_t)D;
            if (in) {
                const uint32_t old =
                    atomicOr(&s_bits[vl * (kMaxDimX16 / 32) + (s >> 5)], 1u << (s & 31));
                if ((old >> (s & 31)) & 1u) s_dup[vl] = 1;
            }
        }
        __syncthreads();
        if (act) {
            bool keep = in;
            if (in && s_dup[vl]) {  // the first occurrence sums its repeats in l order
                const uint16_t *ci = cbsr_idx + v * k;
                const float *cv = cbsr_val + v * k;
                for (int m = 0; m < l; ++m) keep = keep && ci[m] != s;
                if (keep)
                    for (int m = l + 1; m < k; ++m)
                        if (ci[m] == s) val += cv[m];
            }
            uint8_t *p = rec + v * RS;
            reinterpret_cast<float *>(p)[l] = keep ? val : 0.f;
            reinterpret_cast<uint16_t *>(p + 4 * k)[l] = (uint16_t)(keep ? s : (uint32_t)trash);
        }
        __syncthreads();  // LDS is reused by the next pass
    }
}

}  // namespace

int launch_x16_pack(const float *cbsr_val, const uint16_t *cbsr_idx, uint8_t *rec, int64_t num_cols,
                    int k, int RS, int D, int trash, hipStream_t s) {
    const int vpb = kX16PackBlock / k < kX16PackMaxV ? kX16PackBlock / k : kX16PackMaxV;
    const int64_t groups = ceil_div(num_cols, (int64_t)vpb);
    hipLaunchKernelGGL(x16_pack_kernel,
                       dim3((unsigned)(groups < MAXK_PACK_GRID ? groups : MAXK_PACK_GRID)),
                       dim3(kX16PackBlock), 0, s, cbsr_val, cbsr_idx, rec, (int)num_cols, k, RS, D,
                       trash);
    MAXK_LAUNCHED("x16_pack_kernel");
    return MAXK_OK;
}

namespace {

// acc_g[column] += val[e] * value over the edges [sb, se), sb < se; acc_g is the copy of this
// lane's edge group.  Lanes past k, and edges past se (the descriptors return column 0, weight
// 0), write the trash column: two lanes of a group never share a live address in one ds_write,
// and an idle lane's product never reaches a live column.
template <int KG, int U>
__device__ __forceinline__ void x16_walk(float *acc_g, const int32_t *__restrict__ col_idx,
                                         const float *__restrict__ edge_val,
                                         __amdgpu_buffer_rsrc_t rrs, int RS, int sb, int se, int k,
                                         int trash, int lane) {
    constexpr int G = kWave / KG;  // edges per wave step
    const int grp = lane / KG, l0 = lane % KG;
    const int n = se - sb;  // wave-uniform
    const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
    const auto vrs = wave_buffer(edge_val + sb, (uint32_t)n * 4u);
    for (int base = 0; base < n; base += G * U) {
        uint32_t ro[U];
        float w[U];
        const int lo = (base + grp) * 4;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ro[u] = __builtin_amdgcn_raw_buffer_load_b32(crs, lo + u * G * 4, 0, 0) * (uint32_t)RS;
            w[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vrs, lo + u * G * 4, 0, 0));
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
                const bool live = lok && base + u * G + grp < n;
                float *a = &acc_g[live ? min(s[u], trash) : trash];
                *a = __builtin_fmaf(w[u], v[u], *a);  // one rounding, as in spgemm_fwd.hip
            }
        }
    }
}

// dst[0:D] = (sum over the NC copies of acc[.][0:D]) / div; the copies are zeroed as they are
// read.  vec: D % 4 == 0 and dst 16-B aligned.
template <int NC>
__device__ __forceinline__ void x16_flush(float *acc, int DS, float *__restrict__ dst, int D,
                                          float div, bool scale, bool vec, int lane) {
    wave_lds_fence();
    if (vec) {
        for (int j = lane * 4; j < D; j += kWave * 4) {
            float4 a = *reinterpret_cast<float4 *>(&acc[j]);
            *reinterpret_cast<float4 *>(&acc[j]) = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int g = 1; g < NC; ++g) {
                float4 *pg = reinterpret_cast<float4 *>(&acc[g * DS + j]);
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
            *reinterpret_cast<float4 *>(&dst[j]) = a;
        }
    } else {
        for (int j = lane; j < D; j += kWave) {
            float a = 0.f;
#pragma unroll
            for (int g = 0; g < NC; ++g) {
                a += acc[g * DS + j];
                acc[g * DS + j] = 0.f;
            }
            dst[j] = scale ? a / div : a;
        }
    }
    wave_lds_fence();
}

template <int KG, int U>
__global__ __launch_bounds__(kBlock) void x16_fwd_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const float *__restrict__ edge_val, const uint8_t *__restrict__ rec, uint32_t rec_bytes, int RS,
    const float *__restrict__ row_div, float *__restrict__ out, float *__restrict__ slab,
    int32_t *__restrict__ slab_row, int num_rows, int64_t num_e, int D, int DS, int k, int chunk,
    int n_items, int vec) {
    constexpr int NC = kWave / KG;  // LDS copies per wave (one per edge group)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = lane_id();
    const int item = item_of_wave(n_items);
    if (item < 0) return;  // whole wave; no workgroup barrier below
    float *acc = lds + (size_t)(threadIdx.x / kWave) * NC * DS;
    for (int j = lane * 4; j < NC * DS; j += kWave * 4)
        *reinterpret_cast<float4 *>(&acc[j]) = make_float4(0.f, 0.f, 0.f, 0.f);
    float *acc_g = acc + (lane / KG) * DS;
    const int trash = DS - 1;
    // the record table: a load past it (a column out of range) returns 0
    const auto rrs = wave_buffer(rec, rec_bytes);
    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);
    const int64_t d1 = it.d1;
    int r = it.r;

    // the continuation of row r - 1: only a hub row (longer than an item) leaves one
    int cont = -1;
    if (r > 0) {
        const RowPiece p = cont_piece(CutHubRows{}, it.p_lo, d1, r, row_ptr[r - 1], row_ptr[r], chunk);
        if (p.sb < p.se && p.hub) {
            const float div = row_div ? row_div[r - 1] : 1.f;  // loaded before the walk
            wave_lds_fence();
            x16_walk<KG, U>(acc_g, col_idx, edge_val, rrs, RS, (int)p.sb, (int)p.se, k, trash, lane);
            x16_flush<NC>(acc, DS, slab + (int64_t)item * D, D, div, row_div != nullptr,
                          vec != 0, lane);
            cont = r - 1;
        }
    }
    if (lane == 0) slab_row[item] = cont;

    // the rows whose token lies in [d0, d1)
    for (; r < num_rows; ++r) {
        const int64_t rb = row_ptr[r];
        if (!row_owned(d1, r, rb)) break;
        const int64_t se = row_piece(CutHubRows{}, d1, r, rb, row_ptr[r + 1], chunk).se;
        const float div = row_div ? row_div[r] : 1.f;
        wave_lds_fence();
        if (rb < se)
            x16_walk<KG, U>(acc_g, col_idx, edge_val, rrs, RS, (int)rb, (int)se, k, trash, lane);
        x16_flush<NC>(acc, DS, out + (int64_t)r * D, D, div, row_div != nullptr, vec != 0, lane);
    }
}

struct X16FwdLayout {
    int chunk, n_items, RS, DS, kg;
    size_t rec_bytes, slab_off, row_off, total;
};

// KG: pow2ceil(k), at least 64 / (the copies D allows: 4 up to D = 508, else 2)
X16FwdLayout x16_fwd_layout(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k,
                            int chunk) {
    X16FwdLayout L{};
    L.RS = x16_record_stride(k);
    L.DS = x16_copy_stride(D);
    L.kg = x16_lanes(k, L.DS <= 512 ? 16 : 32);
    L.chunk = x16_chunk(num_rows, num_e, chunk);
    L.n_items = token_items(num_rows, num_e, L.chunk);
    const int64_t cap = x16_item_cap(num_rows + num_e, chunk, L.n_items);
    L.rec_bytes = (size_t)num_cols * L.RS;
    L.slab_off = al256(L.rec_bytes);
    L.row_off = L.slab_off + al256((size_t)cap * D * sizeof(float));
    L.total = L.row_off + al256((size_t)cap * sizeof(int32_t));
    return L;
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" size_t maxk_spgemm_forward_x16_workspace_size(int64_t num_rows, int64_t num_cols,
                                                         int64_t num_e, int32_t dim_origin,
                                                         int32_t dim_k, int32_t chunk_edges) {
    if (num_rows < 0 || num_cols < 0 || num_e < 0 || chunk_edges < 0 ||
        !x16_dims_ok(dim_origin, dim_k))
        return 0;
    return x16_fwd_layout(num_rows, num_cols, num_e, dim_origin, dim_k, chunk_edges).total;
}

extern "C" int maxk_spgemm_forward_x16(const int32_t *row_ptr, const int32_t *col_idx,
                                       const float *edge_val, const float *cbsr_val,
                                       const uint16_t *cbsr_idx, const float *row_div, float *out,
                                       int64_t num_rows, int64_t num_cols, int64_t num_e,
                                       int32_t dim_origin, int32_t dim_k, int32_t chunk_edges,
                                       void *workspace, size_t workspace_bytes, void *stream) {
    clear_error();
    if (int rc = x16_check_dims(dim_origin, dim_k)) return rc;
    MAXK_REQUIRE(num_rows >= 0 && num_rows < (1LL << 31), "num_rows out of range: %lld",
                 (long long)num_rows);
    MAXK_REQUIRE(num_cols >= 0 && num_cols < (1LL << 31), "num_cols out of range");
    MAXK_REQUIRE(num_e >= 0 && num_e < (1LL << 31), "num_e out of range: %lld", (long long)num_e);
    MAXK_REQUIRE(chunk_edges >= 0 && chunk_edges <= kMaxChunk, "chunk_edges must be in [0, 2^24]");
    MAXK_REQUIRE(num_cols * (int64_t)dim_k < (1LL << 31), "num_cols*k too large");
    if (num_rows == 0) return MAXK_OK;
    MAXK_REQUIRE(row_ptr && out, "row_ptr/out must not be NULL");
    MAXK_REQUIRE(num_e == 0 || (col_idx && edge_val && cbsr_val && cbsr_idx),
                 "CSR/CBSR pointers must not be NULL");
    MAXK_REQUIRE(num_e == 0 || num_cols > 0, "edges present but num_cols == 0");
    const int D = dim_origin, k = dim_k;
    const X16FwdLayout L = x16_fwd_layout(num_rows, num_cols, num_e, D, k, chunk_edges);
    MAXK_REQUIRE(L.rec_bytes < (1ull << 32),
                 "packed record table of %zu bytes: num_cols * %d must stay below 4 GiB",
                 L.rec_bytes, L.RS);
    MAXK_REQUIRE(workspace && workspace_bytes >= L.total,
                 "workspace too small: need %zu bytes, got %zu", L.total, workspace_bytes);
    MAXK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-B aligned");
    MAXK_REQUIRE(((uintptr_t)cbsr_val & 3) == 0 && ((uintptr_t)cbsr_idx & 1) == 0 &&
                     ((uintptr_t)out & 3) == 0,
                 "cbsr_val/out must be 4-B aligned, cbsr_idx 2-B aligned");

    char *ws = reinterpret_cast<char *>(workspace);
    uint8_t *rec = reinterpret_cast<uint8_t *>(ws);
    float *slab = reinterpret_cast<float *>(ws + L.slab_off);
    int32_t *slab_row = reinterpret_cast<int32_t *>(ws + L.row_off);
    hipStream_t s = as_stream(stream);
    if (num_cols > 0 && num_e > 0)
        if (int rc = launch_x16_pack(cbsr_val, cbsr_idx, rec, num_cols, k, L.RS, D, L.DS - 1, s))
            return rc;
    const int vec = D % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const bool ok = with_const<16, 32, 64>(L.kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        const size_t lds = (size_t)kWavesPerBlock * (kWave / KG) * L.DS * sizeof(float);
        hipLaunchKernelGGL((x16_fwd_kernel<KG, 8>), item_grid(L.n_items), dim3(kBlock), lds, s,
                           row_ptr, col_idx, edge_val, rec, (uint32_t)L.rec_bytes, L.RS, row_div,
                           out, slab, slab_row, (int)num_rows, num_e, D, L.DS, k, L.chunk,
                           L.n_items, vec);
    });
    if (!ok) return bad_lanes(L.kg);
    MAXK_LAUNCHED("x16_fwd_kernel");
    return launch_slab_fixup<0>(slab, slab_row, out, D, L.n_items, s);
}
