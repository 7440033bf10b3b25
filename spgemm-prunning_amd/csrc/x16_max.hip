// Max aggregation on 16-bit selectors, 1 <= D <= 1024: maxk_spgemm_max_forward / _backward's
// semantics (maxk_hip.h; spgemm_max.hip serves D <= 256 on 8-bit selectors) for rows too wide for
// a u8 selector, with a backward of its own.  DESIGN.md 5.21.
//
// Forward.
//  1. x16_max_pack_kernel: the x16 record [k f32 | k u16 | pad] per source vertex (x16_pack.h;
//     x16_fwd.hip's pack is local to that file, so the same layout is packed here).  A repeated
//     selector folds into its first occurrence (fp32 sum in l order); a folded or >= D slot names
//     the trash column DS - 1, which no flush reads: the walk has no branch on it, and bit 0x100
//     of a selector is a column like any other.
//  2. x16_max_fwd_kernel<KG, U>: one wave per item of the token stream (token_items.h) under the
//     hub-row cut, KG = pow2ceil(k) lanes per edge (8 .. 64; past 64 slots a lane walks l, l + 64,
//     ...), U wave steps of column and then of record loads in flight through buffer descriptors.
//     The wave keeps ONE row of DS = pad4(D) + 4 64-bit keys in LDS and every candidate enters
//     it with a 64-bit LDS maximum; a 32-bit word per column counts the candidates.  12 * DS bytes
//     per wave: 12,336 B at D = 1024, 49,344 B per workgroup, three workgroups per CU.
//       key = order-preserving value bits << 32 | (0x7fffffff - edge) << 1 | sign of a zero
//     as spgemm_max.hip states it (its two key functions are file-local there and restated below;
//     tests/test_x16_max_gpu.py holds the two paths to the same bytes at D <= 256): the unsigned
//     maximum of the keys is the rule's first-largest candidate in any arrival order, a column
//     fewer edges kept than the piece has takes the implicit +0.0 as one more key, key 0 is a row
//     without edges.  The flush decodes four columns per lane and stores 16 B of out and of arg.
//  3. x16_max_fixup_kernel: a hub row cut over items leaves one key row per piece; their unsigned
//     maximum is the row's, in any order -- out and arg do not depend on the item size.
//
// Backward, the two-phase csc form (x16_bwd.hip's, with arg as the mask):
//  1. x16_max_bwd_kernel<KG, U>: one wave per item under CutAtEnd (walk_cut_item).  For every row
//     piece the wave stages grad_out[r, :] and arg[r, :] in LDS (8 * DS bytes per wave) with 16-B
//     loads, then lane groups of KG lanes take one edge each, U wave steps in flight: the group
//     reads its destination's k contiguous u16 selectors and stores the contribution row
//       T[e, l] = (s < D && arg_row[s] == e) ? g_row[s] : 0
//     past the caches.  The E * k look-ups of arg are LDS reads; the mask is a select, so a NaN
//     of grad_out whose arg names another edge gives an exact 0.
//  2. csc_sum_rows (sspmm_push.hip through sspmm_bwd.h) unchanged: each destination's rows summed
//     in CSC slot order.  No atomics in global memory, bitwise repeatable; a slot that never won
//     sums exact zeros.
#include "heads_walk.h"
#include "sspmm_bwd.h"
#include "x16_pack.h"

namespace maxk {
namespace {

constexpr uint32_t kNanValue = 0xffffffffu;   // every NaN: above +Inf (0xff800000)
constexpr uint32_t kZeroValue = 0x80000000u;  // both zeros
constexpr uint32_t kNoEdge = 0x7fffffffu;     // the implicit zero's position: past every edge
constexpr uint64_t kImplicitKey = (uint64_t)kZeroValue << 32;

__device__ __forceinline__ uint64_t max_key(float v, int e) {
    const uint32_t b = __float_as_uint(v);
    uint32_t hi, neg0 = 0u;
    if ((b & 0x7fffffffu) > 0x7f800000u) {
        hi = kNanValue;
    } else if ((b << 1) == 0u) {
        hi = kZeroValue;
        neg0 = b >> 31;
    } else {
        hi = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    return ((uint64_t)hi << 32) | (uint64_t)(((kNoEdge - (uint32_t)e) << 1) | neg0);
}

// The winner's bits and edge; -1 for the implicit zero and for no candidate at all.
__device__ __forceinline__ void max_decode(uint64_t key, float &o, int &a) {
    const uint32_t hi = (uint32_t)(key >> 32), lo = (uint32_t)key;
    const uint32_t pos = lo >> 1;
    uint32_t b = (hi & 0x80000000u) ? (hi & 0x7fffffffu) : ~hi;
    if (hi == kNanValue) b = 0x7fc00000u;
    if (hi == kZeroValue) b = lo << 31;
    if (key == 0ull) b = 0u;
    o = __uint_as_float(b);
    a = pos == 0u ? -1 : (int)(kNoEdge - pos);
}

// ---- forward ------------------------------------------------------------------------------------

// One thread per (vertex, l), vpb = min(64, 256 / k) vertices per workgroup pass, grid-stride.  A
// 1024-bit column set per vertex finds the vertices with a repeated selector; only those scan
// their selectors (top-k output has none).
constexpr int kX16MaxPackBlock = 256;
constexpr int kX16MaxPackV = 64;

__global__ __launch_bounds__(kX16MaxPackBlock) void x16_max_pack_kernel(
    const float *__restrict__ cbsr_val, const uint16_t *__restrict__ cbsr_idx,
    uint8_t *__restrict__ rec, int num_cols, int k, int RS, int D, int trash) {
    __shared__ uint32_t s_bits[kX16MaxPackV * (kMaxDimX16 / 32)];
    __shared__ int s_dup[kX16MaxPackV];
    const int vpb = kX16MaxPackBlock / k < kX16MaxPackV ? kX16MaxPackBlock / k : kX16MaxPackV;
    const int t = threadIdx.x;
    const int vl = t / k, l = t - vl * k;
    for (int64_t g0 = (int64_t)blockIdx.x * vpb; g0 < num_cols; g0 += (int64_t)gridDim.x * vpb) {
        const int64_t v = g0 + vl;
        const bool act = vl < vpb && v < num_cols;
        for (int i = t; i < vpb * (kMaxDimX16 / 32); i += kX16MaxPackBlock) s_bits[i] = 0u;
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

// slab: key rows [2 * cap, D], the continuation of item i at row i, the cut first piece of the
// hub row it owns at row cap + i; cont_row / first_row [cap] name the rows (-1: none).
// LDS of a wave: DS keys, then DS candidate counts.
template <int KG, int U>
__global__ __launch_bounds__(kBlock) void x16_max_fwd_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const uint8_t *__restrict__ rec, uint32_t rec_bytes, int RS, float *__restrict__ out,
    int32_t *__restrict__ arg, unsigned long long *__restrict__ slab, int64_t cap,
    int32_t *__restrict__ cont_row, int32_t *__restrict__ first_row, int num_rows, int64_t num_e,
    int D, int DS, int k, int chunk, int n_items, int vec) {
    constexpr int G = kWave / KG;  // edges per wave step
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds_keys[];
    const int lane = lane_id();
    const int item = item_of_wave(n_items);
    if (item < 0) return;  // whole wave; no workgroup barrier below
    char *mine = reinterpret_cast<char *>(lds_keys) + (size_t)(threadIdx.x / kWave) * DS * 12;
    unsigned long long *key = reinterpret_cast<unsigned long long *>(mine);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(mine + (size_t)DS * 8);
    for (int j = lane; j < DS; j += kWave) {
        key[j] = 0ull;
        cnt[j] = 0u;
    }
    wave_lds_fence();
    const int grp = lane / KG, l0 = lane % KG;
    const int trash = DS - 1;
    // the record table: a load past it (a column out of range) returns 0
    const auto rrs = wave_buffer(rec, rec_bytes);
    if (lane == 0) first_row[item] = -1;

    // column j of the piece's key row: read and cleared; fewer candidates than edges: the
    // implicit +0.0 competes
    auto take = [&](int j, int n) {
        unsigned long long kk = key[j];
        const uint32_t cc = cnt[j];
        key[j] = 0ull;
        cnt[j] = 0u;
        if (cc < (uint32_t)n && kk < kImplicitKey) kk = kImplicitKey;
        return kk;
    };

    auto piece = [&](int row, int64_t sb, int64_t se, bool whole, bool owned) {
        const int n = (int)(se - sb);  // wave-uniform, at most 2 * chunk
        if (n > 0) {
            const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
            for (int base = 0; base < n; base += G * U) {
                uint32_t ro[U];
                const int lo = (base + grp) * 4;
#pragma unroll
                for (int u = 0; u < U; ++u)  // past the piece's end: column 0, never entered
                    ro[u] = __builtin_amdgcn_raw_buffer_load_b32(crs, lo + u * G * 4, 0, 0) *
                            (uint32_t)RS;
                for (int lb = 0; lb < k; lb += KG) {  // one pass unless k > 64
                    const int l = lb + l0;
                    const bool lok = l < k;
                    const uint32_t lc = (uint32_t)(lok ? l : k - 1);  // no load leaves the record
                    const uint32_t vo = 4u * lc, so = 4u * (uint32_t)k + 2u * lc;
                    float v[U];
                    int s[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        v[u] = __uint_as_float(
                            __builtin_amdgcn_raw_buffer_load_b32(rrs, (int)(ro[u] + vo), 0, 0));
                        s[u] = (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(
                            rrs, (int)(ro[u] + so), 0, 0);
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int ei = base + u * G + grp;
                        if (lok && ei < n) {  // a folded or >= D slot names the trash column
                            const int c = min(s[u], trash);
                            atomicMax(&key[c], (unsigned long long)max_key(v[u], (int)sb + ei));
                            atomicAdd(&cnt[c], 1u);
                        }
                    }
                }
            }
        }
        wave_lds_fence();
        if (whole && owned) {
            float *o = out + (int64_t)row * D;
            int32_t *a = arg ? arg + (int64_t)row * D : nullptr;
            if (vec) {  // D % 4 == 0, out and arg 16-B aligned
                for (int j = lane * 4; j < D; j += kWave * 4) {
                    float4 of;
                    int4 af;
                    max_decode(take(j, n), of.x, af.x);
                    max_decode(take(j + 1, n), of.y, af.y);
                    max_decode(take(j + 2, n), of.z, af.z);
                    max_decode(take(j + 3, n), of.w, af.w);
                    *reinterpret_cast<float4 *>(o + j) = of;
                    if (a) *reinterpret_cast<int4 *>(a + j) = af;
                }
            } else {
                for (int j = lane; j < D; j += kWave) {
                    float of;
                    int af;
                    max_decode(take(j, n), of, af);
                    o[j] = of;
                    if (a) a[j] = af;
                }
            }
        } else {
            unsigned long long *sl = slab + ((owned ? cap : 0) + item) * (int64_t)D;
            for (int j = lane; j < D; j += kWave) sl[j] = take(j, n);
        }
        wave_lds_fence();
        if (owned && !whole && lane == 0) first_row[item] = row;
    };
    walk_hub_item(row_ptr, cont_row, num_rows, num_e, item, chunk, lane, piece);
}

// The merge of a hub row's pieces, 16 lanes per item: the group of the item that owns a hub row
// takes the maximum of its first piece and of the continuations in the items after it, and
// stores the winner.
__global__ __launch_bounds__(kBlock) void x16_max_fixup_kernel(
    const unsigned long long *__restrict__ slab, int64_t cap, const int32_t *__restrict__ cont_row,
    const int32_t *__restrict__ first_row, float *__restrict__ out, int32_t *__restrict__ arg,
    int D, int n_items) {
    const int item = (int)((blockIdx.x * (int64_t)kBlock + threadIdx.x) / 16);
    const int g = threadIdx.x % 16;
    if (item >= n_items) return;
    const int row = first_row[item];
    if (row < 0) return;
    int n = 0;
    while (item + 1 + n < n_items && cont_row[item + 1 + n] == row) ++n;
    const unsigned long long *first = slab + (cap + item) * (int64_t)D;
    const unsigned long long *cont = slab + (int64_t)(item + 1) * D;
    for (int j = g; j < D; j += 16) {
        unsigned long long kk = first[j];
        for (int i = 0; i < n; ++i) {
            const unsigned long long c = cont[(int64_t)i * D + j];
            kk = c > kk ? c : kk;
        }
        float o;
        int a;
        max_decode(kk, o, a);
        out[(int64_t)row * D + j] = o;
        if (arg) arg[(int64_t)row * D + j] = a;
    }
}

__global__ void x16_max_fill_kernel(int32_t *__restrict__ p, int64_t n, int32_t v) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}

// ---- backward, phase 1 --------------------------------------------------------------------------

// LDS of a wave: DS floats of grad_out[r, :], then DS words of arg[r, :].
template <int KG, int U>
__global__ __launch_bounds__(kBlock) void x16_max_bwd_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const int32_t *__restrict__ arg, const float *__restrict__ grad,
    const uint16_t *__restrict__ cbsr_idx, uint32_t idx_bytes, float *__restrict__ T, int num_rows,
    int64_t num_e, int D, int DS, int k, int chunk, int n_items, int vec) {
    constexpr int G = kWave / KG;  // edges per wave step
    extern __shared__ __attribute__((aligned(16))) float lds_rows[];
    const int lane = lane_id();
    const int item = item_of_wave(n_items);
    if (item < 0) return;  // whole wave; no workgroup barrier below
    float *grow = lds_rows + (size_t)(threadIdx.x / kWave) * 2 * DS;
    int32_t *arow = reinterpret_cast<int32_t *>(grow + DS);
    const int grp = lane / KG, l0 = lane % KG;
    // the selector table: a load past it (a column out of range) returns 0
    const auto irs = wave_buffer(cbsr_idx, idx_bytes);
    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);
    walk_cut_item(row_ptr, num_rows, it, [&](int q, int64_t sb, int64_t se, int64_t, bool) {
        if (sb >= se) return;
        const float *g = grad + (int64_t)q * D;
        const int32_t *a = arg + (int64_t)q * D;
        wave_lds_fence();  // the previous piece's picks are done
        if (vec) {         // D % 4 == 0, grad_out and arg 16-B aligned
            for (int j = lane * 4; j < D; j += kWave * 4) {
                *reinterpret_cast<float4 *>(grow + j) = *reinterpret_cast<const float4 *>(g + j);
                *reinterpret_cast<int4 *>(arow + j) = *reinterpret_cast<const int4 *>(a + j);
            }
        } else {
            for (int j = lane; j < D; j += kWave) {
                grow[j] = g[j];
                arow[j] = a[j];
            }
        }
        wave_lds_fence();
        const int n = (int)(se - sb);  // wave-uniform, at most chunk
        const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
        float *Tp = T + (size_t)sb * k;
        for (int base = 0; base < n; base += G * U) {
            uint32_t io[U];
            const int lo = (base + grp) * 4;
#pragma unroll
            for (int u = 0; u < U; ++u)
                io[u] = __builtin_amdgcn_raw_buffer_load_b32(crs, lo + u * G * 4, 0, 0) *
                        (uint32_t)k * 2u;
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
                    const int sc = s[u] < D ? s[u] : 0;
                    const bool won = s[u] < D && arow[sc] == (int)sb + e;
                    const float x = won ? grow[sc] : 0.f;  // a select: a masked NaN gives 0
                    if (lok && e < n)  // contribution rows streamed past the caches
                        __builtin_nontemporal_store(x, Tp + (size_t)e * k + l);
                }
            }
        }
    });
}

// ---- host ---------------------------------------------------------------------------------------

// The auto item size.  An item costs two key rows of the slab, 16 * D bytes: the items are
// x16_chunk's (about eight per resident wave slot) until their slabs would pass the record
// table's bytes or kSlabFloor, whichever is larger; from there the items grow instead.
constexpr size_t kSlabFloor = 32u << 20;

struct X16MaxLayout {
    int chunk, n_items, RS, DS, kg;
    int64_t cap;
    size_t rec_bytes, slab_off, cont_off, first_off, total;
};

X16MaxLayout x16_max_layout(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k,
                            int chunk) {
    X16MaxLayout L{};
    L.RS = x16_record_stride(k);
    L.DS = x16_copy_stride(D);
    L.kg = x16_lanes(k, 8);
    L.rec_bytes = (size_t)num_cols * L.RS;
    const int64_t tokens = num_rows + num_e;
    if (chunk > 0) {
        L.chunk = chunk;
        L.n_items = token_items(num_rows, num_e, chunk);
        L.cap = L.n_items;
    } else {
        const int64_t budget =
            (int64_t)((L.rec_bytes > kSlabFloor ? L.rec_bytes : kSlabFloor) / (16 * (size_t)D));
        const int c0 = x16_chunk(num_rows, num_e, 0);
        const int64_t need = ceil_div(tokens, budget);
        L.chunk = need > c0 ? (int)need : c0;
        L.n_items = token_items(num_rows, num_e, L.chunk);
        // non-decreasing in the token count, and at least the item count (x16_item_cap)
        const int64_t cap0 = x16_item_cap(tokens, 0, token_items(num_rows, num_e, c0));
        L.cap = cap0 < budget ? cap0 : budget;
        if (L.cap < L.n_items) L.cap = L.n_items;
    }
    L.slab_off = al256(L.rec_bytes);
    L.cont_off = L.slab_off + al256((size_t)L.cap * 2 * D * sizeof(uint64_t));
    L.first_off = L.cont_off + al256((size_t)L.cap * sizeof(int32_t));
    L.total = L.first_off + al256((size_t)L.cap * sizeof(int32_t));
    return L;
}

int x16_max_check_sizes(int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t D, int32_t k,
                        int32_t chunk) {
    if (int rc = x16_check_dims(D, k)) return rc;
    MAXK_REQUIRE(num_rows >= 0 && num_rows < (1LL << 31), "num_rows out of range: %lld",
                 (long long)num_rows);
    MAXK_REQUIRE(num_cols >= 0 && num_cols < (1LL << 31), "num_cols out of range: %lld",
                 (long long)num_cols);
    MAXK_REQUIRE(num_e >= 0 && num_e < (int64_t)kNoEdge, "num_e out of range: %lld",
                 (long long)num_e);
    MAXK_REQUIRE(chunk >= 0 && chunk <= kMaxChunk, "chunk_edges must be in [0, 2^24]");
    MAXK_REQUIRE(num_cols * (int64_t)k < (1LL << 31), "num_cols*k too large");
    return MAXK_OK;
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" size_t maxk_spgemm_max_forward_x16_workspace_size(int64_t num_rows, int64_t num_cols,
                                                             int64_t num_e, int32_t dim_origin,
                                                             int32_t dim_k, int32_t chunk_edges) {
    if (num_rows < 0 || num_cols < 0 || num_e < 0 || chunk_edges < 0 ||
        !x16_dims_ok(dim_origin, dim_k))
        return 0;
    return x16_max_layout(num_rows, num_cols, num_e, dim_origin, dim_k, chunk_edges).total;
}

extern "C" int maxk_spgemm_max_forward_x16(const int32_t *row_ptr, const int32_t *col_idx,
                                           const float *cbsr_val, const uint16_t *cbsr_idx,
                                           float *out, int32_t *arg, int64_t num_rows,
                                           int64_t num_cols, int64_t num_e, int32_t dim_origin,
                                           int32_t dim_k, int32_t chunk_edges, void *workspace,
                                           size_t workspace_bytes, void *stream) {
    clear_error();
    if (int rc = x16_max_check_sizes(num_rows, num_cols, num_e, dim_origin, dim_k, chunk_edges))
        return rc;
    if (num_rows == 0) return MAXK_OK;
    MAXK_REQUIRE(row_ptr && out, "row_ptr / out must not be NULL");
    MAXK_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)arg & 3) == 0,
                 "out / arg must be 4-B aligned");
    const int D = dim_origin, k = dim_k;
    hipStream_t s = as_stream(stream);
    if (num_e == 0) {
        if (int rc = zero_words(out, num_rows * D, s)) return rc;
        if (arg) {
            const int64_t n = num_rows * D, blocks = ceil_div(n, kBlock);
            hipLaunchKernelGGL(x16_max_fill_kernel,
                               dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kBlock), 0, s,
                               arg, n, -1);
            MAXK_LAUNCHED("x16_max_fill_kernel");
        }
        return MAXK_OK;
    }
    MAXK_REQUIRE(col_idx && cbsr_val && cbsr_idx, "col_idx / cbsr_val / cbsr_idx must not be NULL");
    MAXK_REQUIRE(num_cols > 0, "edges present but num_cols == 0");
    MAXK_REQUIRE(((uintptr_t)cbsr_val & 3) == 0 && ((uintptr_t)cbsr_idx & 1) == 0,
                 "cbsr_val must be 4-B aligned, cbsr_idx 2-B aligned");
    const X16MaxLayout L = x16_max_layout(num_rows, num_cols, num_e, D, k, chunk_edges);
    MAXK_REQUIRE(L.rec_bytes < (1ull << 32),
                 "packed record table of %zu bytes: num_cols * %d must stay below 4 GiB",
                 L.rec_bytes, L.RS);
    MAXK_REQUIRE(workspace && workspace_bytes >= L.total,
                 "workspace too small: need %zu bytes, got %zu", L.total,
                 workspace ? workspace_bytes : (size_t)0);
    MAXK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-B aligned");

    char *ws = reinterpret_cast<char *>(workspace);
    uint8_t *rec = reinterpret_cast<uint8_t *>(ws);
    unsigned long long *slab = reinterpret_cast<unsigned long long *>(ws + L.slab_off);
    int32_t *cont_row = reinterpret_cast<int32_t *>(ws + L.cont_off);
    int32_t *first_row = reinterpret_cast<int32_t *>(ws + L.first_off);
    const int vpb = kX16MaxPackBlock / k < kX16MaxPackV ? kX16MaxPackBlock / k : kX16MaxPackV;
    const int64_t groups = ceil_div(num_cols, (int64_t)vpb);
    hipLaunchKernelGGL(x16_max_pack_kernel,
                       dim3((unsigned)(groups < MAXK_PACK_GRID ? groups : MAXK_PACK_GRID)),
                       dim3(kX16MaxPackBlock), 0, s, cbsr_val, cbsr_idx, rec, (int)num_cols, k,
                       L.RS, D, L.DS - 1);
    MAXK_LAUNCHED("x16_max_pack_kernel");
    const int vec = D % 4 == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)arg & 15) == 0;
    const bool ok = with_const<8, 16, 32, 64>(L.kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        hipLaunchKernelGGL((x16_max_fwd_kernel<KG, 8>), item_grid(L.n_items), dim3(kBlock),
                           (size_t)kWavesPerBlock * L.DS * 12, s, row_ptr, col_idx, rec,
                           (uint32_t)L.rec_bytes, L.RS, out, arg, slab, L.cap, cont_row, first_row,
                           (int)num_rows, num_e, D, L.DS, k, L.chunk, L.n_items, vec);
    });
    if (!ok) return bad_lanes(L.kg);
    MAXK_LAUNCHED("x16_max_fwd_kernel");
    hipLaunchKernelGGL(x16_max_fixup_kernel, dim3((unsigned)ceil_div(L.n_items, kBlock / 16)),
                       dim3(kBlock), 0, s, slab, L.cap, cont_row, first_row, out, arg, D,
                       L.n_items);
    MAXK_LAUNCHED("x16_max_fixup_kernel");
    return MAXK_OK;
}

extern "C" size_t maxk_spgemm_max_backward_x16_workspace_size(int64_t num_rows, int64_t num_cols,
                                                              int64_t num_e, int32_t dim_origin,
                                                              int32_t dim_k, int32_t chunk_edges) {
    if (num_rows < 0 || num_cols < 0 || num_e < 0 || chunk_edges < 0 ||
        !x16_dims_ok(dim_origin, dim_k))
        return 0;
    return csc_sum_workspace_size(num_cols, num_e, dim_k, chunk_edges);
}

extern "C" int maxk_spgemm_max_backward_x16(const int32_t *row_ptr, const int32_t *col_idx,
                                            const int32_t *col_ptr, const int32_t *csc_eid,
                                            const uint16_t *cbsr_idx, const int32_t *arg,
                                            const float *grad_out, float *grad_cbsr,
                                            int64_t num_rows, int64_t num_cols, int64_t num_e,
                                            int32_t dim_origin, int32_t dim_k, int32_t chunk_edges,
                                            void *workspace, size_t workspace_bytes, void *stream) {
    clear_error();
    if (int rc = x16_max_check_sizes(num_rows, num_cols, num_e, dim_origin, dim_k, chunk_edges))
        return rc;
    if (num_cols == 0) return MAXK_OK;
    MAXK_REQUIRE(grad_cbsr && col_ptr, "grad_cbsr / col_ptr must not be NULL");
    MAXK_REQUIRE(num_e == 0 || (row_ptr && col_idx && csc_eid && cbsr_idx && arg && grad_out),
                 "row_ptr / col_idx / csc_eid / cbsr_idx / arg / grad_out must not be NULL");
    MAXK_REQUIRE(num_e == 0 || num_rows > 0, "edges present but num_rows == 0");
    const size_t need = csc_sum_workspace_size(num_cols, num_e, dim_k, chunk_edges);
    MAXK_REQUIRE(workspace && workspace_bytes >= need,
                 "workspace too small: need %zu bytes, got %zu", need,
                 workspace ? workspace_bytes : (size_t)0);
    MAXK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-B aligned");
    MAXK_REQUIRE(((uintptr_t)grad_cbsr & 3) == 0 && ((uintptr_t)grad_out & 3) == 0 &&
                     ((uintptr_t)arg & 3) == 0 && ((uintptr_t)cbsr_idx & 1) == 0,
                 "grad_cbsr / grad_out / arg must be 4-B aligned, cbsr_idx 2-B aligned");
    hipStream_t s = as_stream(stream);
    const int D = dim_origin, k = dim_k;
    if (num_e > 0) {
        const int DS = x16_copy_stride(D);
        const int chunk = x16_chunk(num_rows, num_e, chunk_edges);
        const int n_items = token_items(num_rows, num_e, chunk);
        const int vec = D % 4 == 0 && ((uintptr_t)grad_out & 15) == 0 && ((uintptr_t)arg & 15) == 0;
        const int kg = x16_lanes(k, 8);
        const bool ok = with_const<8, 16, 32, 64>(kg, [&](auto kg_c) {
            constexpr int KG = decltype(kg_c)::value;
            hipLaunchKernelGGL((x16_max_bwd_kernel<KG, 4>), item_grid(n_items), dim3(kBlock),
                               (size_t)kWavesPerBlock * 2 * DS * sizeof(float), s, row_ptr,
                               col_idx, arg, grad_out, cbsr_idx, (uint32_t)(num_cols * dim_k * 2),
                               reinterpret_cast<float *>(workspace), (int)num_rows, num_e, D, DS,
                               k, chunk, n_items, vec);
        });
        if (!ok) return bad_lanes(kg);
        MAXK_LAUNCHED("x16_max_bwd_kernel");
    }
    return csc_sum_rows(s, col_ptr, csc_eid, workspace, grad_cbsr, num_cols, num_e, k, chunk_edges);
}
