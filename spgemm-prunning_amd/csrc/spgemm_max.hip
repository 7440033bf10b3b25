// Max aggregation on CBSR features: out[r, j] = max over the edges of row r of
// scatter(CBSR)[col_idx[e], j], arg[r, j] the winning CSR edge (maxk_hip.h has the rules), and
// its backward.
//
// Forward.  One wavefront per item of the token stream (token_items.h) under the hub-row cut
// rule, KG = pow2ceil(k) lanes per edge (at most a wave), one packed record gathered per edge
// (cbsr_pack.h), U wave steps of gathers in flight.  The wave keeps ONE copy of the row in LDS,
// a 64-bit key per column, and every candidate goes into it with a 64-bit LDS max:
//
//   key = order-preserving value bits << 32 | (0x7fffffff - edge) << 1 | sign of a zero
//
// The value bits order as the floats do (a negative float's bits inverted, a positive one's sign
// set); -0.0 and +0.0 share one value (the strict `>` of the rule ties them) and the low bit
// keeps the winner's sign; every NaN maps to the largest value, so a NaN beats everything.  Among
// equal values the larger inverted position, the lower edge, wins: the unsigned maximum of the
// keys IS the rule's first-largest candidate, whatever order the candidates arrive in.  A second
// LDS word per column counts the candidates; a column fewer edges kept than the piece has takes
// the implicit +0.0 as one more key -- value +0.0 at the position past every edge, so an explicit
// zero of either sign beats it and it wins exactly when 0 > best, or alone.  Key 0 is "nothing":
// a row without edges.
// A hub row cut over items leaves one key row per piece (the owner's in the item's `first` slab,
// each continuation in its `cont` slab); max_fixup_kernel takes their maximum.  Since the keys
// carry the global edge index the merge needs no order, and out and arg do not depend on the item
// size, on where a row is cut or on the order the LDS served the lanes.
//
// Backward.  slot_row_kernel finds the row of every CSC slot's edge (a binary search of row_ptr,
// into the workspace); max_bwd_kernel gives each column a lane group over its slots l, walks the
// column's CSC slots in order and adds grad_out[r, j] where arg[r, j] names the slot's edge:
// E * k gathers of arg, one fp32 sum per (c, l) in CSC slot order, no atomics.
#include "spgemm_max.h"

#include "heads_walk.h"

namespace maxk {
namespace {

constexpr uint32_t kNanValue = 0xffffffffu;   // every NaN: above +Inf (0xff800000)
constexpr uint32_t kZeroValue = 0x80000000u;  // both zeros
constexpr uint32_t kNoEdge = 0x7fffffffu;     // the implicit zero's position: past every edge
constexpr uint64_t kImplicitKey = (uint64_t)kZeroValue << 32;
#ifndef MAXK_MAX_U  // wave steps of record gathers in flight (4 / 8 / 16 timed:
#define MAXK_MAX_U 8  // profiles/r23/max_aggregate/)
#endif
constexpr int kMaxU = MAXK_MAX_U;

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

// slab: key rows [2 * cap, D], the continuation of item i at row i, the cut first piece of the
// hub row it owns at row cap + i; cont_row / first_row [cap] name the rows (-1: none).
__global__ __launch_bounds__(kBlock) void max_fwd_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const uint8_t *__restrict__ rec, uint32_t rec_bytes, int RS, float *__restrict__ out,
    int32_t *__restrict__ arg, unsigned long long *__restrict__ slab, int64_t cap,
    int32_t *__restrict__ cont_row, int32_t *__restrict__ first_row, int num_rows, int64_t num_e,
    int D, int k, int kgs, int chunk, int n_items) {
    __shared__ unsigned long long s_key[kWavesPerBlock][kMaxDim];
    __shared__ uint32_t s_cnt[kWavesPerBlock][kMaxDim];
    const int item = item_of_wave(n_items);
    if (item < 0) return;
    const int lane = lane_id();
    unsigned long long *key = s_key[threadIdx.x / kWave];
    uint32_t *cnt = s_cnt[threadIdx.x / kWave];
    for (int j = lane; j < D; j += kWave) {
        key[j] = 0ull;
        cnt[j] = 0u;
    }
    wave_lds_fence();
    const int KG = 1 << kgs, EP = kWave >> kgs;  // lanes per edge, edges per wave step
    const int grp = lane >> kgs, l0 = lane & (KG - 1);
    const __amdgpu_buffer_rsrc_t rrs = wave_buffer(rec, rec_bytes);
    if (lane == 0) first_row[item] = -1;

    auto piece = [&](int row, int64_t sb, int64_t se, bool whole, bool owned) {
        const int n = (int)(se - sb);
        for (int base = 0; base < n; base += kMaxU * EP) {
            int c[kMaxU], e[kMaxU];
#pragma unroll
            for (int u = 0; u < kMaxU; ++u) {
                const int ei = base + u * EP + grp;
                e[u] = (int)sb + ei;
                c[u] = ei < n ? col_idx[e[u]] : 0;
            }
            for (int lb = 0; lb < k; lb += KG) {
                const RecordSlot slot(lb + l0, k);
                const bool lok = slot.ok;
                const PackedSrc src = slot.src(rrs, k, RS);
                float v[kMaxU];
                int s[kMaxU];
#pragma unroll
                for (int u = 0; u < kMaxU; ++u) src.load(c[u], v[u], s[u]);
#pragma unroll
                for (int u = 0; u < kMaxU; ++u) {
                    // a folded or out-of-range selector is stored as 0x100 | s: no candidate
                    if (lok && base + u * EP + grp < n && s[u] < 0x100) {
                        atomicMax(&key[s[u]], (unsigned long long)max_key(v[u], e[u]));
                        atomicAdd(&cnt[s[u]], 1u);
                    }
                }
            }
        }
        wave_lds_fence();
        const bool direct = whole && owned;
        unsigned long long *sl = slab + ((owned ? cap : 0) + item) * (int64_t)D;
        for (int j = lane; j < D; j += kWave) {
            unsigned long long kk = key[j];
            const uint32_t cc = cnt[j];
            key[j] = 0ull;
            cnt[j] = 0u;
            if (cc < (uint32_t)n && kk < kImplicitKey) kk = kImplicitKey;
            if (direct) {
                float o;
                int a;
                max_decode(kk, o, a);
                out[(int64_t)row * D + j] = o;
                if (arg) arg[(int64_t)row * D + j] = a;
            } else {
                sl[j] = kk;
            }
        }
        wave_lds_fence();
        if (owned && !whole && lane == 0) first_row[item] = row;
    };
    walk_hub_item(row_ptr, cont_row, num_rows, num_e, item, chunk, lane, piece);
}

// The merge of a hub row's pieces, 16 lanes per item as slab_fixup_kernel: the group of the item
// that owns a hub row takes the maximum of its first piece and of the continuations in the items
// after it, and stores the winner.
__global__ __launch_bounds__(kBlock) void max_fixup_kernel(
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

__global__ void fill_words_kernel(int32_t *__restrict__ p, int64_t n, int32_t v) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}

// slot_row[t] = the row of edge csc_eid[t]: the last r with row_ptr[r] <= e.
__global__ __launch_bounds__(kBlock) void slot_row_kernel(const int32_t *__restrict__ row_ptr,
                                                          const int32_t *__restrict__ csc_eid,
                                                          int32_t *__restrict__ slot_row,
                                                          int num_rows, int64_t num_e) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= num_e) return;
    const int e = csc_eid[t];
    int lo = 0, hi = num_rows;  // row_ptr[lo] <= e < row_ptr[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (row_ptr[mid] <= e) lo = mid; else hi = mid;
    }
    slot_row[t] = lo;
}

// One group of 2^kgs lanes per column; lane l0 of it owns the slots l0, l0 + KG, ...
__global__ __launch_bounds__(kBlock) void max_bwd_kernel(
    const int32_t *__restrict__ col_ptr, const int32_t *__restrict__ csc_eid,
    const int32_t *__restrict__ slot_row, const uint8_t *__restrict__ cbsr_idx,
    const int32_t *__restrict__ arg, const float *__restrict__ grad_out,
    float *__restrict__ grad_cbsr, int64_t num_cols, int D, int k, int kgs) {
    constexpr int U = 4;
    const int64_t c = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> kgs;
    const int l0 = threadIdx.x & ((1 << kgs) - 1);
    if (c >= num_cols) return;
    const int tb = col_ptr[c], te = col_ptr[c + 1];
    for (int l = l0; l < k; l += 1 << kgs) {
        const int j = cbsr_idx[c * k + l];
        float acc = 0.f;
        if (j < D) {
            for (int t = tb; t < te; t += U) {
                int e[U], a[U];
                int64_t o[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int tu = t + u < te ? t + u : te - 1;
                    e[u] = csc_eid[tu];
                    o[u] = (int64_t)slot_row[tu] * D + j;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) a[u] = arg[o[u]];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (t + u < te && a[u] == e[u]) acc += grad_out[o[u]];
            }
        }
        grad_cbsr[c * k + l] = acc;
    }
}

int check_max_sizes(int64_t num_rows, int64_t num_cols, int64_t num_e) {
    MAXK_REQUIRE(num_rows >= 0 && num_rows < (1LL << 31), "num_rows out of range: %lld",
                 (long long)num_rows);
    MAXK_REQUIRE(num_cols >= 0 && num_cols < (1LL << 31), "num_cols out of range: %lld",
                 (long long)num_cols);
    MAXK_REQUIRE(num_e >= 0 && num_e < (int64_t)kNoEdge, "num_e out of range: %lld",
                 (long long)num_e);
    return MAXK_OK;
}

int check_max_workspace(const void *workspace, size_t bytes, size_t need) {
    MAXK_REQUIRE(workspace && bytes >= need, "workspace too small: need %zu bytes, got %zu", need,
                 workspace ? bytes : (size_t)0);
    MAXK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-B aligned");
    return MAXK_OK;
}

bool max_shape_ok(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k) {
    return num_rows >= 0 && num_cols >= 0 && num_e >= 0 && D >= 1 && D <= kMaxDim && k >= 1 &&
           k <= D;
}

int lane_shift(int k) {
    int s = 0;
    while ((1 << s) < k && (1 << s) < kWave) ++s;
    return s;
}

// The forward's resident waves per CU its item size assumes (66 VGPRs: 7 per SIMD).
constexpr int kMaxFwdWaves = 28;

struct MaxLayout {
    int chunk, n_items, RS;
    int64_t cap;
    bool wide;
    size_t slab_off, cont_off, first_off, total;
};

MaxLayout max_fwd_layout(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k,
                         int chunk) {
    MaxLayout L{};
    const RecordGeom R = record_geom(num_cols, D, k);
    L.RS = R.RS;
    L.wide = R.wide;
    const size_t lds = (size_t)kWavesPerBlock * kMaxDim * (sizeof(uint64_t) + sizeof(uint32_t));
    L.chunk = walk_chunk(num_rows, num_e, chunk, lds, kMaxFwdWaves);
    L.n_items = token_items(num_rows, num_e, L.chunk);
    L.cap = item_cap(num_rows + num_e, chunk, L.n_items);
    L.slab_off = al256((size_t)num_cols * L.RS);
    L.cont_off = L.slab_off + al256((size_t)L.cap * 2 * D * sizeof(uint64_t));
    L.first_off = L.cont_off + al256((size_t)L.cap * sizeof(int32_t));
    L.total = L.first_off + al256((size_t)L.cap * sizeof(int32_t));
    return L;
}

}  // namespace

size_t max_forward_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k,
                                  int chunk) {
    if (!max_shape_ok(num_rows, num_cols, num_e, D, k) || chunk < 0) return 0;
    return max_fwd_layout(num_rows, num_cols, num_e, D, k, chunk).total;
}

int max_forward(const int32_t *row_ptr, const int32_t *col_idx, const float *cbsr_val,
                const uint8_t *cbsr_idx, float *out, int32_t *arg, int64_t num_rows,
                int64_t num_cols, int64_t num_e, int D, int k, int chunk, void *workspace,
                size_t workspace_bytes, void *stream) {
    if (int rc = check_max_sizes(num_rows, num_cols, num_e)) return rc;
    MAXK_REQUIRE(chunk >= 0, "chunk_edges must be >= 0");
    if (int rc = check_cbsr_dims(D, k, num_cols)) return rc;
    if (num_rows == 0) return MAXK_OK;
    MAXK_REQUIRE(row_ptr && out, "row_ptr / out must not be NULL");
    MAXK_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)arg & 3) == 0,
                 "out / arg must be 4-B aligned");
    hipStream_t s = as_stream(stream);
    if (num_e == 0) {
        if (int rc = zero_words(out, num_rows * D, s)) return rc;
        if (arg) {
            const int64_t n = num_rows * D, blocks = ceil_div(n, kBlock);
            hipLaunchKernelGGL(fill_words_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)),
                               dim3(kBlock), 0, s, arg, n, -1);
            MAXK_LAUNCHED("fill_words_kernel");
        }
        return MAXK_OK;
    }
    MAXK_REQUIRE(col_idx && cbsr_val && cbsr_idx, "col_idx / cbsr_val / cbsr_idx must not be NULL");
    MAXK_REQUIRE(num_cols > 0, "edges present but num_cols == 0");
    MAXK_REQUIRE(((uintptr_t)cbsr_val & 3) == 0, "cbsr_val must be 4-B aligned");
    const MaxLayout L = max_fwd_layout(num_rows, num_cols, num_e, D, k, chunk);
    MAXK_REQUIRE(!L.wide, "num_cols: the max aggregation takes tables below 2^24 columns and "
                 "4 GiB of records (%lld columns of %d bytes)", (long long)num_cols, L.RS);
    if (int rc = check_max_workspace(workspace, workspace_bytes, L.total)) return rc;
    char *ws = reinterpret_cast<char *>(workspace);
    uint8_t *rec = reinterpret_cast<uint8_t *>(ws);
    unsigned long long *slab = reinterpret_cast<unsigned long long *>(ws + L.slab_off);
    int32_t *cont_row = reinterpret_cast<int32_t *>(ws + L.cont_off);
    int32_t *first_row = reinterpret_cast<int32_t *>(ws + L.first_off);
    if (int rc = launch_cbsr_pack(cbsr_val, cbsr_idx, rec, num_cols, k, L.RS, D, copy_stride(D) - 1,
                                  s))
        return rc;
    hipLaunchKernelGGL(max_fwd_kernel, item_grid(L.n_items), dim3(kBlock), 0, s, row_ptr, col_idx,
                       rec, (uint32_t)((uint64_t)num_cols * L.RS), L.RS, out, arg, slab, L.cap,
                       cont_row, first_row, (int)num_rows, num_e, D, k, lane_shift(k), L.chunk,
                       L.n_items);
    MAXK_LAUNCHED("max_fwd_kernel");
    hipLaunchKernelGGL(max_fixup_kernel, dim3((unsigned)ceil_div(L.n_items, kBlock / 16)),
                       dim3(kBlock), 0, s, slab, L.cap, cont_row, first_row, out, arg, D,
                       L.n_items);
    MAXK_LAUNCHED("max_fixup_kernel");
    return MAXK_OK;
}

size_t max_backward_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e, int D,
                                   int k) {
    if (!max_shape_ok(num_rows, num_cols, num_e, D, k)) return 0;
    const size_t n = al256((size_t)num_e * sizeof(int32_t));
    return n ? n : 256;  // never empty: one query serves any num_e
}

int max_backward(const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr,
                 const int32_t *csc_eid, const uint8_t *cbsr_idx, const int32_t *arg,
                 const float *grad_out, float *grad_cbsr, int64_t num_rows, int64_t num_cols,
                 int64_t num_e, int D, int k, void *workspace, size_t workspace_bytes,
                 void *stream) {
    (void)col_idx;  // the CSC side names every edge's column already
    if (int rc = check_max_sizes(num_rows, num_cols, num_e)) return rc;
    if (int rc = check_cbsr_dims(D, k, num_cols)) return rc;
    if (num_cols == 0) return MAXK_OK;
    MAXK_REQUIRE(grad_cbsr, "grad_cbsr must not be NULL");
    MAXK_REQUIRE(((uintptr_t)grad_cbsr & 3) == 0 && ((uintptr_t)grad_out & 3) == 0 &&
                     ((uintptr_t)arg & 3) == 0,
                 "grad_cbsr / grad_out / arg must be 4-B aligned");
    hipStream_t s = as_stream(stream);
    if (num_e == 0) return zero_words(grad_cbsr, num_cols * k, s);
    MAXK_REQUIRE(row_ptr && col_ptr && csc_eid && cbsr_idx && arg && grad_out,
                 "row_ptr / col_ptr / csc_eid / cbsr_idx / arg / grad_out must not be NULL");
    MAXK_REQUIRE(num_rows > 0, "edges present but num_rows == 0");
    if (int rc = check_max_workspace(workspace, workspace_bytes,
                                     max_backward_workspace_size(num_rows, num_cols, num_e, D, k)))
        return rc;
    int32_t *slot_row = reinterpret_cast<int32_t *>(workspace);
    hipLaunchKernelGGL(slot_row_kernel, dim3((unsigned)ceil_div(num_e, kBlock)), dim3(kBlock), 0,
                       s, row_ptr, csc_eid, slot_row, (int)num_rows, num_e);
    MAXK_LAUNCHED("slot_row_kernel");
    const int kgs = lane_shift(k);
    hipLaunchKernelGGL(max_bwd_kernel, dim3((unsigned)ceil_div(num_cols << kgs, kBlock)),
                       dim3(kBlock), 0, s, col_ptr, csc_eid, slot_row, cbsr_idx, arg, grad_out,
                       grad_cbsr, num_cols, D, k, kgs);
    MAXK_LAUNCHED("max_bwd_kernel");
    return MAXK_OK;
}

}  // namespace maxk
