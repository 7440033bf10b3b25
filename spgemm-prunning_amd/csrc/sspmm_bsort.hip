// Backward SSpMM, the window-sorted two-phase form (maxk_sspmm_backward_bsort; the forms and
// their formula: sspmm_bwd.h).  Phase 1 (bsort_push_kernel) writes each window of CSR edges'
// contribution rows ordered by destination bucket; phase 2 (bucket_sum_kernel) reads a
// bucket's rows as runs and sums them in an fp64 LDS accumulator.  The plain "bucket" mode
// over CSR-ordered rows left the library in r06.
#include "sspmm_bwd.h"

namespace maxk {
namespace {

// ---- phase 2, bucketed: grad_cbsr[c, :] = sum of T[e, :] over the entries of c's bucket ----
// The bucket-ordered entry list (bucket_eid: per bucket of 2^shift destinations, the CSR
// edge ids into it in CSR order) is cut into equal parts of `part` entries, one
// 1024-thread workgroup each, so a heavy bucket (power-law in-degrees: the largest
// Reddit-sized bucket holds 1.2x the mean) never sets the kernel time alone.  A part
// walks the buckets it meets; per bucket it sums into an fp64 LDS accumulator
// [2^shift, k + 1] and stores the bucket's rows directly when it holds all of the bucket's
// entries, else one fp32 partial to its slab slot (slot 0: the part's first bucket, 1: its
// last); bucket_fixup_kernel adds the partials in part order and zero-fills empty buckets.
// Entries are read in order, LR = pow2ceil(k/4) lanes per T row (16-B loads), 64/LR
// consecutive entries per wave instruction: neighbouring entries of one source row are
// neighbouring T rows, so one line request serves several of them (a Reddit-sized bucket
// of 1024 destinations holds ~2.2 edges of every source row).  Sums go through ds_add_f64:
// on gfx950 it costs about a ds_write (8.8 cycles per wave instruction), ds_add_f32 costs
// 193 (tools/lds_atomic_probe.hip).  fp64 partial sums make the fp32 result independent of
// the order of the adds except in rare rounding ties.  U steps of loads in flight, the
// next step's entry ids prefetched.
template <int LR, int U>
__global__ __launch_bounds__(1024) void bucket_sum_kernel(
    const float *__restrict__ T, const int32_t *__restrict__ bucket_ptr,
    const int32_t *__restrict__ bucket_eid, const uint16_t *__restrict__ bucket_dst,
    float *__restrict__ grad_cbsr, float *__restrict__ slab, int num_cols, int n_buckets,
    int num_e, int k, int shift, int part) {
    __shared__ double acc[kBucketAccDoubles];
    __shared__ int s_j0;
    constexpr int EPI = kWave / LR;  // entries per wave instruction
    constexpr int STEP = EPI * U;    // entries per wave step
    const int tid = threadIdx.x;
    const int lane = lane_id(), w = tid / kWave;
    const int g = lane / LR, q = lane % LR;
    const int kq = k >> 2;
    const bool qok = q < kq;
    const int nacc = k << shift;  // floats of one bucket (output / slab slot)
    const int ks = k + 1;         // LDS row stride (doubles)
    const int nlds = ks << shift;
    const int p = blockIdx.x;
    const int p0 = p * part, p1 = num_e - p0 > part ? p0 + part : num_e;
    if (tid == 0) {  // first bucket of the part: the last j with bucket_ptr[j] <= p0
        int lo = 0, hi = n_buckets - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (bucket_ptr[mid] <= p0) lo = mid; else hi = mid - 1;
        }
        s_j0 = lo;
    }
    __syncthreads();
    const int j0 = s_j0;
    const float4 *__restrict__ T4 = reinterpret_cast<const float4 *>(T);
    for (int j = j0; j < n_buckets; ++j) {
        const int b0 = bucket_ptr[j], b1 = bucket_ptr[j + 1];
        if (b0 >= p1) break;
        if (b0 == b1) continue;  // empty bucket: zero-filled by the fixup
        const int s0 = b0 > p0 ? b0 : p0, s1 = b1 < p1 ? b1 : p1;
        for (int i = tid; i < nlds; i += 1024) acc[i] = 0.0;
        __syncthreads();
        int base = s0 + w * STEP;
        int e[U], d[U];
        auto load_ids = [&](int b) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = b + u * EPI + g;
                const int tc = t < s1 ? t : s1 - 1;
                e[u] = bucket_eid[tc];
                d[u] = t < s1 ? (int)bucket_dst[tc] : -1;
            }
        };
        if (base < s1) load_ids(base);
        for (; base < s1; base += 16 * STEP) {
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                v[u] = T4[(size_t)(uint32_t)e[u] * (uint32_t)kq + (qok ? q : 0)];
            int dc[U];
#pragma unroll
            for (int u = 0; u < U; ++u) dc[u] = d[u];
            if (base + 16 * STEP < s1) load_ids(base + 16 * STEP);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (dc[u] >= 0 && qok) {
                    double *a = &acc[dc[u] * ks + 4 * q];
                    atomicAdd(a + 0, (double)v[u].x);
                    atomicAdd(a + 1, (double)v[u].y);
                    atomicAdd(a + 2, (double)v[u].z);
                    atomicAdd(a + 3, (double)v[u].w);
                }
            }
        }
        __syncthreads();
        const int64_t c0 = (int64_t)j << shift;
        const int rows = num_cols - c0 < (1 << shift) ? (int)(num_cols - c0) : (1 << shift);
        const bool whole = b0 >= p0 && b1 <= p1;
        float *o = whole ? grad_cbsr + c0 * k
                         : slab + ((size_t)p * 2 + (j == j0 ? 0 : 1)) * (size_t)nacc;
        for (int i = tid; i < rows * k; i += 1024) {
            const int r = i / k;
            o[i] = (float)acc[i + r];  // row r starts at r * (k + 1)
        }
        __syncthreads();
    }
}

// Buckets no single part holds whole: the sum of their parts' slab partials in part order;
// empty buckets: zeros.  One thread per 4 floats; blockIdx.x = bucket, blockIdx.y = tile.
__global__ __launch_bounds__(kBlock) void bucket_fixup_kernel(
    const int32_t *__restrict__ bucket_ptr, const float *__restrict__ slab,
    float *__restrict__ grad_cbsr, int num_cols, int k, int shift, int part) {
    const int j = blockIdx.x;
    const int b0 = bucket_ptr[j], b1 = bucket_ptr[j + 1];
    const int plo = b0 / part, phi = b1 > 0 ? (b1 - 1) / part : 0;
    if (b0 != b1 && plo == phi) return;  // stored whole by its part
    const int64_t c0 = (int64_t)j << shift;
    const int rows = num_cols - c0 < (1 << shift) ? (int)(num_cols - c0) : (1 << shift);
    const int n4 = rows * k / 4;  // k % 4 == 0
    const int i = blockIdx.y * kBlock + threadIdx.x;
    if (i >= n4) return;
    float4 *o = reinterpret_cast<float4 *>(grad_cbsr + c0 * k) + i;
    if (b0 == b1) {
        *o = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const size_t nacc4 = ((size_t)k << shift) / 4;
    const float4 *sl = reinterpret_cast<const float4 *>(slab);
    const int lo_slot = plo * part < b0 ? 1 : 0;  // bucket j is the last bucket of part plo
    float4 a = sl[((size_t)plo * 2 + lo_slot) * nacc4 + i];
    for (int p = plo + 1; p <= phi; ++p) {
        const float4 b = sl[(size_t)p * 2 * nacc4 + i];
        a.x += b.x;
        a.y += b.y;
        a.z += b.z;
        a.w += b.w;
    }
    *o = a;
}

// ---- window-sorted phase 1 ("bsort", maxk_sspmm_backward_bsort) ---------------------------
// On a large sparse graph every contribution row the bucketed phase 2 (or csc) reads lies on
// its own random line: at k = 8 a 32-B row costs a 128-B line, so phase 2 runs at the
// fabric's random-line rate whatever k.  Here the edges are cut into windows
// of W consecutive CSR edges (W * k * 4 B fill the 160 KiB LDS stage), one 1024-thread
// workgroup per window: its waves compute the window's rows into LDS in CSR order, then the
// workgroup writes them out to T[window] ordered by destination bucket (win_src: T row
// w0 + i holds edge w0 + win_src[w0 + i]; a stable sort on the bucket, from maxk_bsort_plan).
// A bucket's rows of one window are then one contiguous run (ogbn-products k = 8, W = 5120,
// 1196 buckets: ~4 rows, 137 B), read by bucket_sum_kernel through the plan's positions.  The
// writes stay coalesced: the reorder happens in LDS.
// One workgroup per CU (the stage fills the LDS), so every wave must keep its loads in flight
// across its share of the window: the share is walked in flat batches of edges whatever rows
// they belong to (the source row of each edge from the plan's edge_row), each edge's k values
// gathered straight from G (its rows sit in L2: a window spans ~100 rows on ogbn-products), and
// batch i + 2's weights / selectors / rows and batch i + 1's gathers are issued before batch i
// is computed.  Per-row G staging in LDS as in sspmm_bwd_kernel cost one exposed load latency
// per row segment at this occupancy (2.68 vs 1.45 ms for the CSR-order phase 1, products k=8).
constexpr int kBsortThreads = 1024;
constexpr int kBsortWaves = kBsortThreads / kWave;
constexpr int kBsortStageFloats = 160 * 1024 / 4;
constexpr int kBsortPer = kBsortStageFloats / 4 / kBsortThreads;  // 16-B stage units per thread
static_assert(kBsortStageFloats % (4 * kBsortThreads) == 0, "whole units per thread");

template <int LR, int U, bool ES>
__global__ __launch_bounds__(kBsortThreads) void bsort_push_kernel(
    const int32_t *__restrict__ edge_row, const int32_t *__restrict__ col_idx,
    const float *__restrict__ edge_val, const float *__restrict__ grad,
    const float *__restrict__ row_div, const uint8_t *__restrict__ cbsr_idx,
    const uint8_t *__restrict__ esel, const uint16_t *__restrict__ win_src,
    float *__restrict__ T, int num_e, int D, int k, int W) {
    __shared__ __attribute__((aligned(16))) float stage[kBsortStageFloats];
    constexpr int G = kWave / LR;  // edges per wave instruction
    constexpr int GU = G * U;      // edges per batch
    const int wid = threadIdx.x / kWave;
    const int lane = lane_id();
    const int b = MAXK_P1_XCD ? xcd_contiguous_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int64_t w0l = (int64_t)b * W;
    if (w0l >= num_e) return;  // whole workgroup: padding blocks of the XCD grid
    const int w0 = (int)w0l;
    const int w1 = num_e - w0 > W ? w0 + W : num_e;
    const int per = (w1 - w0 + kBsortWaves - 1) / kBsortWaves;
    const int e0 = w0 + wid * per;
    const int n = (e0 + per < w1 ? e0 + per : w1) - e0;  // this wave's edges (may be <= 0)
    // the write-out's source rows, loaded now so they are in by the time it runs
    const int kq = k >> 2;
    const int nrow = w1 - w0;
    int src[kBsortPer];
#pragma unroll
    for (int j = 0; j < kBsortPer; ++j) {
        const int i = threadIdx.x + j * kBsortThreads;
        src[j] = i < nrow * kq ? (int)win_src[w0 + i / kq] : 0;
    }
    if (n > 0) {
        const int grp = lane / LR;
        const int q = lane % LR;
        const int k4 = k >> 2;
        const bool active = q < k4;
        const uint32_t qsel = 4u * (uint32_t)(active ? q : k4 - 1);
        // past the share's end the buffer loads return 0: weight 0, row 0, selector 0
        const auto vrs = wave_buffer(edge_val + e0, (uint32_t)n * 4u);
        const auto rrs = wave_buffer(edge_row + e0, (uint32_t)n * 4u);
        const auto crs = wave_buffer(col_idx + (ES ? 0 : e0), ES ? 0u : (uint32_t)n * 4u);
        const auto srs = ES ? wave_buffer(esel + (size_t)(uint32_t)e0 * k, (uint32_t)n * k)
                            : wave_buffer(cbsr_idx, 0xffffffffu);
        float *st = stage + (size_t)(e0 - w0) * k + 4 * q;
        struct Batch {  // per lane and wave instruction u: weight, source row, 4 selectors
            float w[U];
            int r[U];
            uint32_t s[U];
        };
        struct Vals {  // the 4 gathered G values and the row's divisor
            float v[U][4];
            float dv[U];
        };
        auto load_batch = [&](int base, Batch &a) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int o = (base + u * G + grp) * 4;
                a.w[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vrs, o, 0, 0));
                a.r[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(rrs, o, 0, 0);
                if (ES) {
                    a.s[u] = __builtin_amdgcn_raw_buffer_load_b32(
                        srs, (int)((uint32_t)(base + u * G + grp) * (uint32_t)k + qsel), 0, 0);
                } else {
                    const uint32_t c = __builtin_amdgcn_raw_buffer_load_b32(crs, o, 0, 0);
                    a.s[u] = __builtin_amdgcn_raw_buffer_load_b32(srs, (int)(c * (uint32_t)k + qsel),
                                                                  0, 0);
                }
            }
        };
        auto gather = [&](const Batch &a, Vals &g) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float *gr = grad + (int64_t)a.r[u] * D;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = (int)((a.s[u] >> (8 * j)) & 255u);
                    g.v[u][j] = gr[c < D ? c : 0];
                }
                g.dv[u] = row_div ? row_div[a.r[u]] : 1.f;
            }
        };
        auto compute = [&](int base, const Batch &a, const Vals &g) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float x[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = (int)((a.s[u] >> (8 * j)) & 255u);
                    const float gv = row_div ? g.v[u][j] / g.dv[u] : g.v[u][j];
                    x[j] = a.w[u] * (c < D ? gv : 0.f);  // a selector >= D reads 0
                }
                const int e = base + u * G + grp;
                if (active && e < n)
                    *reinterpret_cast<float4 *>(st + (size_t)e * k) =
                        make_float4(x[0], x[1], x[2], x[3]);
            }
        };
        Batch a0, a1;
        Vals g0;
        load_batch(0, a0);
        gather(a0, g0);
        if (GU < n) load_batch(GU, a1);
        for (int base = 0; base < n; base += GU) {
            Batch a2;
            Vals g1;
            if (base + 2 * GU < n) load_batch(base + 2 * GU, a2);
            if (base + GU < n) gather(a1, g1);
            compute(base, a0, g0);
            a0 = a1;
            a1 = a2;
            g0 = g1;
        }
    }
    __syncthreads();
    // write-out in bucket order: T row w0 + i <- staged row win_src[w0 + i], 16 B per thread,
    // non-temporal (the 1-4 GB stream would evict the lines phase 1 re-reads)
    const auto trs = wave_buffer(T + (size_t)w0 * k, (uint32_t)nrow * k * 4u);
    const float4 *st4 = reinterpret_cast<const float4 *>(stage);
#pragma unroll
    for (int j = 0; j < kBsortPer; ++j) {
        const int i = threadIdx.x + j * kBsortThreads;
        const int p = i / kq;
        const int sr = src[j] < nrow ? src[j] : nrow - 1;
        const float4 v = st4[sr * kq + (i - p * kq)];
        if (i < nrow * kq)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), trs, i * 16, 0,
                                                   MAXK_T_AUX);
    }
}

// Bucketed phase 2: entries per part (~MAXK_BUCKET_PARTS parts per CU, at least 16384).
int bucket_part(int64_t num_e) {
    int64_t p = ceil_div(num_e, device_cus() * MAXK_BUCKET_PARTS);
    return (int)(p < 16384 ? 16384 : p);
}

// Workspace: T [E + 1, k] floats, then 2 slab rows per part (the part's first and last
// buckets) of 2^shift * k floats each, sized for the widest bucket a plan may carry
// (maxk_bucket_shift); a plan of narrower buckets uses the head of each part's rows.
struct BsortLayout {
    int part;       // entries per part
    int64_t parts;
    size_t slab_off, total;
};

BsortLayout bsort_layout(int64_t num_e, int k) {
    BsortLayout L{};
    L.part = bucket_part(num_e);
    L.parts = ceil_div(num_e, L.part);
    L.slab_off = al256((size_t)(num_e + 1) * k * sizeof(float));
    L.total = L.slab_off +
              (size_t)L.parts * 2 * ((size_t)k << maxk_bucket_shift(k)) * sizeof(float);
    return L;
}

// Phase 2: bucket_sum_kernel over the bucket list (entry i reads T row bucket_row[i]) and the
// fixup of the buckets split over parts.
int bucket_phase2(hipStream_t s, const BsortLayout &L, const float *T, const int32_t *bucket_ptr,
                  const int32_t *bucket_row, const uint16_t *bucket_dst, int bucket_shift,
                  float *grad_cbsr, void *workspace, int64_t num_cols, int64_t num_e, int k) {
    const int64_t nb = (num_cols + (1LL << bucket_shift) - 1) >> bucket_shift;
    float *slab = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + L.slab_off);
    const int nc = (int)num_cols, ne = (int)num_e, nbi = (int)nb;
    const int32_t *bucket_eid = bucket_row;
    const int lr = lanes_per_edge(k / 4);
    const bool ok = L.parts <= 0 || with_lanes(lr, [&](auto lr_c) {
        hipLaunchKernelGGL((bucket_sum_kernel<decltype(lr_c)::value, MAXK_BUCKET_U>),
                           dim3((unsigned)L.parts), dim3(1024), 0, s, T, bucket_ptr, bucket_eid,
                           bucket_dst, grad_cbsr, slab, nc, nbi, ne, k, bucket_shift, L.part);
    });
    if (!ok) return bad_lanes(lr);
    MAXK_LAUNCHED("bucket_sum_kernel");
    hipLaunchKernelGGL(bucket_fixup_kernel,
                       dim3((unsigned)nb, (unsigned)ceil_div(((int64_t)k << bucket_shift) / 4, kBlock)),
                       dim3(kBlock), 0, s, bucket_ptr, slab, grad_cbsr, nc, k, bucket_shift, L.part);
    MAXK_LAUNCHED("bucket_fixup_kernel");
    return MAXK_OK;
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" int32_t maxk_bsort_window(int32_t dim_k) {
    if (dim_k <= 0 || dim_k % 4 != 0 || dim_k > kMaxDim) return -1;
    const int w = kBsortStageFloats / dim_k;
    return w > 65536 ? 65536 : w;
}

extern "C" size_t maxk_sspmm_backward_bsort_workspace_size(int64_t num_rows, int64_t num_cols,
                                                           int64_t num_e, int32_t dim_origin,
                                                           int32_t dim_k) {
    (void)num_rows; (void)num_cols; (void)dim_origin;
    if (num_e < 0 || dim_k <= 0) return 0;
    return bsort_layout(num_e, dim_k).total;
}

extern "C" int maxk_sspmm_backward_bsort(
    const int32_t *row_ptr, const int32_t *col_idx, const float *edge_val, const float *grad_out,
    const float *row_div, const uint8_t *cbsr_idx, const uint8_t *edge_sel,
    const int32_t *bucket_ptr, const int32_t *bucket_pos, const uint16_t *bucket_dst,
    const uint16_t *win_src, const int32_t *edge_row, int32_t bucket_shift, float *grad_cbsr,
    int64_t num_rows,
    int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k, void *workspace,
    size_t workspace_bytes, void *stream) {
    clear_error();
    if (int rc = check_common(num_rows, num_cols, num_e, dim_origin, dim_k, 0)) return rc;
    MAXK_REQUIRE(dim_k % 4 == 0, "window-sorted backward needs dim_k %% 4 == 0, got %d", dim_k);
    MAXK_REQUIRE(bucket_shift >= 0 && bucket_shift <= 16 &&
                     ((int64_t)(dim_k + 1) << bucket_shift) <= kBucketAccDoubles,
                 "bucket_shift %d too large for dim_k %d (2^shift * (k + 1) <= %d)", bucket_shift,
                 dim_k, kBucketAccDoubles);
    hipStream_t s = as_stream(stream);
    if (num_cols == 0) return MAXK_OK;
    MAXK_REQUIRE(grad_cbsr && bucket_ptr, "grad_cbsr/bucket_ptr must not be NULL");
    MAXK_REQUIRE(num_e == 0 || (row_ptr && edge_val && grad_out && (cbsr_idx || edge_sel) &&
                                (edge_sel || col_idx) && bucket_pos && bucket_dst && win_src &&
                                edge_row),
                 "CSR/grad/selector/plan pointers must not be NULL");
    MAXK_REQUIRE(!edge_sel || ((uintptr_t)edge_sel & 3) == 0, "edge_sel must be 4-B aligned");
    const BsortLayout L = bsort_layout(num_e, dim_k);
    MAXK_REQUIRE(workspace && workspace_bytes >= L.total,
                 "workspace too small: need %zu bytes, got %zu", L.total, workspace_bytes);
    float *T = reinterpret_cast<float *>(workspace);
    const int k = dim_k;
    if (num_e > 0) {
        MAXK_REQUIRE(num_rows > 0, "edges present but num_rows == 0");
        const int W = maxk_bsort_window(k);
        const int64_t nwin = ceil_div(num_e, W);
        const dim3 grid((unsigned)(MAXK_P1_XCD ? xcd_grid(nwin) : nwin));
        const int ne = (int)num_e;
        const int lr = lanes_per_edge(k / 4);
        const bool ok = with_lanes(lr, [&](auto lr_c) {
            with_const<0, 1>(edge_sel != nullptr, [&](auto es_c) {
                hipLaunchKernelGGL((bsort_push_kernel<decltype(lr_c)::value, MAXK_BSORT_U,
                                                      decltype(es_c)::value>),
                                   grid, dim3(kBsortThreads), 0, s, edge_row, col_idx, edge_val,
                                   grad_out, row_div, cbsr_idx, edge_sel, win_src, T, ne,
                                   dim_origin, k, W);
            });
        });
        if (!ok) return bad_lanes(lr);
        MAXK_LAUNCHED("bsort_push_kernel");
    }
    return bucket_phase2(s, L, T, bucket_ptr, bucket_pos, bucket_dst, bucket_shift, grad_cbsr,
                         workspace, num_cols, num_e, k);
}
