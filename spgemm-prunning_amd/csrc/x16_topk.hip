// CBSR encode and its adjoint on 16-bit selectors, 1 <= D <= 1024, 1 <= k <= min(D, 256).
//
// x16_topk_kernel<NE>: topk_cbsr_kernel's method (topk_cbsr.hip) with the row spread wider: one
// wave per row, column lane + 64 i in slot i of each lane (coalesced loads), NE = 4, 8 or 16
// slots per lane for D <= 256, 512, 1024, so D = 384 does not pay for 1024's registers.  The
// k-th largest key by the MSB-first radix select over data-adaptive 8-bit digits (a 256-bin
// per-wave LDS histogram); ties taken in column order; the winners compacted into LDS (up to 256
// slots of key, value and a 16-bit column), ranked against each other (key descending, column
// ascending) and stored.  Exact, NaN ranked largest.  With out_dense the masked dense row is
// written in the same pass.  Grid-stride over rows, the next row's loads issued before this
// row is ranked.  LDS per wave: 1 KB histogram + 320 x (4 + 4 + 2) B of slots = 4.1 KB.
//
// x16_scatter_kernel: the adjoint (maxk_topk_backward_x16), one wave per row through an LDS row
// of D floats: zeroed, the k selected columns set, stored whole with 16-B stores.
// DESIGN.md 5.20.
#include "topk_select.h"
#include "x16_pack.h"

namespace maxk {
namespace {

constexpr int kX16Slots = kMaxKX16 + kWave;  // winner slots [0, 256), per-lane scratch [256, 320)

template <int NE>
__global__ __launch_bounds__(kBlock) void x16_topk_kernel(
    const float *__restrict__ x, int64_t ld_x, float *__restrict__ out_val,
    uint16_t *__restrict__ out_idx, float *__restrict__ out_dense, uint32_t *bad_rows,
    int num_rows, int D, int k) {
    // winner slots [0, k), padding slots [k, k4) (key 0, column 0xffff: never ranked above a
    // winner), and per-lane scratch slots [256, 320) for lanes not taking
    __shared__ __attribute__((aligned(16))) uint32_t s_key[kWavesPerBlock][kX16Slots];
    __shared__ float s_val[kWavesPerBlock][kX16Slots];
    __shared__ __attribute__((aligned(16))) uint16_t s_col[kWavesPerBlock][kX16Slots];
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[kWavesPerBlock][256];
    const int wid = threadIdx.x / kWave;
    const int lane = lane_id();
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    const int stride = gridDim.x * kWavesPerBlock;
    uint32_t *hist = s_hist[wid], *skey = s_key[wid];
    float *sval = s_val[wid];
    uint16_t *scol = s_col[wid];
    // loads are unconditional (clamped row / column), masked after: no predicated loads
    int row = blockIdx.x * kWavesPerBlock + wid;
    float vn[NE];
    {
        const float *xr = x + (int64_t)(row < num_rows ? row : num_rows - 1) * ld_x;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int c = lane + kWave * i;
            vn[i] = xr[c < D ? c : D - 1];
        }
    }
    for (; row < num_rows; row += stride) {
        float v[NE];
        uint32_t key[NE];
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const bool ok = lane + kWave * i < D;
            v[i] = ok ? vn[i] : 0.f;
            key[i] = ok ? order_key(v[i]) : 0u;  // a real key is never 0 (order_key)
        }
        {
            const int nrow = row + stride;
            const float *xr = x + (int64_t)(nrow < num_rows ? nrow : row) * ld_x;
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const int c = lane + kWave * i;
                vn[i] = xr[c < D ? c : D - 1];
            }
        }

        // T = the k-th largest key (topk_cbsr_kernel's search): each pass takes the wave min /
        // max of the keys still in play, histograms the 8 bits right below their common prefix
        // and keeps the largest digit whose suffix count still reaches `need`.
        uint32_t thr = 0, pmask = 0;
        int need = k;  // how many of the keys in play are still to be taken
        int sh = 0;    // selection compares key >> sh with thr (after the final shift)
        for (;;) {
            uint32_t mx = 0u, mn = ~0u;
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const bool in = key[i] != 0u && (key[i] & pmask) == thr;
                mx = in && key[i] > mx ? key[i] : mx;
                mn = in && key[i] < mn ? key[i] : mn;
            }
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) {
                const uint32_t a = __shfl_xor(mx, off), b = __shfl_xor(mn, off);
                mx = a > mx ? a : mx;
                mn = b < mn ? b : mn;
            }
            const uint32_t diff = mx ^ mn;
            if (diff == 0u) {  // every key in play is equal: it is T, ties decide
                thr = mx;
                sh = 0;
                break;
            }
            const int hb = 31 - __builtin_clz(diff);  // highest bit where keys in play differ
            const int shift = hb >= 7 ? hb - 7 : 0;   // digit = bits [shift, shift + 8)
            reinterpret_cast<uint4 *>(hist)[lane] = make_uint4(0u, 0u, 0u, 0u);
            wave_lds_fence();
#pragma unroll
            for (int i = 0; i < NE; ++i)  // branch-free: keys out of play add 0
                atomicAdd(&hist[(key[i] >> shift) & 255u],
                          (key[i] != 0u && (key[i] & pmask) == thr) ? 1u : 0u);
            wave_lds_fence();
            const uint4 h = reinterpret_cast<const uint4 *>(hist)[lane];  // bins 4 lane .. + 3
            const uint32_t s3 = h.w, s2 = h.z + s3, s1 = h.y + s2, s0 = h.x + s1;
            uint32_t acc = s0;  // -> sum of s0 over lanes >= this one
#pragma unroll
            for (int off = 1; off < kWave; off <<= 1) {
                const uint32_t t = __shfl_down(acc, off);
                acc += lane + off < kWave ? t : 0u;
            }
            const uint32_t above = acc - s0;  // keys with a digit in a higher lane's bins
            const uint32_t nd = (uint32_t)need;
            // largest digit d with #{digit >= d} >= need: the highest lane holding one
            const int m = (int)(above + s0 >= nd) + (int)(above + s1 >= nd) +
                          (int)(above + s2 >= nd) + (int)(above + s3 >= nd) - 1;
            const uint32_t gt_l = above + (uint32_t)(m == 0) * s1 + (uint32_t)(m == 1) * s2 +
                                  (uint32_t)(m == 2) * s3;  // #{digit > 4 lane + m}
            const uint32_t ge_l = above + (uint32_t)(m == 0) * s0 + (uint32_t)(m == 1) * s1 +
                                  (uint32_t)(m == 2) * s2 + (uint32_t)(m == 3) * s3;
            const uint64_t has = __ballot(m >= 0);
            const int src = 63 - __clzll(has);
            const int dm = __shfl(m, src);
            const uint32_t gt = __shfl(gt_l, src);
            const uint32_t in_bin = __shfl(ge_l, src) - gt;
            need -= (int)gt;
            // keys in play share every bit above shift + 8 (they differ first at bit hb)
            const uint32_t high = shift + 8 >= 32 ? 0u : (mx & (~0u << (shift + 8)));
            thr = high | ((uint32_t)(4 * src + dm) << shift);
            pmask = ~0u << shift;
            sh = shift;
            if (in_bin == (uint32_t)need || shift == 0) break;  // bin fully taken, or T exact
        }
        const int need_eq = need;
        thr >>= sh;

        // select, then compact the winners into LDS slots [0, k)
        const int k4 = (k + 3) & ~3;
        for (int p = k + lane; p < k4; p += kWave) {
            skey[p] = 0u;
            scol[p] = 0xffffu;
        }
        int eq_base = 0, slot_base = 0;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const bool ok = key[i] != 0u;
            const bool eq = ok && (key[i] >> sh) == thr;
            const uint64_t me = __ballot(eq);
            const int eq_rank = eq_base + __popcll(me & lt_mask);
            eq_base += __popcll(me);
            const bool take = (ok && (key[i] >> sh) > thr) || (eq && eq_rank < need_eq);
            if (out_dense && ok)  // the masked dense row (wave-uniform pointer test)
                out_dense[(int64_t)row * D + lane + kWave * i] = take ? v[i] : 0.f;
            const uint64_t mt = __ballot(take);
            const int ws = slot_base + __popcll(mt & lt_mask);
            const int slot = take && ws < k ? ws : kMaxKX16 + lane;  // never past the k slots
            skey[slot] = key[i];
            sval[slot] = v[i];
            scol[slot] = (uint16_t)(lane + kWave * i);
            slot_base += __popcll(mt);
        }
        // any other count than k is a search bug: counted for the host (maxk_topk_error_rows)
        if (lane == 0 && slot_base != k && bad_rows) atomicAdd(bad_rows, 1u);
        wave_lds_fence();
        // rank of winner p among the winners: (key desc, column asc); 4 slots per LDS read
        for (int p = lane; p < k; p += kWave) {
            const uint32_t kp = skey[p];
            const uint32_t cp = scol[p];
            int pos = 0;
            for (int q = 0; q < k4; q += 4) {
                const uint4 kq = *reinterpret_cast<const uint4 *>(&skey[q]);
                const uint2 cq = *reinterpret_cast<const uint2 *>(&scol[q]);
                pos += (kq.x > kp) || (kq.x == kp && (cq.x & 0xffffu) < cp);
                pos += (kq.y > kp) || (kq.y == kp && (cq.x >> 16) < cp);
                pos += (kq.z > kp) || (kq.z == kp && (cq.y & 0xffffu) < cp);
                pos += (kq.w > kp) || (kq.w == kp && (cq.y >> 16) < cp);
            }
            const int64_t o = (int64_t)row * k + pos;
            out_val[o] = sval[p];
            out_idx[o] = (uint16_t)cp;
        }
        wave_lds_fence();  // this row's LDS slots are read before the next row overwrites them
    }
}

// dense[r, :] = 0; dense[r, idx[r, l]] = val[r, l] + add[r, idx[r, l]] (val, add optional).  A
// row's reads all land in LDS before its stores, so dense may alias add.
__global__ __launch_bounds__(kBlock) void x16_scatter_kernel(
    const float *__restrict__ val, const uint16_t *__restrict__ idx, const float *add, float *dense,
    int num_rows, int D, int DS, int k, int vec) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = lane_id();
    float *buf = lds + (size_t)(threadIdx.x / kWave) * DS;
    for (int row = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; row < num_rows;
         row += gridDim.x * kWavesPerBlock) {
        for (int j = lane * 4; j < DS; j += kWave * 4)
            *reinterpret_cast<float4 *>(&buf[j]) = make_float4(0.f, 0.f, 0.f, 0.f);
        wave_lds_fence();
        for (int l = lane; l < k; l += kWave) {
            const int j = idx[(int64_t)row * k + l];
            if (j >= D) continue;
            float x = val ? val[(int64_t)row * k + l] : 0.f;
            if (add) x += add[(int64_t)row * D + j];
            buf[j] = x;
        }
        wave_lds_fence();
        float *dst = dense + (int64_t)row * D;
        if (vec) {
            for (int j = lane * 4; j < D; j += kWave * 4)
                *reinterpret_cast<float4 *>(&dst[j]) = *reinterpret_cast<const float4 *>(&buf[j]);
        } else {
            for (int j = lane; j < D; j += kWave) dst[j] = buf[j];
        }
        wave_lds_fence();
    }
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" int maxk_topk_cbsr_x16(const float *x, int64_t ld_x, float *cbsr_val,
                                  uint16_t *cbsr_idx, float *out_dense, int64_t num_rows,
                                  int32_t dim_origin, int32_t dim_k, void *stream) {
    clear_error();
    if (int rc = x16_check_dims(dim_origin, dim_k)) return rc;
    MAXK_REQUIRE(num_rows >= 0 && num_rows < (1LL << 31), "num_rows out of range");
    MAXK_REQUIRE(ld_x >= dim_origin, "ld_x (%lld) < dim_origin (%d)", (long long)ld_x, dim_origin);
    if (num_rows == 0) return MAXK_OK;
    MAXK_REQUIRE(x && cbsr_val && cbsr_idx, "x/val/idx must not be NULL");
    const int64_t blocks = ceil_div(num_rows, kWavesPerBlock);
    const dim3 grid((unsigned)(blocks < MAXK_TOPK_BLOCKS ? blocks : MAXK_TOPK_BLOCKS));
    uint32_t *bad = topk_bad_rows_counter();
    const int ne = dim_origin <= 256 ? 4 : dim_origin <= 512 ? 8 : 16;
    with_const<4, 8, 16>(ne, [&](auto ne_c) {
        hipLaunchKernelGGL(x16_topk_kernel<decltype(ne_c)::value>, grid, dim3(kBlock), 0,
                           as_stream(stream), x, ld_x, cbsr_val, cbsr_idx, out_dense, bad,
                           (int)num_rows, dim_origin, dim_k);
    });
    MAXK_LAUNCHED("x16_topk_kernel");
    return MAXK_OK;
}

extern "C" int maxk_topk_backward_x16(const float *grad_val, const float *grad_dense,
                                      const uint16_t *cbsr_idx, float *grad_x, int64_t num_rows,
                                      int32_t dim_origin, int32_t dim_k, void *stream) {
    clear_error();
    if (int rc = x16_check_dims(dim_origin, dim_k)) return rc;
    MAXK_REQUIRE(num_rows >= 0 && num_rows < (1LL << 31), "num_rows out of range");
    if (num_rows == 0) return MAXK_OK;
    MAXK_REQUIRE(cbsr_idx && grad_x, "pointers must not be NULL");
    const int DS = x16_copy_stride(dim_origin);
    const int vec = dim_origin % 4 == 0 && ((uintptr_t)grad_x & 15) == 0;
    const int64_t blocks = ceil_div(num_rows, kWavesPerBlock);
    const dim3 grid((unsigned)(blocks < MAXK_TOPK_BLOCKS ? blocks : MAXK_TOPK_BLOCKS));
    hipLaunchKernelGGL(x16_scatter_kernel, grid, dim3(kBlock),
                       (size_t)kWavesPerBlock * DS * sizeof(float), as_stream(stream), grad_val,
                       cbsr_idx, grad_dense, grad_x, (int)num_rows, dim_origin, DS, dim_k, vec);
    MAXK_LAUNCHED("x16_scatter_kernel");
    return MAXK_OK;
}
