// A linear layer on CBSR features (maxk_hip.h has the rules): with x = scatter(CBSR) [V, D] and
// W [O, D] row-major,
//   forward           y[v, o]    = (prior y) + (bias[o]) + sum_j val[v, j] * W[o, idx[v, j]]
//   value gradient    gval[v, j] = sum_o g[v, o] * W[o, idx[v, j]]
//   weight gradient   gW[o, d]   = sum_v sum_{j : idx[v, j] = d} g[v, o] * val[v, j]
// k products per output instead of D.  Every row has its own column set, so there is no shared
// contraction dimension and no MFMA: the three kernels are LDS kernels.
//
// Tile.  The reused operand is W^T.  A workgroup of 16 waves keeps a [D + 1, OT] fp32 tile of it
// in LDS (OT = 128 output columns, 64 when O <= 64; row D is zeros), loads it once and walks the
// rows of its items (chunk_rows rows each, item i of tile t to workgroup i % P).  D = 256,
// OT = 128 is 128.5 KB of the CU's 160 KB: one workgroup per CU, so the workgroup is 1024 threads
// to give every SIMD four waves.
//
// Forward: one wave per row.  Lane j loads (val, idx)[v, j]; slot by slot the pair is broadcast
// with v_readlane into SGPRs, so the LDS row is wave-uniform and lane l reads its CPL = OT / 64
// adjacent columns of it: one conflict-free 8-byte read per slot, 8 slots in flight.  A selector
// >= D is sent to the zero row with the value 0: fma(0, 0, acc) keeps acc and no NaN of val or W
// gets in.
//
// Value gradient: the same tile and the same lane mapping (lanes on output columns), so the LDS
// reads stay conflict-free; the price is a wave reduction per slot.  Four slots are reduced
// together: v_permlane32_swap and v_permlane16_swap each fold two partial registers into one
// with one add, which leaves the four slots' sums of 16 lanes in the four DPP rows, and four DPP
// adds finish them -- 10 instructions per 4 slots, a fixed tree.  O > OT: each tile writes its
// partial [V, k] into the workspace and a second kernel adds the tiles in tile order.
//
// Weight gradient: an accumulator tile [D, OT + 1] in LDS (the pad makes the transposed flush
// conflict-free), lanes on output columns, one column each.  Wave (h, c) of the 16 owns the 64
// columns of half h in the rows d with d % 8 == c: every wave scans every row's selectors, a
// ballot picks its slots, and it adds val * g into its own addresses row by row, slot by slot
// (eight rows' loads in flight), with a plain LDS read-modify-write.  No two waves share an
// address, so there are no atomics and the result does not depend on wave timing.  Each
// workgroup flushes its tile as [OT, D] into the workspace and wgrad_sum_kernel adds the P
// partials of a tile in workgroup order.
#include "common.h"

namespace maxk {
namespace {

constexpr int kLinBlock = 1024;  // one workgroup per CU at D = 256: 4 waves per SIMD
constexpr int kLinWaves = kLinBlock / kWave;
constexpr int kLinChunk = 256;   // chunk_rows = 0
constexpr int kWgOT = 128;       // weight gradient: output columns per tile, one per lane
constexpr int kWgStride = kWgOT + 1;
constexpr int kWgClasses = kLinWaves / (kWgOT / kWave);  // d % 8 picks the wave
constexpr int kWgRows = 8;  // weight gradient: rows whose loads a wave keeps in flight
#ifndef MAXK_LIN_ROUTE_DIV  // maxk_cbsr_linear_route: k <= D / this
#define MAXK_LIN_ROUTE_DIV 16
#endif

template <int CPL>
struct Cols;
template <>
struct Cols<1> {
    float x;
    __device__ __forceinline__ void fma(float a, const Cols &w) { x = fmaf(a, w.x, x); }
    __device__ __forceinline__ float dot(const Cols &w) const { return x * w.x; }
};
template <>
struct alignas(8) Cols<2> {
    float x, y;
    __device__ __forceinline__ void fma(float a, const Cols &w) {
        x = fmaf(a, w.x, x);
        y = fmaf(a, w.y, y);
    }
    __device__ __forceinline__ float dot(const Cols &w) const { return fmaf(x, w.x, y * w.y); }
};

// a[c] = p[o + c] for the columns below O, 0 past them; vec: o and the row are 8-B aligned
template <int CPL>
__device__ __forceinline__ Cols<CPL> load_cols(const float *__restrict__ p, int o, int O,
                                               bool vec) {
    Cols<CPL> a;
    if constexpr (CPL == 2) {
        if (vec && o + 1 < O) return *reinterpret_cast<const Cols<2> *>(p + o);
        a.y = o + 1 < O ? p[o + 1] : 0.f;
    }
    a.x = o < O ? p[o] : 0.f;
    return a;
}

template <int CPL>
__device__ __forceinline__ void store_cols(float *__restrict__ p, int o, int O, bool vec,
                                           const Cols<CPL> &a) {
    if constexpr (CPL == 2) {
        if (vec && o + 1 < O) {
            *reinterpret_cast<Cols<2> *>(p + o) = a;
            return;
        }
        if (o + 1 < O) p[o + 1] = a.y;
    }
    if (o < O) p[o] = a.x;
}

__device__ __forceinline__ int lane_of(int x, int j) { return __builtin_amdgcn_readlane(x, j); }
__device__ __forceinline__ float lane_of(float x, int j) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j));
}

// s[d * OT + ol] = W[o0 + ol, d] (0 past O), row D zeros.  Lanes run along ol: the LDS stores
// are conflict-free; the global loads are 16 B per lane when the rows allow it.
template <int OT>
__device__ __forceinline__ void load_wt(float *__restrict__ s, const float *__restrict__ W, int O,
                                        int D, int o0) {
    const int tid = threadIdx.x, nt = blockDim.x;
    if ((D & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0) {
        const int nq = D >> 2;
        for (int i = tid; i < OT * nq; i += nt) {
            const int ol = i % OT, q = i / OT;
            float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
            if (o0 + ol < O)
                w = *reinterpret_cast<const float4 *>(W + (int64_t)(o0 + ol) * D + 4 * q);
            float *r = s + 4 * q * OT + ol;
            r[0] = w.x;
            r[OT] = w.y;
            r[2 * OT] = w.z;
            r[3 * OT] = w.w;
        }
    } else {
        for (int i = tid; i < OT * D; i += nt) {
            const int ol = i % OT, d = i / OT;
            s[d * OT + ol] = o0 + ol < O ? W[(int64_t)(o0 + ol) * D + d] : 0.f;
        }
    }
    for (int i = tid; i < OT; i += nt) s[D * OT + i] = 0.f;
    __syncthreads();
}

template <int CPL>
__global__ __launch_bounds__(kLinBlock) void lin_fwd_kernel(
    const float *__restrict__ val, const uint8_t *__restrict__ idx, const float *__restrict__ W,
    const float *__restrict__ bias, float *__restrict__ y, int V, int D, int k, int O, int chunk,
    int n_items, int P, int accumulate) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];
    constexpr int OT = kWave * CPL, U = 8;
    const int tile = blockIdx.x / P, p = blockIdx.x % P, o0 = tile * OT;
    load_wt<OT>(s_w, W, O, D, o0);
    const int lane = lane_id(), wave = threadIdx.x / kWave;
    const int oc = o0 + lane * CPL;
    const bool vec = (O & 1) == 0 && (reinterpret_cast<uintptr_t>(y) & 7) == 0;
    Cols<CPL> b = load_cols<CPL>(bias ? bias : W, oc, bias ? O : 0, false);
    const float *sl = s_w + lane * CPL;
    for (int item = p; item < n_items; item += P) {
        const int64_t r1 = (int64_t)(item + 1) * chunk, v1 = r1 < V ? r1 : V;
        for (int64_t v = (int64_t)item * chunk + wave; v < v1; v += kLinWaves) {
            float *yr = y + (int64_t)v * O;
            Cols<CPL> acc = load_cols<CPL>(yr, oc, accumulate ? O : 0, vec);
            acc.x += b.x;
            if constexpr (CPL == 2) acc.y += b.y;
            for (int jb = 0; jb < k; jb += kWave) {
                const int j = jb + lane;
                int d = D;
                float xv = 0.f;
                if (j < k) {
                    d = idx[(int64_t)v * k + j];
                    xv = val[(int64_t)v * k + j];
                    if (d >= D) {
                        d = D;
                        xv = 0.f;
                    }
                }
                const int kc = k - jb < kWave ? k - jb : kWave;
                for (int j0 = 0; j0 < kc; j0 += U) {  // lanes past kc hold (0, zero row)
                    Cols<CPL> w[U];
                    float xj[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        xj[u] = lane_of(xv, j0 + u);
                        w[u] = *reinterpret_cast<const Cols<CPL> *>(sl + lane_of(d, j0 + u) * OT);
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) acc.fma(xj[u], w[u]);
                }
            }
            store_cols<CPL>(yr, oc, O, vec, acc);
        }
    }
}

template <int CTRL>
__device__ __forceinline__ float dpp_add(float x) {
    return x + __int_as_float(
                   __builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}

// The sums over the wave of four per-lane partials, slot s left in every lane of DPP row
// kRowSlot^-1: row 0 slot 0, row 1 slot 2, row 2 slot 1, row 3 slot 3.  permlane32_swap(a, b)
// gives [a.lo, b.lo] and [a.hi, b.hi], whose sum folds the halves of two slots at once;
// permlane16_swap does the same with the odd and even rows.
__device__ __forceinline__ float sum4(float p0, float p1, float p2, float p3) {
    auto fold32 = [](float a, float b) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b),
                                                        false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);
    };
    const float a = fold32(p0, p1), b = fold32(p2, p3);
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false,
                                                    false);
    float x = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    x = dpp_add<0xB1>(x);   // quad_perm [1,0,3,2]
    x = dpp_add<0x4E>(x);   // quad_perm [2,3,0,1]
    x = dpp_add<0x141>(x);  // row_half_mirror
    return dpp_add<0x140>(x);  // row_mirror
}

// out: gval [V, k], or with more than one tile the tiles' partials [n_tiles, V, k]
template <int CPL>
__global__ __launch_bounds__(kLinBlock) void lin_gval_kernel(
    const float *__restrict__ g, const uint8_t *__restrict__ idx, const float *__restrict__ W,
    float *__restrict__ out, int V, int D, int k, int O, int chunk, int n_items, int P) {
    extern __shared__ __attribute__((aligned(16))) float s_w[];
    constexpr int OT = kWave * CPL;
    const int tile = blockIdx.x / P, p = blockIdx.x % P, o0 = tile * OT;
    load_wt<OT>(s_w, W, O, D, o0);
    const int lane = lane_id(), wave = threadIdx.x / kWave;
    const int oc = o0 + lane * CPL;
    const bool vec = (O & 1) == 0 && (reinterpret_cast<uintptr_t>(g) & 7) == 0;
    const float *sl = s_w + lane * CPL;
    float *o_t = out + (int64_t)tile * V * k;
    // the slot of a 64-slot chunk this lane ends up holding (sum4's row order)
    const int row = lane >> 4, mine = 4 * (lane & 15) + ((row & 1) << 1 | row >> 1);
    for (int item = p; item < n_items; item += P) {
        const int64_t r1 = (int64_t)(item + 1) * chunk, v1 = r1 < V ? r1 : V;
        for (int64_t v = (int64_t)item * chunk + wave; v < v1; v += kLinWaves) {
            const Cols<CPL> gl = load_cols<CPL>(g + (int64_t)v * O, oc, O, vec);
            const uint8_t *iv = idx + (int64_t)v * k;
            for (int jb = 0; jb < k; jb += kWave) {
                int d = jb + lane < k ? iv[jb + lane] : D;
                d = d < D ? d : D;  // past D and past k: the zero row
                const int kc = k - jb < kWave ? k - jb : kWave;
                float res = 0.f;
                for (int j0 = 0; j0 < kc; j0 += 4) {
                    float pr[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        pr[u] = gl.dot(
                            *reinterpret_cast<const Cols<CPL> *>(sl + lane_of(d, j0 + u) * OT));
                    const float x = sum4(pr[0], pr[1], pr[2], pr[3]);
                    if ((lane & 15) == (j0 >> 2)) res = x;
                }
                // a selector >= D: exactly 0, whatever g holds
                if (mine < kc) o_t[(int64_t)v * k + jb + mine] = iv[jb + mine] < D ? res : 0.f;
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void gval_sum_kernel(const float *__restrict__ part,
                                                          float *__restrict__ gval, int64_t n,
                                                          int n_tiles) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float a = part[i];
    for (int t = 1; t < n_tiles; ++t) a += part[t * n + i];
    gval[i] = a;
}

// part: [n_tiles, P, kWgOT, D]
__global__ __launch_bounds__(kLinBlock) void lin_wgrad_kernel(
    const float *__restrict__ g, const float *__restrict__ val, const uint8_t *__restrict__ idx,
    float *__restrict__ part, int V, int D, int k, int O, int chunk, int n_items, int P) {
    extern __shared__ __attribute__((aligned(16))) float s_acc[];
    const int tile = blockIdx.x / P, p = blockIdx.x % P, o0 = tile * kWgOT;
    for (int i = threadIdx.x; i < D * kWgStride; i += kLinBlock) s_acc[i] = 0.f;
    __syncthreads();
    const int lane = lane_id(), wave = threadIdx.x / kWave;
    const int half = wave / kWgClasses, cls = wave % kWgClasses;
    const int o = o0 + half * kWave + lane;
    float *sl = s_acc + half * kWave + lane;
    for (int item = p; item < n_items; item += P) {
        const int64_t r1 = (int64_t)(item + 1) * chunk, v1 = r1 < V ? r1 : V;
        // every wave, every row, kWgRows rows' loads in flight: a wave's rows are one dependent
        // chain, and a row at a time the chain is bound by the latency of its three loads
        // v is an int: check_lin_shape keeps V + kWgRows inside one
        for (int v = item * chunk; v < (int)v1; v += kWgRows) {
            float gl[kWgRows];
#pragma unroll
            for (int r = 0; r < kWgRows; ++r)
                gl[r] = v + r < v1 && o < O ? g[(int64_t)(v + r) * O + o] : 0.f;
            for (int jb = 0; jb < k; jb += kWave) {
                const int j = jb + lane;
                int d[kWgRows];
                float xv[kWgRows];
#pragma unroll
                for (int r = 0; r < kWgRows; ++r) {
                    const bool ok = v + r < v1 && j < k;
                    d[r] = ok ? idx[(int64_t)(v + r) * k + j] : D;
                    xv[r] = ok ? val[(int64_t)(v + r) * k + j] : 0.f;
                }
#pragma unroll
                for (int r = 0; r < kWgRows; ++r) {
                    unsigned long long m = __ballot(d[r] < D && d[r] % kWgClasses == cls);
                    while (m) {  // this wave's slots of the row, in slot order
                        const int jj = __builtin_ctzll(m);
                        m &= m - 1;
                        float *a = sl + lane_of(d[r], jj) * kWgStride;
                        *a = fmaf(lane_of(xv[r], jj), gl[r], *a);
                    }
                }
            }
        }
    }
    __syncthreads();
    float *dst = part + (int64_t)(tile * P + p) * kWgOT * D;
    const int cols = O - o0 < kWgOT ? O - o0 : kWgOT;
    for (int i = threadIdx.x; i < cols * D; i += kLinBlock) {
        const int ol = i / D, d = i % D;
        dst[i] = s_acc[d * kWgStride + ol];
    }
}

__global__ __launch_bounds__(kBlock) void wgrad_sum_kernel(const float *__restrict__ part,
                                                           float *__restrict__ gw, int O, int D,
                                                           int P) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)O * D) return;
    const int o = (int)(i / D), d = (int)(i % D);
    const float *src = part + ((int64_t)(o / kWgOT) * P * kWgOT + o % kWgOT) * D + d;
    float a = src[0];
    for (int p = 1; p < P; ++p) a += src[(int64_t)p * kWgOT * D];
    gw[i] = a;
}

struct LinLayout {
    int chunk, n_items, n_tiles, P, cpl;
    size_t lds;
};

int check_lin_shape(int64_t V, int D, int k, int64_t O, int chunk) {
    // the weight gradient counts rows in int, a batch of kWgRows past the last one
    MAXK_REQUIRE(V >= 0 && V < (1LL << 31) - 64, "num_rows out of range: %lld", (long long)V);
    MAXK_REQUIRE(D >= 1 && D <= kMaxDim, "dim_origin must be in [1,256], got %d", D);
    MAXK_REQUIRE(k >= 1 && k <= D, "dim_k must be in [1,dim_origin], got %d", k);
    MAXK_REQUIRE(O >= 1 && O < (1LL << 24), "out_feats must be in [1, 2^24), got %lld",
                 (long long)O);
    MAXK_REQUIRE(V * (int64_t)k < (1LL << 31), "num_rows*k too large");
    MAXK_REQUIRE(chunk >= 0, "chunk_rows must be >= 0");
    return MAXK_OK;
}

// The same conditions for a size query, which reports a refused shape as 0 bytes and leaves no
// message behind.
bool lin_shape_ok(int64_t V, int D, int k, int64_t O, int chunk) {
    const bool ok = check_lin_shape(V, D, k, O, chunk) == MAXK_OK;
    if (!ok) clear_error();
    return ok;
}

// The tile is 64 or 128 columns wide for the W^T kernels, kWgOT for the weight gradient.
LinLayout lin_layout(int64_t V, int D, int64_t O, int chunk, bool wgrad) {
    LinLayout L{};
    L.cpl = wgrad ? 1 : (O <= kWave ? 1 : 2);
    const int ot = wgrad ? kWgOT : kWave * L.cpl;
    L.n_tiles = (int)ceil_div(O, ot);
    L.chunk = chunk > 0 ? chunk : kLinChunk;
    L.n_items = (int)ceil_div(V, L.chunk);
    const int64_t slots = device_cus() / L.n_tiles;  // one resident workgroup per CU
    L.P = (int)(L.n_items < slots ? L.n_items : (slots > 1 ? slots : 1));
    if (L.P < 1) L.P = 1;
    L.lds = wgrad ? (size_t)D * kWgStride * sizeof(float) : (size_t)(D + 1) * ot * sizeof(float);
    return L;
}

int check_lin_workspace(const void *workspace, size_t bytes, size_t need) {
    if (need == 0) return MAXK_OK;
    MAXK_REQUIRE(workspace && bytes >= need, "workspace too small: need %zu bytes, got %zu", need,
                 workspace ? bytes : (size_t)0);
    MAXK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-B aligned");
    return MAXK_OK;
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" int maxk_cbsr_linear_forward(const float *cbsr_val, const uint8_t *cbsr_idx,
                                        const float *weight, const float *bias, float *y,
                                        int64_t num_rows, int32_t dim_origin, int32_t dim_k,
                                        int64_t out_feats, int32_t accumulate, int32_t chunk_rows,
                                        void *stream) {
    clear_error();
    if (int rc = check_lin_shape(num_rows, dim_origin, dim_k, out_feats, chunk_rows)) return rc;
    if (num_rows == 0) return MAXK_OK;
    MAXK_REQUIRE(cbsr_val && cbsr_idx && weight && y,
                 "cbsr_val / cbsr_idx / weight / y must not be NULL");
    MAXK_REQUIRE((((uintptr_t)cbsr_val | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)y) & 3) ==
                     0, "cbsr_val / weight / bias / y must be 4-B aligned");
    const LinLayout L = lin_layout(num_rows, dim_origin, out_feats, chunk_rows, false);
    const dim3 grid((unsigned)(L.n_tiles * L.P));
    auto launch = [&](auto cpl) {
        hipLaunchKernelGGL(lin_fwd_kernel<decltype(cpl)::value>, grid, dim3(kLinBlock), L.lds,
                           as_stream(stream), cbsr_val, cbsr_idx, weight, bias, y, (int)num_rows,
                           dim_origin, dim_k, (int)out_feats, L.chunk, L.n_items, L.P,
                           accumulate ? 1 : 0);
    };
    with_const<1, 2>(L.cpl, launch);
    MAXK_LAUNCHED("lin_fwd_kernel");
    return MAXK_OK;
}

extern "C" size_t maxk_cbsr_linear_backward_values_workspace_size(int64_t num_rows,
                                                                  int32_t dim_origin,
                                                                  int32_t dim_k, int64_t out_feats,
                                                                  int32_t chunk_rows) {
    if (!lin_shape_ok(num_rows, dim_origin, dim_k, out_feats, chunk_rows)) return 0;
    const LinLayout L = lin_layout(num_rows, dim_origin, out_feats, chunk_rows, false);
    return L.n_tiles > 1 ? al256((size_t)L.n_tiles * num_rows * dim_k * sizeof(float)) : 0;
}

extern "C" int maxk_cbsr_linear_backward_values(const float *grad_out, const uint8_t *cbsr_idx,
                                                const float *weight, float *grad_val,
                                                int64_t num_rows, int32_t dim_origin,
                                                int32_t dim_k, int64_t out_feats,
                                                int32_t chunk_rows, void *workspace,
                                                size_t workspace_bytes, void *stream) {
    clear_error();
    if (int rc = check_lin_shape(num_rows, dim_origin, dim_k, out_feats, chunk_rows)) return rc;
    if (num_rows == 0) return MAXK_OK;
    MAXK_REQUIRE(grad_out && cbsr_idx && weight && grad_val,
                 "grad_out / cbsr_idx / weight / grad_val must not be NULL");
    MAXK_REQUIRE((((uintptr_t)grad_out | (uintptr_t)weight | (uintptr_t)grad_val) & 3) == 0,
                 "grad_out / weight / grad_val must be 4-B aligned");
    const LinLayout L = lin_layout(num_rows, dim_origin, out_feats, chunk_rows, false);
    if (int rc = check_lin_workspace(workspace, workspace_bytes,
                                     maxk_cbsr_linear_backward_values_workspace_size(
                                         num_rows, dim_origin, dim_k, out_feats, chunk_rows)))
        return rc;
    float *out = L.n_tiles > 1 ? reinterpret_cast<float *>(workspace) : grad_val;
    hipStream_t s = as_stream(stream);
    const dim3 grid((unsigned)(L.n_tiles * L.P));
    auto launch = [&](auto cpl) {
        hipLaunchKernelGGL(lin_gval_kernel<decltype(cpl)::value>, grid, dim3(kLinBlock), L.lds, s,
                           grad_out, cbsr_idx, weight, out, (int)num_rows, dim_origin, dim_k,
                           (int)out_feats, L.chunk, L.n_items, L.P);
    };
    with_const<1, 2>(L.cpl, launch);
    MAXK_LAUNCHED("lin_gval_kernel");
    if (L.n_tiles > 1) {
        const int64_t n = num_rows * dim_k;
        hipLaunchKernelGGL(gval_sum_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0,
                           s, out, grad_val, n, L.n_tiles);
        MAXK_LAUNCHED("gval_sum_kernel");
    }
    return MAXK_OK;
}

extern "C" size_t maxk_cbsr_linear_backward_weight_workspace_size(int64_t num_rows,
                                                                  int32_t dim_origin,
                                                                  int32_t dim_k, int64_t out_feats,
                                                                  int32_t chunk_rows) {
    if (!lin_shape_ok(num_rows, dim_origin, dim_k, out_feats, chunk_rows)) return 0;
    const LinLayout L = lin_layout(num_rows, dim_origin, out_feats, chunk_rows, true);
    return al256((size_t)L.n_tiles * L.P * kWgOT * dim_origin * sizeof(float));
}

extern "C" int maxk_cbsr_linear_backward_weight(const float *grad_out, const float *cbsr_val,
                                                const uint8_t *cbsr_idx, float *grad_weight,
                                                int64_t num_rows, int32_t dim_origin,
                                                int32_t dim_k, int64_t out_feats,
                                                int32_t chunk_rows, void *workspace,
                                                size_t workspace_bytes, void *stream) {
    clear_error();
    if (int rc = check_lin_shape(num_rows, dim_origin, dim_k, out_feats, chunk_rows)) return rc;
    MAXK_REQUIRE(grad_weight && ((uintptr_t)grad_weight & 3) == 0,
                 "grad_weight must not be NULL and 4-B aligned");
    hipStream_t s = as_stream(stream);
    if (num_rows == 0) return zero_words(grad_weight, out_feats * dim_origin, s);
    MAXK_REQUIRE(grad_out && cbsr_val && cbsr_idx,
                 "grad_out / cbsr_val / cbsr_idx must not be NULL");
    MAXK_REQUIRE((((uintptr_t)grad_out | (uintptr_t)cbsr_val) & 3) == 0,
                 "grad_out / cbsr_val must be 4-B aligned");
    const LinLayout L = lin_layout(num_rows, dim_origin, out_feats, chunk_rows, true);
    if (int rc = check_lin_workspace(workspace, workspace_bytes,
                                     maxk_cbsr_linear_backward_weight_workspace_size(
                                         num_rows, dim_origin, dim_k, out_feats, chunk_rows)))
        return rc;
    float *part = reinterpret_cast<float *>(workspace);
    hipLaunchKernelGGL(lin_wgrad_kernel, dim3((unsigned)(L.n_tiles * L.P)), dim3(kLinBlock), L.lds,
                       s, grad_out, cbsr_val, cbsr_idx, part, (int)num_rows, dim_origin, dim_k,
                       (int)out_feats, L.chunk, L.n_items, L.P);
    MAXK_LAUNCHED("lin_wgrad_kernel");
    hipLaunchKernelGGL(wgrad_sum_kernel,
                       dim3((unsigned)ceil_div(out_feats * dim_origin, kBlock)), dim3(kBlock), 0,
                       s, part, grad_weight, (int)out_feats, dim_origin, L.P);
    MAXK_LAUNCHED("wgrad_sum_kernel");
    return MAXK_OK;
}

// Where the forward and the value gradient beat the dense products they replace
// (profiles/r24/cbsr_linear/).  Not a rule for the weight gradient, which loses nearly everywhere,
// and so not for a step that runs all three: maxk_hip.h says what was measured.
extern "C" int maxk_cbsr_linear_route(int32_t dim_origin, int32_t dim_k, int64_t out_feats) {
    return dim_origin >= 1 && dim_origin <= kMaxDim && dim_k >= 1 && out_feats >= 1 &&
           dim_k * MAXK_LIN_ROUTE_DIV <= dim_origin;
}
