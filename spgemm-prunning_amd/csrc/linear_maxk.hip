// Fused linear + MaxK for gfx950: cbsr = topk_k(x [V, I] @ W^T (+ b)), W [D, I] row-major.  An
// fp32 MFMA GEMM whose epilogue runs the MaxK row selection on the accumulators, so the dense
// hidden matrix h [V, D] never reaches memory (maxk_hip.h has the contract).
//
// Ownership.  A workgroup of four waves owns a tile of 64 whole rows x all D columns, and a
// wave owns 16 of those rows x all columns: a row's top-k never crosses waves, so the selection
// needs no workgroup barrier and no hand-over.  (The alternative, 64 x 64 subtiles of
// v_mfma_f32_32x32x2_f32, spreads a row over four waves and needs both.)
//
// Inner loop.  v_mfma_f32_16x16x4_f32: A = x[16 rows, 4 k] with lane l holding row l % 16 at
// k-position l / 16, B = W^T[4 k, 16 columns] with lane l holding column l % 16 at k-position
// l / 16, C[16, 16] in 4 registers, lane l register r = row 4 (l / 16) + r, column l % 16.  The
// columns are cut into NB = 4, 8 or 16 blocks of 16 (D <= 64, 128, 256): 4 NB accumulator
// registers.  x and W are staged through LDS in K-slabs of 32 columns, rows 36 words apart: a
// lane reads 16 B, its row's k-positions 16 s + 4 (l / 16) + (0..3), and uses them in four
// MFMAs -- x and W read the same positions, so the products pair up, and with 36 j mod 64
// taking each multiple of 4 once the 16 lanes of a k-position cover the 64 banks exactly.  Per
// 16 k-positions a wave reads 1 + NB x 16 B per lane and issues 4 NB MFMAs.  The K tail (I not
// a multiple of 32) and the column tail (D < 16 NB) are zeros in LDS: the loop has no branch
// on either.  A row's sum over I is therefore in one fixed order whatever V, the row's place in
// its tile or the tile's place in the grid: slab by slab, position by position, the MFMA's own
// 4-term sum inside.
//
// Staging.  One slab buffer (W [16 NB, 36] + x [64, 36] words, 45 KB at NB = 16), filled from
// registers: each thread loads the next slab's NB / 2 + 2 16-byte pieces (VEC: I, ld_x and the
// pointers allow 16-byte loads; otherwise four scalar loads a piece) before the current slab's
// MFMAs and stores them after the barrier that follows them.  The slab after a tile's last is
// the next tile's first, so its loads fly during the epilogue.  Loads are unconditional at
// clamped rows and columns and masked afterwards.
//
// Epilogue.  The bias is added to the accumulators (lane = column), which then go to the wave's
// [16, 16 NB + 4] rows of an LDS tile that aliases the slab buffer (one barrier).  Rows are read
// back in the selection's layouts: for k <= MAXK_TOPK_ROWS4_KMAX four rows a step, 16 lanes a
// row, columns 64 i + 4 q + j (16-byte reads) into rows4_take / rows4_emit; above it one row a
// step, column lane + 64 i, into wave_row_select (topk_select.h, the encode's own bodies).
// What is stored is the fp32 sum that was ranked.
//
// Budget at NB = 16: LDS 64 x 260 x 4 = 66,560 B tile + at most 11,520 B of winners = 78,080 B,
// two workgroups per CU (the radix select's 256-word histogram lives in the row it has just
// read); 64 accumulator + 40 prefetch registers, capped at 256 for two waves per SIMD.  The
// second workgroup's MFMAs run under the first one's selection and barriers.
#include "common.h"
#include "topk_select.h"

namespace maxk {
namespace {

constexpr int kLmWaveRows = 16;                          // one MFMA row block
constexpr int kLmTile = kLmWaveRows * kWavesPerBlock;    // rows per workgroup tile
constexpr int kLmKS = 32;                                // K-slab columns
constexpr int kLmLd = kLmKS + 4;                         // slab row stride in words
constexpr int kLmF4 = kLmKS / 4;                         // 16-byte pieces per slab row
constexpr int kLmXF4 = kLmTile * kLmF4 / kBlock;         // x pieces per thread and slab
constexpr int kLmSelSlots = kMaxDim + kWave;             // wave_row_select's slots
constexpr int kLmWaveSelWords = 2 * kLmSelSlots + kLmSelSlots / 4;  // keys, values, columns
#ifndef MAXK_LM_WGS_PER_CU  // grid: resident workgroups per CU the tile loop is spread over
#define MAXK_LM_WGS_PER_CU 2
#endif

__host__ __device__ constexpr int lm_tile_ld(int nb) { return 16 * nb + 4; }
// words of the slab buffer and the epilogue tile that share the front of the LDS
__host__ __device__ constexpr int lm_front_words(int nb) {
    const int slab = (16 * nb + kLmTile) * kLmLd, tile = kLmTile * lm_tile_ld(nb);
    return slab > tile ? slab : tile;
}

// row[c .. c + 3], 0 at and past I or when !rowok.  Unconditional loads at clamped columns.
template <bool VEC>
__device__ __forceinline__ float4 lm_load4(const float *__restrict__ row, int c, int I,
                                           bool rowok) {
    float4 f;
    if constexpr (VEC) {  // I % 4 == 0: a piece is inside or outside as a whole
        f = *reinterpret_cast<const float4 *>(row + (c < I ? c : I - 4));
        if (!(rowok && c < I)) f = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        const float a = row[c < I ? c : I - 1], b = row[c + 1 < I ? c + 1 : I - 1],
                    d = row[c + 2 < I ? c + 2 : I - 1], e = row[c + 3 < I ? c + 3 : I - 1];
        f = make_float4(rowok && c < I ? a : 0.f, rowok && c + 1 < I ? b : 0.f,
                        rowok && c + 2 < I ? d : 0.f, rowok && c + 3 < I ? e : 0.f);
    }
    return f;
}

// The wave's 16 tile rows through the four-rows-per-wave selection.
template <int NB, int J>
__device__ __forceinline__ void lm_select_rows4(const float *my, int row_base, int num_rows,
                                                int D, int k, uint32_t *wl,
                                                float *__restrict__ out_val,
                                                uint8_t *__restrict__ out_idx, uint32_t &n_bad) {
    constexpr int TLD = lm_tile_ld(NB);
    const int lane = lane_id();
    const int sub = lane >> 4, q = lane & 15;
    const int k4 = (k + 3) & ~3;
    uint32_t *wkey = wl + sub * (3 * k4), *wval = wkey + k4, *wcol = wval + k4;
    bool ok[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) ok[t] = 64 * (t >> 2) + 4 * q + (t & 3) < D;
#pragma unroll 1
    for (int g = 0; g < kLmWaveRows / 4; ++g) {
        const int rl = 4 * g + sub, row = row_base + rl;
        float v[16];
        uint32_t key[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < NB / 4)  // the tile has 16 NB columns
                f = *reinterpret_cast<const float4 *>(my + rl * TLD + 64 * i + 4 * q);
            v[4 * i] = f.x;
            v[4 * i + 1] = f.y;
            v[4 * i + 2] = f.z;
            v[4 * i + 3] = f.w;
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) key[t] = ok[t] ? order_key(v[t]) : 0u;
        bool take[16];
        const bool live = row < num_rows;
        rows4_take<J>(key, ok, k, q, live, take, n_bad);
        rows4_emit<float>(v, key, take, k, q, live, row, wkey, wval, wcol, out_val, out_idx,
                          nullptr);
    }
}

// ... and through the wave-per-row radix select.
template <int NB>
__device__ __forceinline__ void lm_select_wave(float *my, int row_base, int num_rows, int D,
                                               int k, uint32_t *wl, float *__restrict__ out_val,
                                               uint8_t *__restrict__ out_idx,
                                               uint32_t *bad_rows) {
    constexpr int TLD = lm_tile_ld(NB);
    const int lane = lane_id();
    uint32_t *skey = wl;
    float *sval = reinterpret_cast<float *>(wl + kLmSelSlots);
    uint8_t *scol = reinterpret_cast<uint8_t *>(wl + 2 * kLmSelSlots);
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ok[i] = lane + kWave * i < D;
#pragma unroll 1
    for (int r = 0; r < kLmWaveRows; ++r) {
        const int row = row_base + r;
        if (row >= num_rows) break;  // wave-uniform
        float v[4];
        uint32_t key[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = (i < NB / 4 && ok[i]) ? my[r * TLD + lane + kWave * i] : 0.f;
            key[i] = ok[i] ? order_key(v[i]) : 0u;
        }
        wave_lds_fence();
        // NB = 16: the row is in registers now and its 260 words serve as the histogram
        uint32_t *hist = NB == 16 ? reinterpret_cast<uint32_t *>(my + r * TLD)
                                  : wl + kLmWaveSelWords;
        wave_row_select<float>(v, key, ok, k, lane, row, D, hist, skey, sval, scol, out_val,
                               out_idx, nullptr, nullptr, bad_rows);
    }
}

template <int NB, bool VEC>
__global__ __launch_bounds__(kBlock, MAXK_LM_WGS_PER_CU) void linear_maxk_kernel(
    const float *__restrict__ x, int64_t ld_x, const float *__restrict__ w,
    const float *__restrict__ bias, float *__restrict__ out_val, uint8_t *__restrict__ out_idx,
    uint32_t *bad_rows, int num_rows, int I, int D, int k, int n_tiles, int wave_sel_words) {
    extern __shared__ __attribute__((aligned(16))) float lds_lm[];
    constexpr int DP = 16 * NB, TLD = lm_tile_ld(NB);
    constexpr int WF4 = DP * kLmF4 / kBlock;  // W pieces per thread and slab
    float *ws = lds_lm;                       // [DP][kLmLd]
    float *xs = lds_lm + DP * kLmLd;          // [kLmTile][kLmLd]
    const int tid = threadIdx.x, wid = tid / kWave, lane = lane_id();
    float *my = lds_lm + wid * kLmWaveRows * TLD;  // the wave's rows of the epilogue tile
    uint32_t *wl = reinterpret_cast<uint32_t *>(lds_lm + lm_front_words(NB)) +
                   (size_t)wid * wave_sel_words;
    const int pr = tid / kLmF4, pc = 4 * (tid % kLmF4);  // this thread's piece: row, column
    constexpr int kRowStep = kBlock / kLmF4;             // rows between a thread's pieces
    const int frag = (lane & 15) * kLmLd + 4 * (lane >> 4);  // MFMA operand: row, k-position

    float4 pw[WF4], px[kLmXF4];
    auto load_slab = [&](int tile, int k0) {
#pragma unroll
        for (int u = 0; u < WF4; ++u) {
            const int r = pr + kRowStep * u;
            pw[u] = lm_load4<VEC>(w + (r < D ? r : D - 1) * I, k0 + pc, I, r < D);  // < 2^31
        }
#pragma unroll
        for (int u = 0; u < kLmXF4; ++u) {
            const int64_t r = (int64_t)tile * kLmTile + pr + kRowStep * u;
            px[u] = lm_load4<VEC>(x + (r < num_rows ? r : num_rows - 1) * ld_x, k0 + pc, I, true);
        }
    };
    uint32_t n_bad = 0;
    load_slab(blockIdx.x, 0);
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        f32x4 acc[NB];
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < I; k0 += kLmKS) {
            __syncthreads();  // the slab (or the epilogue tile) in LDS is no longer read
#pragma unroll
            for (int u = 0; u < WF4; ++u)
                *reinterpret_cast<float4 *>(ws + (pr + kRowStep * u) * kLmLd + pc) = pw[u];
#pragma unroll
            for (int u = 0; u < kLmXF4; ++u)
                *reinterpret_cast<float4 *>(xs + (pr + kRowStep * u) * kLmLd + pc) = px[u];
            __syncthreads();
            const bool last = k0 + kLmKS >= I;  // then the next tile's first slab (rows clamped)
            load_slab(last ? tile + (int)gridDim.x : tile, last ? 0 : k0 + kLmKS);
#pragma unroll
            for (int s = 0; s < kLmKS / 16; ++s) {
                const float4 a =
                    *reinterpret_cast<const float4 *>(xs + wid * kLmWaveRows * kLmLd + frag + 16 * s);
#pragma unroll
                for (int c0 = 0; c0 < NB; c0 += 4) {
                    float4 b[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        b[c] = *reinterpret_cast<const float4 *>(ws + (c0 + c) * 16 * kLmLd + frag +
                                                                 16 * s);
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        acc[c0 + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[c].x, acc[c0 + c], 0, 0, 0);
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        acc[c0 + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[c].y, acc[c0 + c], 0, 0, 0);
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        acc[c0 + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[c].z, acc[c0 + c], 0, 0, 0);
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        acc[c0 + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[c].w, acc[c0 + c], 0, 0, 0);
                }
            }
        }
        // ---- epilogue: bias, accumulators -> the wave's tile rows, selection
        if (bias) {
#pragma unroll
            for (int cb = 0; cb < NB; ++cb) {
                const int col = cb * 16 + (lane & 15);
                const float bv = bias[col < D ? col : D - 1];  // columns past D are never ranked
                acc[cb] += f32x4{bv, bv, bv, bv};
            }
        }
        __syncthreads();  // every wave has read the last slab: the tile takes its place
#pragma unroll
        for (int cb = 0; cb < NB; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                my[(4 * (lane >> 4) + r) * TLD + cb * 16 + (lane & 15)] = acc[cb][r];
        wave_lds_fence();
        const int row_base = tile * kLmTile + wid * kLmWaveRows;
        if (k <= 32)
            lm_select_rows4<NB, 2>(my, row_base, num_rows, D, k, wl, out_val, out_idx, n_bad);
        else if (k <= MAXK_TOPK_ROWS4_KMAX)
            lm_select_rows4<NB, 4>(my, row_base, num_rows, D, k, wl, out_val, out_idx, n_bad);
        else
            lm_select_wave<NB>(my, row_base, num_rows, D, k, wl, out_val, out_idx, bad_rows);
    }
    if (n_bad) atomicAdd(bad_rows, n_bad);  // maxk_topk_error_rows
}

// per-wave words of the selection's LDS, after the tile
int lm_wave_sel_words(int nb, int k) {
    if (k <= MAXK_TOPK_ROWS4_KMAX) return 4 * 3 * ((k + 3) & ~3);  // four rows of winners
    return kLmWaveSelWords + (nb == 16 ? 0 : 256);                 // ... + the histogram
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" int maxk_linear_maxk_forward(const float *x, int64_t ld_x, const float *weight,
                                        const float *bias, float *cbsr_val, uint8_t *cbsr_idx,
                                        int64_t num_rows, int32_t in_dim, int32_t dim, int32_t k,
                                        void *stream) {
    clear_error();
    MAXK_REQUIRE(num_rows >= 0 && num_rows < (1LL << 31) - kLmTile, "num_rows out of range");
    MAXK_REQUIRE(dim >= 1 && dim <= kMaxDim, "dim must be in [1,256], got %d", dim);
    MAXK_REQUIRE(k >= 1 && k <= dim, "k must be in [1,dim], got %d", k);
    MAXK_REQUIRE(in_dim >= 1 && in_dim < (1 << 23), "in_dim must be in [1,2^23), got %d", in_dim);
    MAXK_REQUIRE(ld_x >= in_dim, "ld_x (%lld) < in_dim (%d)", (long long)ld_x, in_dim);
    if (num_rows == 0) return MAXK_OK;
    MAXK_REQUIRE(x && weight && cbsr_val && cbsr_idx,
                 "x / weight / cbsr_val / cbsr_idx must not be NULL");
    MAXK_REQUIRE((((uintptr_t)x | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)cbsr_val) & 3) ==
                     0, "x / weight / bias / cbsr_val must be 4-B aligned");
    uint32_t *bad = topk_bad_rows_counter();
    MAXK_REQUIRE(bad, "the top-k bad-row counter has no device address");
    const int nb = dim <= 64 ? 4 : (dim <= 128 ? 8 : 16);
    const bool vec = in_dim % 4 == 0 && ld_x % 4 == 0 &&
                     (((uintptr_t)x | (uintptr_t)weight) & 15) == 0;
    const int64_t n_tiles = ceil_div(num_rows, kLmTile);
    const int64_t slots = device_cus() * MAXK_LM_WGS_PER_CU;
    const dim3 grid((unsigned)(n_tiles < slots ? n_tiles : slots));
    const int sel = lm_wave_sel_words(nb, k);
    const size_t lds = ((size_t)lm_front_words(nb) + (size_t)kWavesPerBlock * sel) * 4;
    MAXK_REQUIRE(lds <= kPullLdsBytes, "LDS need %zu B exceeds the workgroup's", lds);
    auto launch = [&](auto nbc) {
        constexpr int NB = decltype(nbc)::value;
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, as_stream(stream), x, ld_x, weight,
                               bias, cbsr_val, cbsr_idx, bad, (int)num_rows, in_dim, dim, k,
                               (int)n_tiles, sel);
        };
        vec ? go(linear_maxk_kernel<NB, true>) : go(linear_maxk_kernel<NB, false>);
    };
    with_const<4, 8, 16>(nb, launch);
    MAXK_LAUNCHED("linear_maxk_kernel");
    return MAXK_OK;
}

// Where the fused forward beats torch.addmm followed by maxk_topk_cbsr: nowhere.  At the 24
// measured points (profiles/r25/linear_maxk/: 233 K and 2.45 M rows, in_dim 100 / 256 / 602,
// dim 256, k 8 / 16 / 32 / 64) the pair is faster at 23 and level at one, so the answer is 0
// for every shape; what the fused call saves is memory, the [num_rows, dim] product.
extern "C" int maxk_linear_maxk_route(int64_t num_rows, int32_t in_dim, int32_t dim, int32_t k) {
    (void)num_rows, (void)in_dim, (void)dim, (void)k;
    return 0;
}
