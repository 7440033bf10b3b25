// Backward SSpMM, the push (the forms and their formula: sspmm_bwd.h).
// Phase 1 walks the CSR of A and, per edge, either adds its k values to grad_cbsr with global
// fp32 atomics (maxk_sspmm_backward: each G row staged once in LDS; MI355X executes float
// atomics memory-side and they are bound by request count, ~6 ms for Reddit-sized at any k in
// 2..16) or stores them as a contribution row T[e] in CSR edge order (non-temporal 16-B buffer
// stores, so the 7.3 GB stream does not evict the selector table every edge gathers from).
// The csc phase 2 (maxk_sspmm_backward_csc) gathers a destination's rows through the CSC
// permutation and sums them in a fixed order.
// Both phases use the token-stream work partition of token_items.h (one wave per item of C
// tokens) under its cut-at-the-item's-end rule: an item walks exactly the edges, or CSC slots,
// whose tokens it holds.  Loads-in-flight depth per launch from the average degree
// (pick_depth).
#include "sspmm_bwd.h"

namespace maxk {
namespace {

enum { kAtomic = 0, kStore = 1, kStoreX4 = 2, kStoreX4W = 3, kStoreX4S = 4 };

// A contribution row's 16 B in phase 2.  NT: rows of whole 128-B lines (k % 32 == 0) are read
// once, so non-temporally -- ogbn-products-sized csc backward k = 32 7.85 -> 7.77 ms, with the
// selector stream 6.71 -> 6.60, k = 64 15.14 -> 14.75; rows sharing a line (k <= 16) need
// the line kept for the other row, and lose 3-6 % that way (Reddit-sized csc k = 16 3.86 ->
// 4.10, products k = 16 5.17 -> 5.37, bsort k = 8 3.06 -> 3.15; profiles/r06/tune/t_load_nt/).
template <bool NT>
__device__ __forceinline__ float4 t_load4(const float4 *p) {
    if constexpr (NT)
        return __builtin_bit_cast(float4,
                                  __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p)));
    return *p;
}

// kStoreX4 (k % 4 == 0): LR = pow2ceil(k/4) lanes per edge, each lane owning 4
// consecutive l: one u32 selector load, four LDS reads, one 16-B store; 64/LR
// edges per wave step (4x fewer memory instructions per edge than one l per
// lane).  All memory goes through wave-uniform buffer descriptors with 32-bit
// offsets (wave_buffer, common.h), which keeps 64-bit address math out of the loop:
//  * col_idx / edge_val over the segment [sb, se): the lane's offset is fixed per
//    batch and the step's part is the instruction's immediate; past se the loads
//    return 0 (column 0, weight 0), so nothing is clamped;
//  * the selector table: offset c*k + 4q, one 24-bit multiply-add (kStoreX4W, for
//    tables past 2^24 columns, a 32-bit multiply);
//  * T rows [sb, se): past se, or for lanes q >= k/4 (offset pushed past 2^31), the
//    hardware drops the store, so no store is predicated.
// Cache policy of the T stores: MAXK_T_AUX (0 plain, 2 nt, 16 sc1).  Store lag as in
// push_edges below.
// ES (edge selectors, maxk_sspmm_backward_csc_sel): the selectors come as a per-edge stream
// esel[e * k + l] (= cbsr_idx[col_idx[e], l]) read in CSR order beside the weights, instead
// of a gather of the destination's row of cbsr_idx per edge: no column loads and no random
// selector line per edge (an ogbn-products-sized table is 20-80 MB, and each gather moved a
// whole 128-B line from the Infinity Cache).
template <int LR, int U, bool WIDE, bool ES = false>
__device__ __forceinline__ void push_x4(const float *g_lds, const int32_t *__restrict__ col_idx,
                                        const float *__restrict__ edge_val,
                                        const uint8_t *__restrict__ cbsr_idx,
                                        float *__restrict__ T, int sb, int se, int k, int lane,
                                        const uint8_t *__restrict__ esel = nullptr) {
    constexpr int G = kWave / LR;
    constexpr int GU = G * U;
    const int grp = lane / LR;
    const int q = lane % LR;
    const int k4 = k >> 2;
    const int n = se - sb;  // wave-uniform, <= chunk
    const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
    const auto vrs = wave_buffer(edge_val + sb, (uint32_t)n * 4u);
    // ES: the segment's selector stream; else the table (offsets < num_cols*k < 2^31)
    const auto srs = ES ? wave_buffer(esel + (size_t)(uint32_t)sb * k, (uint32_t)n * k)
                        : wave_buffer(cbsr_idx, 0xffffffffu);
    const auto trs = wave_buffer(T + (size_t)(uint32_t)sb * k, (uint32_t)n * k * 4u);  // <= 2 MiB
    const uint32_t qsel = 4u * (uint32_t)(q < k4 ? q : k4 - 1);
    const uint32_t qst = q < k4 ? 16u * q : 0x80000000u;  // store offset term; past the end if idle
    const uint32_t kb = 4u * (uint32_t)k;                    // T row bytes
    auto sel_off = [&](int c) -> int {
        return WIDE ? (int)((uint32_t)c * (uint32_t)k + qsel)
                    : (int)(__umul24((uint32_t)c, (uint32_t)k) + qsel);
    };
    int c[U];
    float w[U];
    {
        const int lo = grp * 4;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ES) c[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(crs, lo + u * G * 4, 0, 0);
            w[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vrs, lo + u * G * 4, 0, 0));
        }
    }
    u32x4 xp[U];
    uint32_t sto = 0;  // T byte offset of the pending batch's step 0 for this lane
    bool pending = false;
    for (int base = 0;; base += GU) {  // base: edge offset inside the segment
        const bool has_next = base + GU < n;  // wave-uniform
        int cn[U];
        float wn[U];
        if (has_next) {
            const int lo = (base + GU + grp) * 4;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ES)
                    cn[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(crs, lo + u * G * 4, 0, 0);
                wn[u] = __uint_as_float(
                    __builtin_amdgcn_raw_buffer_load_b32(vrs, lo + u * G * 4, 0, 0));
            }
        }
        uint32_t sv[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            sv[u] = __builtin_amdgcn_raw_buffer_load_b32(
                srs, ES ? (int)((uint32_t)(base + u * G + grp) * (uint32_t)k + qsel)
                        : sel_off(c[u]), 0, 0);
        if (pending) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                __builtin_amdgcn_raw_buffer_store_b128(xp[u], trs, (int)(sto + u * G * kb), 0,
                                                       MAXK_T_AUX);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t s = sv[u];
            xp[u].x = __float_as_uint(w[u] * g_lds[s & 255u]);
            xp[u].y = __float_as_uint(w[u] * g_lds[(s >> 8) & 255u]);
            xp[u].z = __float_as_uint(w[u] * g_lds[(s >> 16) & 255u]);
            xp[u].w = __float_as_uint(w[u] * g_lds[s >> 24]);
        }
        sto = (uint32_t)(base + grp) * kb + qst;
        pending = true;
        if (!has_next) break;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ES) c[u] = cn[u];
            w[u] = wn[u];
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
        __builtin_amdgcn_raw_buffer_store_b128(xp[u], trs, (int)(sto + u * G * kb), 0, MAXK_T_AUX);
}

// Walk edges [sb, se) (sb < se) of one staged row.  All loads are
// unconditional (clamped addresses).
//  kAtomic: one predicated global fp32 atomic per (edge, l).
//  kStore (k <= KG): contribution rows go to T in CSR edge order with a
//    one-batch store lag.  On gfx950 stores count in vmcnt with the loads, so a
//    wait for a load drains every OLDER store: per batch the order is
//    [prefetch col/val of batch i+1] [selector loads of batch i] [stores of
//    batch i-1] [wait selectors] -> the stores in flight are always younger than
//    the loads being waited for.  Masked lanes store to the dummy row of T, so
//    no store is predicated (a predicated store becomes a branch + full wait).
template <int KG, int U, int MODE>
__device__ __forceinline__ void push_edges(const float *g_lds, const int32_t *__restrict__ col_idx,
                                           const float *__restrict__ edge_val,
                                           const uint8_t *__restrict__ cbsr_idx,
                                           float *__restrict__ dst, int dummy, int sb, int se,
                                           int k, int lane, const uint8_t *__restrict__ esel) {
    if constexpr (MODE == kStoreX4S) {
        push_x4<KG, U, false, true>(g_lds, col_idx, edge_val, cbsr_idx, dst, sb, se, k, lane,
                                    esel);
        return;
    }
    if constexpr (MODE == kStoreX4 || MODE == kStoreX4W) {
        push_x4<KG, U, MODE == kStoreX4W>(g_lds, col_idx, edge_val, cbsr_idx, dst, sb, se, k, lane);
        return;
    }
    constexpr int G = kWave / KG;
    constexpr int GU = G * U;
    const int grp = lane / KG;
    const int l0 = lane % KG;
    const int last = se - 1;
    int c[U];
    float w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int e = sb + u * G + grp;
        const int ec = e < se ? e : last;
        c[u] = col_idx[ec];
        w[u] = edge_val[ec];
    }
    if (MODE == kStore && k <= KG) {
        const bool lok = l0 < k;
        const int lc = lok ? l0 : k - 1;
        float xp[U] = {};
        int rp[U];  // T row of each pending store (dummy for masked lanes)
        bool pending = false;
        for (int base = sb;; base += GU) {
            const bool has_next = base + GU < se;  // wave-uniform
            int cn[U];
            float wn[U];
            if (has_next) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int e = base + GU + u * G + grp;
                    const int ec = e < se ? e : last;
                    cn[u] = col_idx[ec];
                    wn[u] = edge_val[ec];
                }
            }
            int s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s[u] = cbsr_idx[c[u] * k + lc];
            }
            if (pending) {
#pragma unroll
                for (int u = 0; u < U; ++u) dst[(size_t)(uint32_t)rp[u] * k + lc] = xp[u];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = base + u * G + grp;
                xp[u] = w[u] * g_lds[s[u]];
                rp[u] = (e < se && lok) ? e : dummy;
            }
            pending = true;
            if (!has_next) break;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                c[u] = cn[u];
                w[u] = wn[u];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) dst[(size_t)(uint32_t)rp[u] * k + lc] = xp[u];
        return;
    }
    for (int base = sb;; base += GU) {
        const bool has_next = base + GU < se;  // wave-uniform
        for (int lb = 0; lb < k; lb += KG) {
            const int l = lb + l0;
            const bool lok = l < k;
            const int lc = lok ? l : k - 1;
            int s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = cbsr_idx[c[u] * k + lc];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = base + u * G + grp;
                const float x = w[u] * g_lds[s[u]];
                if (MODE == kAtomic) {
                    if (e < se && lok) atomicAdd(&dst[c[u] * k + l], x);
                } else {
                    dst[(size_t)(uint32_t)((e < se && lok) ? e : dummy) * k + (lok ? l : 0)] = x;
                }
            }
        }
        if (!has_next) break;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = base + GU + u * G + grp;
            const int ec = e < se ? e : last;
            c[u] = col_idx[ec];
            w[u] = edge_val[ec];
        }
    }
}

template <int KG, int U, int MODE>
__global__ __launch_bounds__(kBlock, MAXK_BWD_WAVES) void sspmm_bwd_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const float *__restrict__ edge_val, const float *__restrict__ grad,
    const float *__restrict__ row_div, const uint8_t *__restrict__ cbsr_idx,
    float *__restrict__ dst, int num_rows, int64_t num_e, int D, int k, int chunk, int n_items,
    const uint8_t *__restrict__ esel) {
    __shared__ __attribute__((aligned(16))) float lds[kWavesPerBlock][kMaxDim];
    const int wid = threadIdx.x / kWave;
    const int lane = lane_id();
    // MAXK_P1_XCD: XCD-contiguous items, as in the forward (an ordered graph's destinations,
    // whose selectors every edge reads, then stay close within one XCD)
    const int blk = MAXK_P1_XCD ? xcd_contiguous_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int item = blk * kWavesPerBlock + wid;
    if (item >= n_items) return;
    float *g_lds = lds[wid];
    *reinterpret_cast<float4 *>(&g_lds[lane * 4]) = make_float4(0.f, 0.f, 0.f, 0.f);

    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);
    // Rows q = r-1 (continuation), r, r+1, ...: each one's piece under CutAtEnd.  row_ptr /
    // row_div of 64 consecutive rows sit one per lane (read with readlane), and each row's G
    // values (4 per lane, columns lane + 64*i) are loaded while the previous row's edges are
    // pushed: no per-row dependent load before a row can start.
    int q = it.r > 0 ? it.r - 1 : 0;
    PtrWindow win{row_ptr, num_rows, 0, 0};
    win.load(q, lane);
    float dvw = row_div ? row_div[q + lane < num_rows ? q + lane : num_rows - 1] : 1.f;
    auto load_g = [&](int row, float (&g)[4]) {
        const float *gr = grad + (int64_t)(row < num_rows ? row : num_rows - 1) * D;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = lane + kWave * i;
            g[i] = gr[j < D ? j : D - 1];
        }
    };
    float gn[4];
    load_g(q, gn);
    for (; q < num_rows; ++q) {
        if (win.slide(q, lane) && row_div)  // the divisor window moves with it
            dvw = row_div[q + lane < num_rows ? q + lane : num_rows - 1];
        const int rb = win.begin(q);
        const int re = win.end(q);
        if (!row_owned(it.d1, q, rb)) break;
        float g[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = gn[i];
        if (q + 1 < num_rows) load_g(q + 1, gn);
        const RowPiece p = any_piece(CutAtEnd{}, it.d0, it.d1, q, rb, re);
        if (p.sb >= p.se) continue;
        const float div = __builtin_bit_cast(
            float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dvw), q - win.wb));
        wave_lds_fence();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = lane + kWave * i;
            if (j < D) g_lds[j] = row_div ? g[i] / div : g[i];
        }
        wave_lds_fence();
        push_edges<KG, U, MODE>(g_lds, col_idx, edge_val, cbsr_idx, dst, (int)num_e, (int)p.sb,
                                (int)p.se, k, lane, esel);
    }
}

// ---- H heads (maxk_sspmm_backward_heads): edge_val [H, num_e], grad [H, num_rows, D] --------
// The kStore phase 1 with the heads summed per edge before anything is stored,
//   T[e, l] = sum_h w[h, e] * G[h, r, sel[c, l]] / row_div[r]     (c = col_idx[e], e in row r),
// so an edge costs one column load, one selector gather and one contribution row whatever H;
// phase 2 (csc_sum_kernel) then runs as for one head.  Per row piece the H rows G[h, r, :] /
// row_div[r] are staged side by side in the wave's LDS (g_lds[h * DS + j], DS = heads_stride(D):
// H * DS floats per wave, 8.3 KB at H = 8, D = 256; the pad columns [D, DS) hold zeros).  A
// selector byte >= D is clamped to the last pad column (`trash`): with rows at a stride below
// 256 it would otherwise read the next head's row.  Per edge and l the sum is formed in head
// order, x = w[0] * g_0[s], then x = fma(w[h], g_h[s], x): at H == 1 the one product the
// single-head kernel stores.
// The weights of a batch, U * H per lane, are loaded with the batch's selectors and held in
// registers (w[U][HB], HB = 4 or 8 >= H: the loops over heads are unrolled to HB under
// wave-uniform h < H tests, so no array is indexed by a run-time value), which keeps the order
// [columns of batch i+1] [selectors and weights of batch i] [stores of batch i-1] [wait]: the
// stores in flight are younger than every load being waited for, as in push_edges.

// LDS row stride of one head: D rounded up to 4 floats plus 4 zeroed pad floats (16-B rows).
__host__ __device__ inline int heads_stride(int D) { return (D + 3) / 4 * 4 + 4; }

// x[i] (+)= w * g[s_i] for the four selector bytes of sv, each clamped to the trash column
template <bool FIRST>
__device__ __forceinline__ void heads_term4(float (&x)[4], float w, const float *g, uint32_t sv,
                                            uint32_t trash) {
    const uint32_t s[4] = {sv & 255u, (sv >> 8) & 255u, (sv >> 16) & 255u, sv >> 24};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float gv = g[s[i] < trash ? s[i] : trash];
        x[i] = FIRST ? w * gv : __builtin_fmaf(w, gv, x[i]);
    }
}

// k % 4 == 0: push_x4 for H heads (LR = pow2ceil(k/4) lanes per edge, four l per lane, one u32
// selector load and one 16-B store per edge and lane).  Columns, weights and T rows go through
// buffer descriptors over the segment [sb, se): past se the loads return 0 (column 0, weight
// 0) and the stores are dropped, as are those of the idle lanes q >= k/4.
template <int LR, int U, int HB>
__device__ __forceinline__ void push_heads_x4(const float *g_lds, int DS,
                                              const int32_t *__restrict__ col_idx,
                                              const float *__restrict__ edge_val, int64_t num_e,
                                              int H, const uint8_t *__restrict__ cbsr_idx,
                                              float *__restrict__ T, int sb, int se, int k,
                                              int lane) {
    constexpr int G = kWave / LR;
    constexpr int GU = G * U;
    const int grp = lane / LR;
    const int q = lane % LR;
    const int k4 = k >> 2;
    const int n = se - sb;  // wave-uniform, <= chunk
    const uint32_t trash = (uint32_t)DS - 1u;
    const auto crs = wave_buffer(col_idx + sb, (uint32_t)n * 4u);
    __amdgpu_buffer_rsrc_t vrs[HB];
#pragma unroll
    for (int h = 0; h < HB; ++h)
        vrs[h] = wave_buffer(edge_val + (int64_t)(h < H ? h : 0) * num_e + sb, (uint32_t)n * 4u);
    const auto srs = wave_buffer(cbsr_idx, 0xffffffffu);  // offsets < num_cols * k < 2^31
    const auto trs = wave_buffer(T + (size_t)(uint32_t)sb * k, (uint32_t)n * k * 4u);
    const uint32_t qsel = 4u * (uint32_t)(q < k4 ? q : k4 - 1);
    const uint32_t qst = q < k4 ? 16u * q : 0x80000000u;  // store offset term; past the end if idle
    const uint32_t kb = 4u * (uint32_t)k;                    // T row bytes
    int c[U];
    {
        const int lo = grp * 4;
#pragma unroll
        for (int u = 0; u < U; ++u)
            c[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(crs, lo + u * G * 4, 0, 0);
    }
    u32x4 xp[U];
    uint32_t sto = 0;  // T byte offset of the pending batch's step 0 for this lane
    bool pending = false;
    for (int base = 0;; base += GU) {  // base: edge offset inside the segment
        const bool has_next = base + GU < n;  // wave-uniform
        int cn[U];
        if (has_next) {
            const int lo = (base + GU + grp) * 4;
#pragma unroll
            for (int u = 0; u < U; ++u)
                cn[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(crs, lo + u * G * 4, 0, 0);
        }
        uint32_t sv[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            sv[u] = __builtin_amdgcn_raw_buffer_load_b32(
                srs, (int)(__umul24((uint32_t)c[u], (uint32_t)k) + qsel), 0, 0);
        float w[U][HB];
        {
            const int lo = (base + grp) * 4;
#pragma unroll
            for (int h = 0; h < HB; ++h) {
                if (h < H) {
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        w[u][h] = __uint_as_float(
                            __builtin_amdgcn_raw_buffer_load_b32(vrs[h], lo + u * G * 4, 0, 0));
                }
            }
        }
        if (pending) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                __builtin_amdgcn_raw_buffer_store_b128(xp[u], trs, (int)(sto + u * G * kb), 0,
                                                       MAXK_T_AUX);
        }
        float x[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) heads_term4<true>(x[u], w[u][0], g_lds, sv[u], trash);
#pragma unroll
        for (int h = 1; h < HB; ++h) {
            if (h < H) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    heads_term4<false>(x[u], w[u][h], g_lds + h * DS, sv[u], trash);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            xp[u].x = __float_as_uint(x[u][0]);
            xp[u].y = __float_as_uint(x[u][1]);
            xp[u].z = __float_as_uint(x[u][2]);
            xp[u].w = __float_as_uint(x[u][3]);
        }
        sto = (uint32_t)(base + grp) * kb + qst;
        pending = true;
        if (!has_next) break;
#pragma unroll
        for (int u = 0; u < U; ++u) c[u] = cn[u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
        __builtin_amdgcn_raw_buffer_store_b128(xp[u], trs, (int)(sto + u * G * kb), 0, MAXK_T_AUX);
}

// Any k: KG = pow2ceil(k) lanes per edge (<= 64), one l per lane and pass, passes over l for
// k > 64.  All loads unconditional with clamped addresses; a masked lane (past se, or l >= k)
// stores to the dummy row T[num_e]; the stores of a pass are issued after the selector loads of
// the next one.
template <int KG, int U, int HB>
__device__ __forceinline__ void push_heads_scalar(const float *g_lds, int DS,
                                                  const int32_t *__restrict__ col_idx,
                                                  const float *__restrict__ edge_val,
                                                  int64_t num_e, int H,
                                                  const uint8_t *__restrict__ cbsr_idx,
                                                  float *__restrict__ T, int sb, int se, int k,
                                                  int lane) {
    constexpr int G = kWave / KG;
    constexpr int GU = G * U;
    const int grp = lane / KG;
    const int l0 = lane % KG;
    const int last = se - 1;
    const int dummy = (int)num_e;
    const int trash = DS - 1;
    int c[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int e = sb + u * G + grp;
        c[u] = col_idx[e < se ? e : last];
    }
    float xp[U] = {};
    int rp[U];   // T row of each pending store (dummy for masked lanes)
    int lp = 0;  // ... and its column
    bool pending = false;
    for (int base = sb;; base += GU) {
        const bool has_next = base + GU < se;  // wave-uniform
        int cn[U];
        if (has_next) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = base + GU + u * G + grp;
                cn[u] = col_idx[e < se ? e : last];
            }
        }
        float w[U][HB];
#pragma unroll
        for (int h = 0; h < HB; ++h) {
            if (h < H) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int e = base + u * G + grp;
                    w[u][h] = edge_val[(int64_t)h * num_e + (e < se ? e : last)];
                }
            }
        }
        for (int lb = 0; lb < k; lb += KG) {  // one pass unless k > 64
            const int l = lb + l0;
            const bool lok = l < k;
            const int lc = lok ? l : k - 1;
            int s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = cbsr_idx[c[u] * k + lc];
            if (pending) {
#pragma unroll
                for (int u = 0; u < U; ++u) T[(size_t)(uint32_t)rp[u] * k + lp] = xp[u];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s[u] = s[u] < trash ? s[u] : trash;
                xp[u] = w[u][0] * g_lds[s[u]];
            }
#pragma unroll
            for (int h = 1; h < HB; ++h) {
                if (h < H) {
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        xp[u] = __builtin_fmaf(w[u][h], g_lds[h * DS + s[u]], xp[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = base + u * G + grp;
                rp[u] = (e < se && lok) ? e : dummy;
            }
            lp = lc;
            pending = true;
        }
        if (!has_next) break;
#pragma unroll
        for (int u = 0; u < U; ++u) c[u] = cn[u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) T[(size_t)(uint32_t)rp[u] * k + lp] = xp[u];
}

// LG: lanes per edge (X4: pow2ceil(k/4), else pow2ceil(k)); HB: 4 or 8, >= H.
template <int LG, int U, int HB, bool X4>
__global__ __launch_bounds__(kBlock, MAXK_BWD_WAVES) void sspmm_bwd_heads_kernel(
    const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
    const float *__restrict__ edge_val, const float *__restrict__ grad,
    const float *__restrict__ row_div, const uint8_t *__restrict__ cbsr_idx,
    float *__restrict__ T, int num_rows, int64_t num_e, int D, int DS, int k, int chunk,
    int n_items, int H, int vec) {
    extern __shared__ __attribute__((aligned(16))) float g_heads[];  // [kWavesPerBlock][H * DS]
    const int wid = threadIdx.x / kWave;
    const int lane = lane_id();
    const int blk = MAXK_P1_XCD ? xcd_contiguous_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int item = blk * kWavesPerBlock + wid;
    if (item >= n_items) return;  // whole wave; no workgroup barrier below
    float *g_lds = g_heads + (size_t)wid * H * DS;
    // the pad columns [D, DS) of every head's row are never staged over: zeroed once
    for (int h = 0; h < H; ++h)
        if (lane < DS - D) g_lds[h * DS + D + lane] = 0.f;

    const ItemRange it = item_range(row_ptr, num_rows, num_e, item, chunk);
    // rows q = r - 1 (continuation), r, r + 1, ...: each one's piece under CutAtEnd, row_ptr of
    // 64 consecutive rows one per lane, as in sspmm_bwd_kernel
    int q = it.r > 0 ? it.r - 1 : 0;
    PtrWindow win{row_ptr, num_rows, 0, 0};
    win.load(q, lane);
    for (; q < num_rows; ++q) {
        win.slide(q, lane);
        const int rb = win.begin(q);
        const int re = win.end(q);
        if (!row_owned(it.d1, q, rb)) break;
        const RowPiece p = any_piece(CutAtEnd{}, it.d0, it.d1, q, rb, re);
        if (p.sb >= p.se) continue;
        const float div = row_div ? row_div[q] : 1.f;
        wave_lds_fence();  // the previous piece's reads of g_lds are done
        for (int h = 0; h < H; ++h) {
            const float *gr = grad + ((int64_t)h * num_rows + q) * D;
            float *gl = g_lds + h * DS;
            if (vec) {
                for (int j = lane * 4; j < D; j += kWave * 4) {
                    float4 v = *reinterpret_cast<const float4 *>(&gr[j]);
                    if (row_div) v = make_float4(v.x / div, v.y / div, v.z / div, v.w / div);
                    *reinterpret_cast<float4 *>(&gl[j]) = v;
                }
            } else {
                for (int j = lane; j < D; j += kWave) gl[j] = row_div ? gr[j] / div : gr[j];
            }
        }
        wave_lds_fence();
        if constexpr (X4)
            push_heads_x4<LG, U, HB>(g_lds, DS, col_idx, edge_val, num_e, H, cbsr_idx, T,
                                     (int)p.sb, (int)p.se, k, lane);
        else
            push_heads_scalar<LG, U, HB>(g_lds, DS, col_idx, edge_val, num_e, H, cbsr_idx, T,
                                         (int)p.sb, (int)p.se, k, lane);
    }
}

// ---- phase 2: grad_cbsr[c, :] = sum over the CSC slots t of c of T[eid[t], :] -------

// Sum the contribution rows T[eid[t]] (k floats each) for t in [tb, te) into
// dst[0:k], in a fixed order.  VEC (k in {4,8,...,256}): LR = k/4 lanes per row
// (16-B loads), 64/LR rows per wave step, U steps in flight; the row groups are
// combined by xor butterflies.  Scalar: KG = pow2ceil(k) lanes per row.
template <bool VEC, int KG, int U, bool NT = false, typename EidAt>
__device__ __forceinline__ void segment_sum(const float *__restrict__ T, EidAt eid, int64_t tb,
                                            int64_t te, int k, float *__restrict__ dst, int lane) {
    if constexpr (VEC) {
        const int LR = k / 4, RI = kWave / LR;
        const int g = lane / LR, q = lane % LR;
        const float4 *__restrict__ T4 = reinterpret_cast<const float4 *>(T);
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int64_t base = tb; base < te; base += (int64_t)RI * U) {
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t t = base + u * RI + g;
                const int e = eid(t < te ? t : tb);
                v[u] = t_load4<NT>(&T4[(size_t)(uint32_t)e * LR + q]);
                if (t >= te) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                a.x += v[u].x;
                a.y += v[u].y;
                a.z += v[u].z;
                a.w += v[u].w;
            }
        }
        for (int off = LR; off < kWave; off <<= 1) {
            a.x += __shfl_xor(a.x, off);
            a.y += __shfl_xor(a.y, off);
            a.z += __shfl_xor(a.z, off);
            a.w += __shfl_xor(a.w, off);
        }
        if (g == 0) reinterpret_cast<float4 *>(dst)[q] = a;
    } else {
        constexpr int G = kWave / KG;
        const int grp = lane / KG;
        for (int l = lane % KG; l - lane % KG < k; l += KG) {  // one pass unless k > 64
            const bool lok = l < k;
            const int lc = lok ? l : k - 1;
            float a = 0.f;
            for (int64_t base = tb; base < te; base += (int64_t)G * U) {
                float v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t t = base + u * G + grp;
                    const int e = eid(t < te ? t : tb);
                    v[u] = T[(size_t)(uint32_t)e * k + lc];
                    if (t >= te) v[u] = 0.f;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) a += v[u];
            }
            for (int off = KG; off < kWave; off <<= 1) a += __shfl_xor(a, off);
            if (grp == 0 && lok) dst[l] = a;
        }
    }
}

// Grouped destinations (low average in-degree, e.g. the halo columns of an N = 8 shard, ~6
// slots each, where segment_sum spends one wave step and a 3-stage butterfly per destination).
// Each lane group of LR = k/4 lanes walks one destination's slots U at a time into its own
// float4 (in slot order: bitwise the same run to run), stores the row the step it ends and takes
// the item's next destination, so 64/LR destinations are in flight per wave; the next step's
// gathers are issued before this step's sums.  Destinations are handed out by
// RowHandout<CutAtEnd> (token_items.h): in order while owned by the item and holding at most
// lmax of its slots; returns the first one not taken (the caller sums a longer one with the
// whole wave).  k % 4 == 0.
template <int U, bool NT = false, typename EidAt>
__device__ __forceinline__ int csc_groups(const float *__restrict__ T, EidAt eid_at,
                                          const int32_t *__restrict__ col_ptr, int c,
                                          int num_cols, int64_t d1, int k, int lmax,
                                          float *__restrict__ grad_cbsr, int lane) {
    const int LR = k / 4, NG = kWave / LR;
    const int g = lane / LR, q = lane % LR;
    const float4 *__restrict__ T4 = reinterpret_cast<const float4 *>(T);
    RowHandout<CutAtEnd> h(col_ptr, num_cols, c, d1, lmax, lane);
    int dst = -1;  // this group's destination and its slot range [t, te)
    int64_t t = 0, te = 0;
    auto assign = [&]() {
        h.assign<1>(dst < 0, NG, LR, g, lane, [&](int col, int cb, int ce) {
            dst = col;
            t = cb;
            te = ce;
        });
    };
    auto gather = [&](float4 (&v)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (dst >= 0 && t + u < te) v[u] = t_load4<NT>(&T4[(size_t)(uint32_t)eid_at(t + u) * LR + q]);
        }
    };
    assign();
    float4 v[U];
    gather(v);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    while (__ballot(dst >= 0)) {
        const int cdst = dst;
        const bool fin = cdst >= 0 && t + U >= te;
        if (fin) dst = -1;
        t += U;
        assign();
        float4 vn[U];
        gather(vn);  // the next step's rows in flight while this step's are summed
#pragma unroll
        for (int u = 0; u < U; ++u) {
            a.x += v[u].x;
            a.y += v[u].y;
            a.z += v[u].z;
            a.w += v[u].w;
            v[u] = vn[u];
        }
        if (fin) {
            reinterpret_cast<float4 *>(grad_cbsr + (int64_t)cdst * k)[q] = a;
            a = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    return h.next;
}

// STAGED (chunk <= kCscStage): the item's CSC slots are one contiguous range of csc_eid,
// starting at d0 - c (the tokens before d0 hold c destination tokens), so the wave copies
// up to `chunk` of them into LDS with coalesced loads before its first segment: every T-row
// gather then waits for one load instead of two dependent ones (a destination of ogbn-products
// averages 50 slots, two U-steps, so each step used to wait for its eid loads first).
constexpr int kCscStage = 2048;
// GROUP (VEC, STAGED): destinations of at most kCscGroupMax slots go through csc_groups.
constexpr int kCscGroupMax = 64;
template <bool VEC, int KG, int U, bool STAGED, bool GROUP = false, bool NT = false>
__global__ __launch_bounds__(kBlock) void csc_sum_kernel(const int32_t *__restrict__ col_ptr,
                                                         const int32_t *__restrict__ eid,
                                                         const float *__restrict__ T,
                                                         float *__restrict__ grad_cbsr,
                                                         float *__restrict__ slab,
                                                         int32_t *__restrict__ slab_row,
                                                         int num_cols, int64_t num_e, int k,
                                                         int chunk, int n_items) {
    extern __shared__ int32_t s_eid[];  // STAGED: [kWavesPerBlock][chunk]
    const int wid = threadIdx.x / kWave;
    const int lane = lane_id();
    const int blk = !MAXK_XCD_SUM      ? (int)blockIdx.x
                    : MAXK_XCD_SUM_RUN ? xcd_window_block(blockIdx.x, gridDim.x, MAXK_XCD_SUM_RUN)
                                       : xcd_contiguous_block(blockIdx.x, gridDim.x);
    const int item = blk * kWavesPerBlock + wid;
    if (item >= n_items) return;
    const ItemRange it = item_range(col_ptr, num_cols, num_e, item, chunk);
    const int64_t d1 = it.d1, p_lo = it.p_lo;  // p_lo: the item's first CSC slot
    int c = it.r;
    int32_t *se_lds = s_eid + (STAGED ? wid * chunk : 0);
    if constexpr (STAGED) {
        const int n_pos = (int)(num_e - p_lo < chunk ? num_e - p_lo : chunk);
        for (int i = lane; i < n_pos; i += kWave) se_lds[i] = eid[p_lo + i];
        wave_lds_fence();
    }
    auto eid_at = [&](int64_t t) -> int {
        if constexpr (STAGED)
            return se_lds[(int)(t - p_lo)];
        else
            return eid[t];
    };
    int cont = -1;
    if (c > 0) {
        const RowPiece p = cont_piece(CutAtEnd{}, it.p_lo, d1, c, col_ptr[c]);
        if (p.sb < p.se) {
            segment_sum<VEC, KG, U, NT>(T, eid_at, p.sb, p.se, k, slab + (int64_t)item * k, lane);
            cont = c - 1;
        }
    }
    if (lane == 0) slab_row[item] = cont;
    for (; c < num_cols; ++c) {
        if constexpr (GROUP) {
            c = csc_groups<U, NT>(T, eid_at, col_ptr, c, num_cols, d1, k, kCscGroupMax, grad_cbsr,
                              lane);
            if (c >= num_cols) break;
        }
        const int64_t cb = col_ptr[c];
        if (!row_owned(d1, c, cb)) break;
        const RowPiece p = row_piece(CutAtEnd{}, d1, c, cb, col_ptr[c + 1]);
        segment_sum<VEC, KG, U, NT>(T, eid_at, p.sb, p.se, k, grad_cbsr + (int64_t)c * k, lane);
    }
}

// Auto item size: ~`per_slot` items per resident wave slot on the device's CUs, in [256, 2048].
int bwd_chunk(int64_t num_rows, int64_t num_e, int32_t chunk, int per_slot) {
    if (chunk > 0) return chunk;
    const int64_t total = num_rows + num_e;
    int64_t c = ceil_div(total, device_cus() * 32 * per_slot);
    c = c < 256 ? 256 : (c > 2048 ? 2048 : c);
    return (int)c;
}

// Loads in flight per lane ("depth" U): one wave step covers `per_step` edges (or
// contribution rows), a batch U steps.  Deep batches keep more bytes in flight on long
// rows; on short rows they are mostly masked lanes.  Largest U in [lo, hi] (powers of
// two) whose batch still fits an average row (measured: products deg 50 -> 4, Reddit /
// proteins deg 500-600 -> 16 for phase 1; 4 / 8 for phase 2).
int pick_depth(int64_t num_e, int64_t rows, int per_step, int lo, int hi) {
    const int64_t avg = rows > 0 ? num_e / rows : 0;
    int u = lo;
    while (u < hi && (int64_t)per_step * u * 2 <= avg) u <<= 1;
    return u;
}

template <int MODE>
int launch_push(hipStream_t s, const int32_t *row_ptr, const int32_t *col_idx,
                const float *edge_val, const float *grad, const float *row_div,
                const uint8_t *cbsr_idx, float *dst, int nr, int64_t num_cols, int64_t num_e,
                int D, int k, int chunk, const uint8_t *esel = nullptr) {
    const int n_items = token_items(nr, num_e, chunk);
    const int64_t blocks = ceil_div(n_items, kWavesPerBlock);
    const dim3 grid((unsigned)(MAXK_P1_XCD ? xcd_grid(blocks) : blocks));
    if (MODE == kStore && ((MAXK_BWD_X4 && k % 4 == 0) || esel)) {
        const int lr = lanes_per_edge(k / 4);
        const int u = MAXK_X4_U > 0 ? MAXK_X4_U : pick_depth(num_e, nr, kWave / lr, 4, 16);
        const bool wide = num_cols >= (1 << 24);  // selector offsets need a 32-bit multiply
        // the selector stream and the table at depth 4, 8 or 16; the wide table at 8 only
        const int mode = esel ? kStoreX4S : wide ? kStoreX4W : kStoreX4;
        const int depth = mode == kStoreX4W ? 8 : u <= 4 ? 4 : u <= 8 ? 8 : 16;
        const bool ok = with_lanes(lr, [&](auto lr_c) {
            with_const<kStoreX4, kStoreX4W, kStoreX4S>(mode, [&](auto mode_c) {
                with_const<4, 8, 16>(depth, [&](auto u_c) {
                    constexpr int LR = decltype(lr_c)::value, M = decltype(mode_c)::value,
                                  U = decltype(u_c)::value;
                    if constexpr (M != kStoreX4W || U == 8)
                        hipLaunchKernelGGL((sspmm_bwd_kernel<LR, U, M>), grid, dim3(kBlock), 0, s,
                                           row_ptr, col_idx, edge_val, grad, row_div, cbsr_idx,
                                           dst, nr, num_e, D, k, chunk, n_items, esel);
                });
            });
        });
        if (!ok) return bad_lanes(lr);
        MAXK_LAUNCHED("sspmm_bwd_kernel");
        return MAXK_OK;
    }
    const int kg = lanes_per_edge(k);
    const bool ok = with_lanes(kg, [&](auto kg_c) {
        constexpr int KG = decltype(kg_c)::value;
        hipLaunchKernelGGL((sspmm_bwd_kernel<KG, (KG >= 8 ? MAXK_BWD_U : 4), MODE>), grid,
                           dim3(kBlock), 0, s, row_ptr, col_idx, edge_val, grad, row_div,
                           cbsr_idx, dst, nr, num_e, D, k, chunk, n_items, nullptr);
    });
    if (!ok) return bad_lanes(kg);
    MAXK_LAUNCHED("sspmm_bwd_kernel");
    return MAXK_OK;
}

// Phase 1 for H heads, at depth kHeadsDepth = 4 on every graph: a lane holds U * HB weights, and
// at depth 8 with HB = 8 the kernel needs 187 VGPRs (two waves per SIMD, against four at depth
// 4) -- Reddit-sized k = 16, the workload whose degree would pick 8 (pick_depth): H = 8 7.04 ms
// at depth 8, 0.192 of the H calls of that run, 5.60 ms and 0.159 at depth 4; H = 4 5.18 and
// 5.25 ms, 0.286 and 0.289 (profiles/r13/heads_bwd/bench_depth_by_degree.json, bench.json).
constexpr int kHeadsDepth = 4;
int launch_push_heads(hipStream_t s, const int32_t *row_ptr, const int32_t *col_idx,
                      const float *edge_val, const float *grad, const float *row_div,
                      const uint8_t *cbsr_idx, float *T, int nr, int64_t num_e, int D, int k,
                      int H, int chunk) {
    const int n_items = token_items(nr, num_e, chunk);
    const int64_t blocks = ceil_div(n_items, kWavesPerBlock);
    const dim3 grid((unsigned)(MAXK_P1_XCD ? xcd_grid(blocks) : blocks));
    const int DS = heads_stride(D);
    const size_t lds = (size_t)kWavesPerBlock * H * DS * sizeof(float);
    const int vec = D % 4 == 0 && ((uintptr_t)grad & 15) == 0;
    const bool x4 = k % 4 == 0;
    const int lg = lanes_per_edge(x4 ? k / 4 : k);
    const bool ok = with_lanes(lg, [&](auto lg_c) {
        with_const<4, 8>(H <= 4 ? 4 : 8, [&](auto hb_c) {
            with_const<0, 1>(x4, [&](auto x4_c) {
                constexpr int LG = decltype(lg_c)::value, HB = decltype(hb_c)::value;
                constexpr bool X4 = decltype(x4_c)::value;
                hipLaunchKernelGGL((sspmm_bwd_heads_kernel<LG, kHeadsDepth, HB, X4>), grid,
                                   dim3(kBlock), lds, s, row_ptr, col_idx, edge_val, grad,
                                   row_div, cbsr_idx, T, nr, num_e, D, DS, k, chunk, n_items, H,
                                   vec);
            });
        });
    });
    if (!ok) return bad_lanes(lg);
    MAXK_LAUNCHED("sspmm_bwd_heads_kernel");
    return MAXK_OK;
}

bool vec_sum(int k) { return k >= 4 && (k & (k - 1)) == 0; }

struct CscLayout {
    int chunk, n_items;
    size_t t_bytes, slab_off, row_off, total;
};

CscLayout csc_layout(int64_t num_cols, int64_t num_e, int k, int chunk) {
    CscLayout L{};
    L.chunk = bwd_chunk(num_cols, num_e, chunk, MAXK_P2_ITEMS);
    L.n_items = token_items(num_cols, num_e, L.chunk);
    L.t_bytes = al256((size_t)(num_e + 1) * k * sizeof(float));  // + dummy row for masked lanes
    L.slab_off = L.t_bytes;
    L.row_off = L.slab_off + al256((size_t)L.n_items * k * sizeof(float));
    L.total = L.row_off + al256((size_t)L.n_items * sizeof(int32_t));
    return L;
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" size_t maxk_sspmm_backward_workspace_size(int64_t num_rows, int64_t num_cols,
                                                     int64_t num_e, int32_t dim_origin,
                                                     int32_t dim_k, int32_t chunk_edges) {
    (void)num_rows; (void)num_cols; (void)num_e; (void)dim_origin; (void)dim_k;
    (void)chunk_edges;
    return 0;
}

extern "C" int maxk_sspmm_backward(const int32_t *row_ptr, const int32_t *col_idx,
                                   const float *edge_val, const float *grad_out,
                                   const float *row_div, const uint8_t *cbsr_idx,
                                   float *grad_cbsr, int64_t num_rows, int64_t num_cols,
                                   int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                   int32_t chunk_edges, void *workspace, size_t workspace_bytes,
                                   void *stream) {
    (void)workspace; (void)workspace_bytes;
    clear_error();
    if (int rc = check_common(num_rows, num_cols, num_e, dim_origin, dim_k, chunk_edges)) return rc;
    hipStream_t s = as_stream(stream);
    if (num_cols > 0) {
        MAXK_REQUIRE(grad_cbsr != nullptr, "grad_cbsr must not be NULL");
        if (int rc = zero_words(grad_cbsr, num_cols * dim_k, s)) return rc;
    }
    if (num_rows == 0 || num_e == 0) return MAXK_OK;
    MAXK_REQUIRE(row_ptr && col_idx && edge_val && grad_out && cbsr_idx,
                 "CSR/grad/selector pointers must not be NULL");
    MAXK_REQUIRE(num_cols > 0, "edges present but num_cols == 0");
    return launch_push<kAtomic>(s, row_ptr, col_idx, edge_val, grad_out, row_div, cbsr_idx,
                                grad_cbsr, (int)num_rows, num_cols, num_e, dim_origin, dim_k,
                                bwd_chunk(num_rows, num_e, chunk_edges, MAXK_P1_ITEMS));
}

extern "C" size_t maxk_sspmm_backward_csc_workspace_size(int64_t num_rows, int64_t num_cols,
                                                         int64_t num_e, int32_t dim_origin,
                                                         int32_t dim_k, int32_t chunk_edges) {
    (void)num_rows; (void)dim_origin;
    if (num_cols < 0 || num_e < 0 || dim_k <= 0) return 0;
    return csc_layout(num_cols, num_e, dim_k, chunk_edges).total;
}

namespace maxk {
namespace {
// Phase 2 and the fix-up over the csc_layout workspace `ws`, whose contribution rows T phase 1
// has written: the launch both the single-head csc backward and the multi-head one end with.
int launch_csc_sum(hipStream_t s, const CscLayout &L, const int32_t *col_ptr,
                   const int32_t *csc_eid, char *ws, float *grad_cbsr, int64_t num_cols,
                   int64_t num_e, int k) {
    const float *T = reinterpret_cast<const float *>(ws);
    float *slab = reinterpret_cast<float *>(ws + L.slab_off);
    int32_t *slab_row = reinterpret_cast<int32_t *>(ws + L.row_off);
    const int64_t blocks = ceil_div(L.n_items, kWavesPerBlock);
    const dim3 grid((unsigned)(MAXK_XCD_SUM ? xcd_grid(blocks) : blocks));
    const int nc = (int)num_cols;
    const bool staged = MAXK_CSC_STAGE && L.chunk <= kCscStage;
    const size_t lds = (size_t)kWavesPerBlock * L.chunk * sizeof(int32_t);
    // T rows of whole 128-B lines: non-temporal reads (t_load4)
    const bool nt = MAXK_T_LOAD_NT && k % 32 == 0;
    // csc_sum_kernel<VEC, KG, U, STAGED, GROUP, NT>, each argument a const_t
    auto sum = [&](auto vec, auto kg, auto u, auto st, auto group, auto ntc) {
        constexpr bool ST = decltype(st)::value;
        hipLaunchKernelGGL((csc_sum_kernel<decltype(vec)::value, decltype(kg)::value,
                                           decltype(u)::value, ST, decltype(group)::value,
                                           decltype(ntc)::value>),
                           grid, dim3(kBlock), ST ? lds : 0, s, col_ptr, csc_eid, T, grad_cbsr,
                           slab, slab_row, nc, num_e, k, L.chunk, L.n_items);
    };
    constexpr const_t<0> no;
    constexpr const_t<1> yes;
    const int kg = lanes_per_edge(k);
    bool ok = true;
    if (staged && vec_sum(k) && k >= 16 && k <= 64 &&
        num_e < (int64_t)MAXK_CSC_GROUP_DEG * num_cols) {
        // few slots per destination: lane groups per destination (csc_groups)
        with_const<0, 1>(nt, [&](auto ntc) {
            sum(yes, const_t<64>{}, const_t<MAXK_CSC_GROUP_U>{}, yes, yes, ntc);
        });
    } else if (vec_sum(k)) {
        const int rows_per_step = kWave / (k / 4);
        const int u = MAXK_SUM_U > 0 ? MAXK_SUM_U
                                     : pick_depth(num_e, num_cols, rows_per_step, 2, 8);
        // staged and non-temporal, staged, or neither
        with_const<2, 4, 8>(u <= 2 ? 2 : u <= 4 ? 4 : 8, [&](auto uc) {
            with_const<0, 1>(staged, [&](auto st) {
                with_const<0, 1>(staged && nt, [&](auto ntc) {
                    if constexpr (decltype(st)::value || !decltype(ntc)::value)
                        sum(yes, const_t<64>{}, uc, st, no, ntc);
                });
            });
        });
    } else {
        ok = with_lanes(kg, [&](auto kgc) {
            with_const<0, 1>(staged, [&](auto st) { sum(no, kgc, const_t<4>{}, st, no, no); });
        });
    }
    if (!ok) return bad_lanes(kg);
    MAXK_LAUNCHED("csc_sum_kernel");
    return launch_slab_fixup<1>(slab, slab_row, grad_cbsr, k, L.n_items, s);
}

// edge_sel (k % 4 == 0): phase 1 reads each edge's selectors from this per-edge stream instead
// of gathering them from cbsr_idx (push_x4, ES).
int csc_impl(const int32_t *row_ptr, const int32_t *col_idx, const float *edge_val,
             const float *grad_out, const float *row_div, const uint8_t *cbsr_idx,
             const uint8_t *edge_sel, const int32_t *col_ptr, const int32_t *csc_eid,
             float *grad_cbsr, int64_t num_rows, int64_t num_cols, int64_t num_e,
             int32_t dim_origin, int32_t dim_k, int32_t chunk_edges, void *workspace,
             size_t workspace_bytes, void *stream) {
    if (int rc = check_common(num_rows, num_cols, num_e, dim_origin, dim_k, chunk_edges)) return rc;
    hipStream_t s = as_stream(stream);
    if (num_cols == 0) return MAXK_OK;
    MAXK_REQUIRE(grad_cbsr && col_ptr, "grad_cbsr/col_ptr must not be NULL");
    MAXK_REQUIRE(num_e == 0 || (row_ptr && col_idx && edge_val && grad_out &&
                                (cbsr_idx || edge_sel) && csc_eid),
                 "CSR/grad/selector/transpose pointers must not be NULL");
    const CscLayout L = csc_layout(num_cols, num_e, dim_k, chunk_edges);
    MAXK_REQUIRE(workspace && workspace_bytes >= L.total,
                 "workspace too small: need %zu bytes, got %zu", L.total, workspace_bytes);
    char *ws = reinterpret_cast<char *>(workspace);
    float *T = reinterpret_cast<float *>(ws);
    const int k = dim_k;
    if (num_e > 0 && num_rows > 0) {
        if (int rc = launch_push<kStore>(s, row_ptr, col_idx, edge_val, grad_out, row_div,
                                         cbsr_idx, T, (int)num_rows, num_cols, num_e,
                                         dim_origin, k,
                                         bwd_chunk(num_rows, num_e, chunk_edges, MAXK_P1_ITEMS),
                                         edge_sel))
            return rc;
    }
    return launch_csc_sum(s, L, col_ptr, csc_eid, ws, grad_cbsr, num_cols, num_e, k);
}

// edge_sel[e * k + l] = cbsr_idx[col_idx[e] * k + l]: wb = 16, 4 or 1 bytes per thread (the
// widest that divides k and both arrays' alignment)
__global__ __launch_bounds__(kBlock) void edge_sel_kernel(const int32_t *__restrict__ col_idx,
                                                          const uint8_t *__restrict__ cbsr_idx,
                                                          uint8_t *__restrict__ edge_sel,
                                                          int64_t n_words, int k, int wb) {
    // grid-stride: the launch caps its grid (num_e * k one-byte words can pass the
    // 2^32 - 1 threads of one grid dimension)
    const int wpe = k / wb;  // words per edge
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_words; i += stride) {
        const int64_t e = i / wpe;
        const int w = (int)(i % wpe);
        const size_t src = (size_t)(uint32_t)col_idx[e] * k + (size_t)w * wb;
        if (wb == 16)
            reinterpret_cast<uint4 *>(edge_sel)[i] =
                *reinterpret_cast<const uint4 *>(cbsr_idx + src);
        else if (wb == 4)
            reinterpret_cast<uint32_t *>(edge_sel)[i] =
                *reinterpret_cast<const uint32_t *>(cbsr_idx + src);
        else
            edge_sel[i] = cbsr_idx[src];
    }
}
}  // namespace

size_t csc_sum_workspace_size(int64_t num_cols, int64_t num_e, int k, int chunk) {
    const CscLayout L = csc_layout(num_cols, num_e, k, chunk);
    if (chunk > 0) return L.total;
    // bwd_chunk's items hold at least 256 tokens, and at least tokens / (its item target) until
    // they reach 2048
    const int64_t tokens = num_cols + num_e, aim = device_cus() * 32 * MAXK_P2_ITEMS;
    const int64_t a = ceil_div(tokens, 256), lo = a < aim ? a : aim, hi = ceil_div(tokens, 2048);
    int64_t cap = lo > hi ? lo : hi;
    if (cap < L.n_items) cap = L.n_items;
    return L.t_bytes + al256((size_t)cap * k * sizeof(float)) +
           al256((size_t)cap * sizeof(int32_t));
}

int csc_sum_rows(hipStream_t s, const int32_t *col_ptr, const int32_t *csc_eid, void *ws,
                 float *grad_cbsr, int64_t num_cols, int64_t num_e, int k, int chunk) {
    return launch_csc_sum(s, csc_layout(num_cols, num_e, k, chunk), col_ptr, csc_eid,
                          reinterpret_cast<char *>(ws), grad_cbsr, num_cols, num_e, k);
}

}  // namespace maxk

extern "C" int maxk_sspmm_backward_csc(const int32_t *row_ptr, const int32_t *col_idx,
                                       const float *edge_val, const float *grad_out,
                                       const float *row_div, const uint8_t *cbsr_idx,
                                       const int32_t *col_ptr, const int32_t *csc_eid,
                                       float *grad_cbsr, int64_t num_rows, int64_t num_cols,
                                       int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                       int32_t chunk_edges, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    clear_error();
    MAXK_REQUIRE(num_e == 0 || cbsr_idx, "cbsr_idx must not be NULL");
    return csc_impl(row_ptr, col_idx, edge_val, grad_out, row_div, cbsr_idx, nullptr, col_ptr,
                    csc_eid, grad_cbsr, num_rows, num_cols, num_e, dim_origin, dim_k, chunk_edges,
                    workspace, workspace_bytes, stream);
}

extern "C" int maxk_sspmm_backward_csc_sel(const int32_t *row_ptr, const int32_t *col_idx,
                                           const float *edge_val, const float *grad_out,
                                           const float *row_div, const uint8_t *edge_sel,
                                           const int32_t *col_ptr, const int32_t *csc_eid,
                                           float *grad_cbsr, int64_t num_rows, int64_t num_cols,
                                           int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                           int32_t chunk_edges, void *workspace,
                                           size_t workspace_bytes, void *stream) {
    clear_error();
    MAXK_REQUIRE(dim_k % 4 == 0, "edge selectors need dim_k %% 4 == 0, got %d", dim_k);
    MAXK_REQUIRE(num_e == 0 || edge_sel, "edge_sel must not be NULL");
    MAXK_REQUIRE(((uintptr_t)edge_sel & 3) == 0, "edge_sel must be 4-B aligned");
    return csc_impl(row_ptr, col_idx, edge_val, grad_out, row_div, nullptr, edge_sel, col_ptr,
                    csc_eid, grad_cbsr, num_rows, num_cols, num_e, dim_origin, dim_k, chunk_edges,
                    workspace, workspace_bytes, stream);
}

extern "C" size_t maxk_sspmm_backward_heads_workspace_size(int64_t num_rows, int64_t num_cols,
                                                           int64_t num_e, int32_t dim_origin,
                                                           int32_t dim_k, int32_t num_heads,
                                                           int32_t chunk_edges) {
    if (num_heads < 1 || num_heads > MAXK_MAX_HEADS) return 0;
    return maxk_sspmm_backward_csc_workspace_size(num_rows, num_cols, num_e, dim_origin, dim_k,
                                                  chunk_edges);
}

extern "C" int maxk_sspmm_backward_heads(const int32_t *row_ptr, const int32_t *col_idx,
                                         const float *edge_val, const float *grad_out,
                                         const float *row_div, const uint8_t *cbsr_idx,
                                         const int32_t *col_ptr, const int32_t *csc_eid,
                                         float *grad_cbsr, int64_t num_rows, int64_t num_cols,
                                         int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                         int32_t num_heads, int32_t chunk_edges, void *workspace,
                                         size_t workspace_bytes, void *stream) {
    clear_error();
    if (int rc = check_common(num_rows, num_cols, num_e, dim_origin, dim_k, chunk_edges)) return rc;
    MAXK_REQUIRE(num_heads >= 1 && num_heads <= MAXK_MAX_HEADS,
                 "num_heads must be in [1,%d], got %d", MAXK_MAX_HEADS, num_heads);
    MAXK_REQUIRE(num_cols < (1 << 24), "num_cols: the multi-head feature backward takes tables "
                 "below 2^24 columns (%lld columns)", (long long)num_cols);
    if (num_cols == 0) return MAXK_OK;
    MAXK_REQUIRE(grad_cbsr && col_ptr, "grad_cbsr/col_ptr must not be NULL");
    MAXK_REQUIRE(num_e == 0 || (row_ptr && col_idx && edge_val && grad_out && cbsr_idx && csc_eid),
                 "CSR/grad/selector/transpose pointers must not be NULL");
    const CscLayout L = csc_layout(num_cols, num_e, dim_k, chunk_edges);
    MAXK_REQUIRE(workspace && workspace_bytes >= L.total,
                 "workspace too small: need %zu bytes, got %zu", L.total, workspace_bytes);
    MAXK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-B aligned");
    MAXK_REQUIRE(((uintptr_t)edge_val & 3) == 0 && ((uintptr_t)grad_out & 3) == 0 &&
                     ((uintptr_t)grad_cbsr & 3) == 0,
                 "float buffers must be 4-B aligned");
    hipStream_t s = as_stream(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    if (num_e > 0 && num_rows > 0) {
        if (int rc = launch_push_heads(s, row_ptr, col_idx, edge_val, grad_out, row_div, cbsr_idx,
                                       reinterpret_cast<float *>(ws), (int)num_rows, num_e,
                                       dim_origin, dim_k, num_heads,
                                       bwd_chunk(num_rows, num_e, chunk_edges, MAXK_P1_ITEMS)))
            return rc;
    }
    return launch_csc_sum(s, L, col_ptr, csc_eid, ws, grad_cbsr, num_cols, num_e, dim_k);
}

// edge_sel_kernel's grid: one thread per word up to 64 workgroups per CU, then grid-stride
extern "C" int64_t maxk_edge_selectors_blocks(int64_t n_words) {
    const int64_t b = ceil_div(n_words < 0 ? 0 : n_words, (int64_t)kBlock);
    const int64_t cap = device_cus() * 64;
    return b < cap ? b : cap;
}

extern "C" int maxk_edge_selectors(const int32_t *col_idx, const uint8_t *cbsr_idx,
                                   int64_t num_e, int32_t dim_k, uint8_t *edge_sel, void *stream) {
    clear_error();
    MAXK_REQUIRE(dim_k >= 1 && dim_k <= kMaxDim, "dim_k must be in [1,256], got %d", dim_k);
    MAXK_REQUIRE(num_e >= 0 && num_e * (int64_t)dim_k < (1LL << 40), "num_e out of range");
    if (num_e == 0) return MAXK_OK;
    MAXK_REQUIRE(col_idx && cbsr_idx && edge_sel, "pointers must not be NULL");
    // any k and alignment: the widest word that divides k and both arrays' alignment (the
    // _sel entry points accept 4-B aligned streams, and this is their fallback past 2^24 columns)
    const uintptr_t al = (uintptr_t)edge_sel | (uintptr_t)cbsr_idx;
    const int wb = dim_k % 16 == 0 && (al & 15) == 0 ? 16 : dim_k % 4 == 0 && (al & 3) == 0 ? 4 : 1;
    const int64_t n_words = num_e * (dim_k / wb);
    hipLaunchKernelGGL(edge_sel_kernel, dim3((unsigned)maxk_edge_selectors_blocks(n_words)), dim3(kBlock), 0,
                       as_stream(stream), col_idx, cbsr_idx, edge_sel, n_words, dim_k, wb);
    MAXK_LAUNCHED("edge_sel_kernel");
    return MAXK_OK;
}
