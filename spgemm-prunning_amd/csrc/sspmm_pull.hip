// Backward SSpMM, the pull (maxk_sspmm_backward_pull / _pull_tiles; the forms and their
// formula: sspmm_bwd.h): per tile (row slice, destination bucket) the edges' values are
// gathered straight from G / row_div into an fp64 LDS accumulator, with no per-edge
// contribution rows.
#include <algorithm>

#include "sspmm_bwd.h"

namespace maxk {
namespace {

// ---- pull: the backward without contribution rows -------------------------------------
// grad_cbsr[c, :] = sum over the edges (r -> c) of w * G'[r, sel[c, :]], G' = G / row_div.
// The pull plan (maxk_pull_plan) sorts the edges into tiles: tile t = (row slice s,
// destination bucket j), t = s * n_buckets + j, CSR order inside a tile, each entry
// carrying its source row, weight and column within the bucket.  Workgroup t sums tile t
// into an fp64 LDS accumulator [2^shift, k + 1] (as bucket_sum_kernel, ds_add_f64) and
// stores it, fp32, to tile_out[t]; pull_reduce_kernel adds a bucket's slices in slice
// order.  The k values of an entry are gathered straight from G': workgroups start in tile
// order, so the ones in flight read one slice of G' rows (~3.5 MB, the size of an XCD's
// L2), and a source row's entries in a tile (~2 at Reddit scale) are neighbours in one
// wave instruction.  This replaces the 7.4 GB write + ~10 GB read of T by ~1.2 GB of
// entries and 2 x slices x 15 MB of tile partials (Reddit k=16).
__global__ __launch_bounds__(kBlock) void gprime_kernel(const float *__restrict__ G,
                                                        const float *__restrict__ row_div,
                                                        float *__restrict__ Gp, int64_t n4,
                                                        int D4) {
    const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (i >= n4) return;
    const float dv = row_div[i / D4];
    float4 v = reinterpret_cast<const float4 *>(G)[i];
    v.x /= dv;
    v.y /= dv;
    v.z /= dv;
    v.w /= dv;
    reinterpret_cast<float4 *>(Gp)[i] = v;
}

// LR = pow2ceil(k/4) lanes per entry, lane q owning l = 4q..4q+3: per entry one 8-B entry
// load, one u32 selector read (from LDS when the bucket's selector rows fit next to the
// accumulator, SEL_LDS), four gathers and four LDS adds; 64/LR entries per wave
// instruction, U instructions per wave step, the next step's entries prefetched.
// Entry = {row within the slice | column within the bucket << 16, weight bits}.
template <int LR, int U, bool SEL_LDS, int VPL>
__global__ __launch_bounds__(1024) void pull_tile_kernel(
    const float *__restrict__ Gp, const uint8_t *__restrict__ cbsr_idx,
    const int32_t *__restrict__ tile_ptr, const uint2 *__restrict__ ent,
    float *__restrict__ tile_out, int64_t num_cols, int n_buckets, int rows_per_slice, int D,
    int k, int shift) {
    extern __shared__ double acc[];  // [(k + 1) << shift], then (SEL_LDS) [k << shift] bytes
    constexpr int EPI = kWave / LR;
    constexpr int STEP = EPI * U;
    const int tid = threadIdx.x;
    const int lane = lane_id(), w = tid / kWave;
    const int g = lane / LR, q = lane % LR;
    const bool qok = q < k / VPL;
    const int ks = k + 1;
    const int t = blockIdx.x;
    const int j = t % n_buckets;
    const float *__restrict__ Gs = Gp + (size_t)(t / n_buckets) * rows_per_slice * D;
    const int s0 = tile_ptr[t], s1 = tile_ptr[t + 1];
    const int64_t c0 = (int64_t)j << shift;
    const uint8_t *__restrict__ selg = cbsr_idx + c0 * k;
    uint8_t *sel_lds = reinterpret_cast<uint8_t *>(acc + (ks << shift));
    for (int i = tid; i < (ks << shift); i += 1024) acc[i] = 0.0;
    if (SEL_LDS) {
        const int rows = num_cols - c0 < (1 << shift) ? (int)(num_cols - c0) : (1 << shift);
        const int nb = rows * k;  // c0 * k is a multiple of 16 (shift >= 4), as is sel_lds
        for (int i = tid; i < nb / 16; i += 1024)
            reinterpret_cast<uint4 *>(sel_lds)[i] = reinterpret_cast<const uint4 *>(selg)[i];
        for (int i = (nb & ~15) + tid; i < nb; i += 1024) sel_lds[i] = selg[i];
    }
    __syncthreads();
    int base = s0 + w * STEP;
    uint2 en[U];
    // kShfl: 8-B loads with one entry per lane fetch the step's STEP entries (NL = STEP / 64
    // loads); each lane group then takes its entry from the loading lane with ds_bpermute:
    // NL memory instructions per step for the entries instead of U (the texture addresser,
    // not LDS, is the busy unit; Reddit k=8 / 16 / 32: -3.5 / -5.8 / -5.3 %).  With more than
    // 8 lanes per entry the two shuffles per instruction outweigh the loads saved (k=64 +4 %).
    constexpr bool kShfl = MAXK_PULL_SHFL && LR <= 8;
    constexpr int NL = (STEP + kWave - 1) / kWave;
    uint2 my[NL];
    auto load_ids = [&](int b) {
        if constexpr (kShfl) {
#pragma unroll
            for (int m = 0; m < NL; ++m) {
                const int e = b + m * kWave + lane;
                my[m] = ent[e < s1 ? e : s1 - 1];
                if (e >= s1 || m * kWave + lane >= STEP) my[m].x = 0xffff0000u;  // no entry
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = b + u * EPI + g;
                en[u] = ent[e < s1 ? e : s1 - 1];
                if (e >= s1) en[u].x = 0xffff0000u;  // no entry: row 0 (a valid gather), column 0xffff
            }
        }
    };
    if (base < s1) load_ids(base);
    for (; base < s1; base += 16 * STEP) {
        if constexpr (kShfl) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int m = (u * EPI) / kWave;  // compile-time after unrolling
                const int src = (u * EPI + g - m * kWave) * 4;
                en[u].x = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)my[m].x);
                en[u].y = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)my[m].y);
            }
        }
        uint32_t sv[U];
        int dc[U];
        float wc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t key = en[u].x;
            dc[u] = (key >> 16) == 0xffffu ? -1 : (int)(key >> 16);
            // VPL (4 or 1) consecutive selectors of the entry's destination, lane q's share
            const int bo = (dc[u] < 0 ? 0 : dc[u]) * k + (qok ? q : 0) * VPL;
            const uint8_t *sb8 = SEL_LDS ? sel_lds : selg;
            sv[u] = VPL == 4 ? *reinterpret_cast<const uint32_t *>(sb8 + bo) : (uint32_t)sb8[bo];
        }
        float v[U][VPL];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float *gr = Gs + (en[u].x & 0xffffu) * (uint32_t)D;
#pragma unroll
            for (int i = 0; i < VPL; ++i) {  // a selector >= D (D < 256) contributes 0
                const uint32_t c = (sv[u] >> (8 * i)) & 255u;
                const bool in = c < (uint32_t)D;
                const float x = gr[in ? c : 0u];
                v[u][i] = in ? x : 0.0f;
            }
            wc[u] = __uint_as_float(en[u].y);
        }
        if (base + 16 * STEP < s1) load_ids(base + 16 * STEP);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (dc[u] >= 0 && qok) {
                double *a = &acc[dc[u] * ks + VPL * q];
#pragma unroll
                for (int i = 0; i < VPL; ++i) atomicAdd(a + i, (double)(wc[u] * v[u][i]));
            }
        }
    }
    __syncthreads();
    float *o = tile_out + (size_t)t * ((size_t)k << shift);
    if (MAXK_PULL_F4_FLUSH && k % 4 == 0) {  // 16-B stores: 4x fewer store instructions
        for (int i4 = tid; i4 < (k << shift) / 4; i4 += 1024) {
            const double *a = &acc[i4 * 4 + (i4 * 4) / k];  // 4 l of one row (k % 4 == 0)
            reinterpret_cast<float4 *>(o)[i4] =
                make_float4((float)a[0], (float)a[1], (float)a[2], (float)a[3]);
        }
    } else {
        for (int i = tid; i < (k << shift); i += 1024) o[i] = (float)acc[i + i / k];
    }
}

// ---- pull, quantile-slot form (k % 4 == 0) ----------------------------------------------
// The gathers of pull_tile_kernel are bound by the cache lines one wave instruction touches
// (the texture addresser and L1 take a line per cycle, not a lane): an instruction carries
// 64 / LR entries x LR lanes, each lane one value of its entry's source row, so the ~2
// entries of one row in an instruction land on ~6 of the row's eight 128-B lines, four
// instructions per step.  pull_sel_kernel therefore re-orders every destination's k
// selectors once per call: sorted ascending, and laid out so that a lane's four bytes
// (instructions i = 0..3) hold sorted positions i * k/4 + q.  Instruction i then gathers
// only the i-th quarter of every row's selected columns, ~2 lines of a row instead of ~6 (a
// model of the tile stream: 9.2 -> 5.2 distinct lines per entry at Reddit's ~2.2 entries per
// row and tile).  lmap keeps each slot's original l; pull_reduce_kernel writes the sums back
// in CBSR order.  Slot of sorted position p: lane q = p % (k/4), instruction i = p / (k/4)
// -> slot 4q + i.  Equal selectors (never produced by top-k) rank by l, so the map is a
// permutation of the k slots whatever the input.
__global__ __launch_bounds__(kBlock) void pull_sel_kernel(const uint8_t *__restrict__ sel,
                                                          uint8_t *__restrict__ sel_q,
                                                          uint8_t *__restrict__ lmap,
                                                          int64_t num_cols, int k, int kp,
                                                          int vpl) {
    __shared__ uint32_t bm[kBlock / 4 * 8];  // 256-bit column set per destination
    __shared__ uint8_t s_out[kBlock], l_out[kBlock];
    const int nd = kBlock / k;  // destinations per block (k % 4 == 0, k <= 256)
    const int tid = threadIdx.x;
    const int d = tid / k, l = tid % k;
    const int64_t c0 = (int64_t)blockIdx.x * nd;
    const int64_t c = c0 + d;
    const bool act = d < nd && c < num_cols;
    for (int i = tid; i < nd * 8; i += kBlock) bm[i] = 0u;
    __syncthreads();
    const uint32_t s = act ? sel[c * k + l] : 0u;
    if (act) atomicOr(&bm[d * 8 + (s >> 5)], 1u << (s & 31));
    __syncthreads();
    if (act) {
        int distinct = 0, rank = 0;
        for (int wd = 0; wd < 8; ++wd) {
            const uint32_t b = bm[d * 8 + wd];
            distinct += __popc(b);
            if (wd < (int)(s >> 5)) rank += __popc(b);
        }
        rank += __popc(bm[d * 8 + (s >> 5)] & ((1u << (s & 31)) - 1u));
        if (distinct < k) {  // repeated selectors: rank by (selector, l)
            rank = 0;
            for (int m = 0; m < k; ++m) {
                const uint32_t sm = sel[c * k + m];
                rank += (sm < s) || (sm == s && m < l);
            }
        }
        // part h = rank / kp (pull_q_kernel's parts), then the quantile slot inside it
        // lane q of a part holds sorted positions i * (kp / vpl) + q, i < vpl, in slots
        // vpl * q + i
        const int ql = kp / vpl, h = rank / kp, r = rank % kp;
        const int slot = h * kp + vpl * (r % ql) + r / ql;
        s_out[d * k + slot] = (uint8_t)s;
        l_out[d * k + slot] = (uint8_t)l;
    }
    __syncthreads();
    const int64_t nb = (num_cols - c0 < nd ? num_cols - c0 : nd) * (int64_t)k;
    if (tid < nb) {
        sel_q[c0 * k + tid] = s_out[tid];
        lmap[c0 * k + tid] = l_out[tid];
    }
}

// pull_sel_kernel with four selectors per thread (k % 4 == 0, 4-byte aligned selectors): one
// u32 load and store per thread instead of a byte each, and a destination's 256-bit column
// set read once per four ranks (ogbn-products-sized, k=32: 2.45M destinations).
__global__ __launch_bounds__(kBlock) void pull_sel4_kernel(const uint8_t *__restrict__ sel,
                                                           uint8_t *__restrict__ sel_q,
                                                           uint8_t *__restrict__ lmap,
                                                           int64_t num_cols, int k, int kp,
                                                           int vpl) {
    __shared__ uint32_t bm[kBlock * 8];  // 256-bit column set per destination (k >= 4)
    __shared__ uint32_t s_out[kBlock], l_out[kBlock];
    const int tpd = k / 4;      // threads per destination
    const int nd = kBlock / tpd;  // destinations per block
    const int tid = threadIdx.x;
    const int d = tid / tpd, l0 = (tid % tpd) * 4;
    const int64_t c0 = (int64_t)blockIdx.x * nd;
    const int64_t c = c0 + d;
    const bool act = d < nd && c < num_cols;
    for (int i = tid; i < nd * 8; i += kBlock) bm[i] = 0u;
    __syncthreads();
    const uint32_t w4 = act ? *reinterpret_cast<const uint32_t *>(sel + c * k + l0) : 0u;
    if (act) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t sj = (w4 >> (8 * j)) & 255u;
            atomicOr(&bm[d * 8 + (sj >> 5)], 1u << (sj & 31));
        }
    }
    __syncthreads();
    if (act) {
        uint32_t wds[8];
        int distinct = 0;
#pragma unroll
        for (int wd = 0; wd < 8; ++wd) {
            wds[wd] = bm[d * 8 + wd];
            distinct += __popc(wds[wd]);
        }
        uint8_t *so = reinterpret_cast<uint8_t *>(s_out), *lo = reinterpret_cast<uint8_t *>(l_out);
        const int ql = kp / vpl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t sj = (w4 >> (8 * j)) & 255u;
            const int l = l0 + j;
            int rank = 0;
            if (distinct == k) {
                const int hi = (int)(sj >> 5);
#pragma unroll
                for (int wd = 0; wd < 8; ++wd) {
                    rank += wd < hi ? __popc(wds[wd]) : 0;
                    rank += wd == hi ? __popc(wds[wd] & ((1u << (sj & 31)) - 1u)) : 0;
                }
            } else {  // repeated selectors: rank by (selector, l)
                for (int m = 0; m < k; ++m) {
                    const uint32_t sm = sel[c * k + m];
                    rank += (sm < sj) || (sm == sj && m < l);
                }
            }
            const int h = rank / kp, r = rank % kp;
            const int slot = h * kp + vpl * (r % ql) + r / ql;
            so[d * k + slot] = (uint8_t)sj;
            lo[d * k + slot] = (uint8_t)l;
        }
    }
    __syncthreads();
    const int64_t nbytes = (num_cols - c0 < nd ? num_cols - c0 : nd) * (int64_t)k;
    if ((int64_t)tid * 4 < nbytes) {
        reinterpret_cast<uint32_t *>(sel_q + c0 * k)[tid] = s_out[tid];
        reinterpret_cast<uint32_t *>(lmap + c0 * k)[tid] = l_out[tid];
    }
}

// One tile's entry loop of pull_q_kernel: adds the tile's n_e entries (ers)
// into the fp64 accumulator, gathering from the slice's G' rows (grs).
// GROW (the stream form): an entry's key is {global row << shift | column in the bucket} and
// grs covers all of G', so one loop walks a bucket's entries of every slice.
template <int LR, int U, bool FULLD, int VPL, bool GROW = false>
__device__ __forceinline__ void pull_q_entries(double *acc, const uint8_t *sel_lds,
                                               __amdgpu_buffer_rsrc_t grs,
                                               __amdgpu_buffer_rsrc_t ers, int n_e, int D,
                                               int kp, int shift) {
    constexpr int EPI = kWave / LR;                 // entries per wave instruction
    constexpr int STEP = EPI * U;                   // entries per wave step
    constexpr int NL = (STEP + kWave - 1) / kWave;  // entry loads per step (one per lane)
    const int tid = threadIdx.x;
    const int lane = lane_id(), w = tid / kWave;
    // Lane -> (entry g, lane-in-entry q).  The texture path serves a 16-lane quarter in four
    // lane columns {c, c+4, c+8, c+12}, and lanes of one cache line that sit in one quad
    // cost extra cycles (tools/ta_probe.hip, L1-resident: 4 lines per quarter cost 4.2
    // cycles spread one lane per quad, 8.7 with a quad per line).  In one instruction the
    // LR lanes of an entry gather LR consecutive sorted columns, often one line, so they
    // are spread over the quads and gathered into columns: a column holds four consecutive
    // lanes-in-entry of one entry (LR >= 4) or all LR lanes of 4/LR neighbouring entries
    // (LR < 4; neighbours in CSR order share a source row most often).
    constexpr int EPQ = LR < 16 ? 16 / LR : 1;  // entries per 16-lane quarter
    const int lc = (lane % 16) % 4, lm = (lane % 16) / 4;  // column, lane's place in it
    constexpr bool TR = MAXK_PULL_TRANSPOSE && LR <= 16;  // an entry within a quarter
    const int g = !TR ? lane / LR
                  : LR >= 4 ? (lane / 16) * EPQ + lc / (LR / 4 > 0 ? LR / 4 : 1)
                            : (lane / 16) * EPQ + lc * (4 / LR) + lm / LR;
    const int q = !TR ? lane % LR
                  : LR >= 4 ? (lc % (LR / 4 > 0 ? LR / 4 : 1)) * 4 + lm
                            : lm % LR;
    const bool qok = q < kp / VPL;
    const int ks = pull_ks(kp, shift);
    const uint32_t Db = (uint32_t)D * 4u;
    const int stride = 16 * STEP;  // 16 waves
    const int base = w * STEP;     // entry offsets relative to the tile's first entry
    // Every step is issued the same way: no load sits under a branch, since the compiler
    // merges the counters of the two sides of a branch conservatively and then waits for
    // loads it could leave in flight.  Entries past the tile read 0 (past the descriptor),
    // their gathers get offsets past the G' descriptor (0, no memory access), their weight
    // 0, and their adds (+0.0) go to a lane-private row of the accumulator.  The loop runs
    // an even number of steps; the last issue is never consumed.
    const int nsteps = base < n_e ? (n_e - base + stride - 1) / stride : 0;
    const int idle = (w * kWave + lane) & ((1 << shift) - 1);

    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    u32x2 myA[NL], myB[NL];
    float vA[U][VPL], vB[U][VPL];
    int dA[U], dB[U];
    float wA[U], wB[U];
    auto load_ent = [&](u32x2(&my)[NL], int n) {
#pragma unroll
        for (int m = 0; m < NL; ++m)
            my[m] = __builtin_amdgcn_raw_buffer_load_b64(
                ers, (int)((uint32_t)(base + n * stride + m * kWave + lane) * 8u), 0, 0);
    };
    // step n: entries from my (then reloaded for step n + 2), selectors, gathers into v
    auto issue = [&](u32x2(&my)[NL], float(&v)[U][VPL], int(&dc)[U], float(&wc)[U], int n) {
        uint32_t ex[U], ey[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = (u * EPI) / kWave;  // compile-time after unrolling
            const int src = (u * EPI + g - m * kWave) * 4;
            ex[u] = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)my[m][0]);
            ey[u] = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)my[m][1]);
        }
        load_ent(my, n + 2);
        uint64_t sv[U];
        bool ok[U];
        const int eb = base + n * stride + g;  // this lane group's entry of instruction 0
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ok[u] = eb + u * EPI < n_e && qok;
            const int d = !ok[u] ? idle
                          : GROW ? (int)(ex[u] & ((1u << shift) - 1u))
                                 : (int)(ex[u] >> 16);
            dc[u] = d * ks + VPL * q * ok[u];
            const uint8_t *sp = sel_lds + d * kp + (ok[u] ? q * VPL : 0);
            if constexpr (VPL == 8)
                sv[u] = *reinterpret_cast<const uint64_t *>(sp);
            else if constexpr (VPL == 4)
                sv[u] = *reinterpret_cast<const uint32_t *>(sp);
            else
                sv[u] = *reinterpret_cast<const uint16_t *>(sp);
            wc[u] = ok[u] ? __uint_as_float(ey[u]) : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t ro =
                ok[u] ? (GROW ? ex[u] >> shift : ex[u] & 0xffffu) * Db : 0x80000000u;
#pragma unroll
            for (int i = 0; i < VPL; ++i) {
                const uint32_t c = VPL == 8 ? (uint32_t)(sv[u] >> (8 * i)) & 255u
                                            : ((uint32_t)sv[u] >> (8 * i)) & 255u;
                uint32_t off = ro + c * 4u;
                if (!FULLD) off = c < (uint32_t)D ? off : 0x80000000u;  // past the buffer: 0
                v[u][i] = __builtin_bit_cast(
                    float, __builtin_amdgcn_raw_buffer_load_b32(grs, (int)off, 0, 0));
            }
        }
    };
    auto consume = [&](float(&v)[U][VPL], int(&dc)[U], float(&wc)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double *a = &acc[dc[u]];
#pragma unroll
            for (int i = 0; i < VPL; ++i) atomicAdd(a + i, (double)(wc[u] * v[u][i]));
        }
    };
    if (nsteps > 0) {
        load_ent(myA, 0);
        load_ent(myB, 1);
        // keep step 1's entries ahead of step 0's gathers: the loop head waits for them with
        // step 0's gathers still in flight only if they were issued first
        __builtin_amdgcn_sched_barrier(0);
        issue(myA, vA, dA, wA, 0);
        // sched_barrier: the machine scheduler would otherwise hoist a consume's multiplies
        // and the next issue's shuffles above the gathers, waiting for loads meant to stay in
        // flight
        for (int n = 0; n < nsteps; n += 2) {
            issue(myB, vB, dB, wB, n + 1);
            __builtin_amdgcn_sched_barrier(0);
            consume(vA, dA, wA);
            __builtin_amdgcn_sched_barrier(0);
            issue(myA, vA, dA, wA, n + 2);
            __builtin_amdgcn_sched_barrier(0);
            consume(vB, dB, wB);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// Where tile t's pieces live: its slice's first row and row count, its bucket's first column.
struct PullTile {
    int64_t r0, nrows, c0;
    int s0, s1;
};
// Tile t = slice * n_buckets + bucket; its entries are [tile_ptr[i], tile_ptr[i + 1]), i = t
// for a full plan, i = t's position in the tile list for a listed one (pull_q_kernel).
__device__ __forceinline__ PullTile pull_tile_of(int t, int i, const int32_t *__restrict__ tile_ptr,
                                                 int n_buckets, int rows_per_slice,
                                                 int64_t num_rows, int shift) {
    PullTile p;
    p.r0 = (int64_t)(t / n_buckets) * rows_per_slice;
    p.nrows = num_rows - p.r0 < rows_per_slice ? num_rows - p.r0 : rows_per_slice;
    p.c0 = (int64_t)(t % n_buckets) << shift;
    p.s0 = tile_ptr[i];
    p.s1 = tile_ptr[i + 1];
    return p;
}

// Part h of each destination's slot-ordered selectors (kp bytes of its k-byte row) for the
// bucket starting at column c0, loaded to registers (up to kSelRegs 16-B pieces per
// thread) and then stored to LDS.
constexpr int kSelRegs = 2;
struct PullSel {
    uint4 v[kSelRegs];
};
// ... of the `rows` destinations from column c0 on (the pieces past them hold zeros)
__device__ __forceinline__ PullSel pull_sel_load_rows(const uint8_t *__restrict__ sel_q,
                                                      int64_t c0, int rows, int k, int kp, int h) {
    PullSel r;
    const int tid = threadIdx.x;
    const uint8_t *__restrict__ selg = sel_q + c0 * k + h * kp;
    // piece i: destination i / ppr, bytes [16 * (i % ppr), +16) of its kp (ppr = kp / 16), or
    // for kp < 16 whole 16-B groups of 16 / kp destinations packed from their kp-byte parts
#pragma unroll
    for (int m = 0; m < kSelRegs; ++m) {
        const int i = tid + m * 1024;
        uint4 x = make_uint4(0u, 0u, 0u, 0u);
        if (kp % 16 == 0) {
            const int ppr = kp / 16;
            if (i < rows * ppr)
                x = *reinterpret_cast<const uint4 *>(selg + (int64_t)(i / ppr) * k + (i % ppr) * 16);
        } else {  // kp % 16 != 0 (kp % 4 == 0): 4-byte words, 4 per piece
            uint32_t wd[4];
            const int wpr = kp / 4;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int wi = i * 4 + b;
                wd[b] = wi < rows * wpr
                            ? *reinterpret_cast<const uint32_t *>(selg + (int64_t)(wi / wpr) * k +
                                                                  (wi % wpr) * 4)
                            : 0u;
            }
            x = make_uint4(wd[0], wd[1], wd[2], wd[3]);
        }
        r.v[m] = x;
    }
    return r;
}
__device__ __forceinline__ PullSel pull_sel_load(const uint8_t *__restrict__ sel_q, int64_t c0,
                                                 int64_t num_cols, int k, int kp, int h,
                                                 int shift) {
    const int rows = num_cols - c0 < (1 << shift) ? (int)(num_cols - c0) : (1 << shift);
    return pull_sel_load_rows(sel_q, c0, rows, k, kp, h);
}
__device__ __forceinline__ void pull_sel_store(uint8_t *sel_lds, const PullSel &r, int kp,
                                               int shift) {
    const int n16 = (kp << shift) / 16;
#pragma unroll
    for (int m = 0; m < kSelRegs; ++m) {
        const int i = threadIdx.x + m * 1024;
        if (i < n16) reinterpret_cast<uint4 *>(sel_lds)[i] = r.v[m];
    }
}

// tile_out[t] is [2^shift, k] in slot order; part h fills slots [h * kp, (h + 1) * kp).
__device__ __forceinline__ void pull_flush(const double *acc, float *__restrict__ tile_out, int t,
                                           int h, int k, int kp, int shift) {
    const int ks = pull_ks(kp, shift);
    float *o = tile_out + (size_t)t * ((size_t)k << shift) + h * kp;
    const int w4 = kp / 4;
    for (int i4 = threadIdx.x; i4 < (kp << shift) / 4; i4 += 1024) {
        const int c = i4 / w4, s4 = i4 % w4;
        const double *a = &acc[c * ks + 4 * s4];
        *reinterpret_cast<float4 *>(o + (size_t)c * k + 4 * s4) =
            make_float4((float)a[0], (float)a[1], (float)a[2], (float)a[3]);
    }
}

// Parts: with H = k / kp parts, destination c's slots split by sorted position into H
// groups of kp (part h: the h-th kp smallest selectors), and one workgroup sums one part of
// one tile: the accumulator holds kp slots per destination, so a bucket holds H times the
// destinations and a source row meets ~H times fewer buckets; each part's gathers cover
// only its share of a row's columns (the h-th kp order statistics of every entry).  The
// tile's entries are read H times (kp: maxk_pull_shift, transpose.hip).
// One 1024-thread workgroup per (tile, part), as pull_tile_kernel (fp64 LDS accumulator of
// the bucket, its slot-ordered selector rows copied next to it), with:
//  * quantile slots (pull_sel_kernel): lane q's u32 selector word holds its four
//    instructions' columns;
//  * a two-step software pipeline: step n's gathers are issued before step n-1's adds, and
//    the entries two steps ahead, so a wave keeps 2 x 4U gathers in flight and never waits
//    on loads it has just issued (the one-step loop waited for every load at its head);
//  * the G' gathers through a wave-uniform buffer descriptor over the slice's rows with
//    32-bit offsets (no 64-bit address math per value); a selector >= D (possible only
//    when D < 256, !FULLD) gets an offset past the descriptor, and the hardware returns 0;
//  * tiles in XCD order (MAXK_PULL_XCD): XCD x runs the x-th eighth of the tile sequence
//    in order, so each XCD's L2 holds the one slice it works on instead of every XCD
//    pulling every slice.
template <int LR, int U, bool FULLD, int VPL>
__global__ __launch_bounds__(1024) void pull_q_kernel(
    const float *__restrict__ Gp, const uint8_t *__restrict__ sel_q,
    const int32_t *__restrict__ tile_ptr, const uint2 *__restrict__ ent,
    float *__restrict__ tile_out, int64_t num_cols, int n_buckets, int n_tiles,
    int rows_per_slice, int64_t num_rows, int D, int k, int kp, int shift,
    const int32_t *__restrict__ tile_list) {
    // tile_list (maxk_sspmm_backward_pull_tiles): only the listed tiles run; tile_ptr then
    // holds their entry ranges and tile_out their partials, both by list position
    extern __shared__ double acc[];  // [ks << shift], then [kp << shift] selector bytes
    const int tid = threadIdx.x;
    const int ks = pull_ks(kp, shift);
    const int H = k / kp;
    const int tp = MAXK_PULL_XCD ? xcd_contiguous_block(blockIdx.x, gridDim.x) : blockIdx.x;
    if (tp >= n_tiles * H) return;  // the XCD grid's padding
    const int ti = tp / H, h = tp % H;
    const int t = tile_list ? tile_list[ti] : ti;
    const PullTile p = pull_tile_of(t, ti, tile_ptr, n_buckets, rows_per_slice, num_rows, shift);
    uint8_t *sel_lds = reinterpret_cast<uint8_t *>(acc + (ks << shift));
    for (int i = tid; i < (ks << shift); i += 1024) acc[i] = 0.0;
    pull_sel_store(sel_lds, pull_sel_load(sel_q, p.c0, num_cols, k, kp, h, shift), kp, shift);
    __syncthreads();
    const auto grs =
        wave_buffer(Gp + p.r0 * D, (uint32_t)(p.nrows > 0 ? p.nrows : 0) * (uint32_t)D * 4u);
    const auto ers = wave_buffer(ent + p.s0, (uint32_t)(p.s1 - p.s0) * 8u);
    pull_q_entries<LR, U, FULLD, VPL>(acc, sel_lds, grs, ers, p.s1 - p.s0, D, kp, shift);
    __syncthreads();
    pull_flush(acc, tile_out, ti, h, k, kp, shift);
}

// The stream form (maxk_sspmm_backward_pull_stream): one workgroup per (bucket, part) for the
// whole call.  The stream plan's buckets [bucket_col[b], bucket_col[b + 1]) hold about equal
// entry counts, as many buckets as fill whole rounds of one workgroup per CU; a bucket's
// entries ent[grp_ptr[b] .. grp_ptr[b + 1]) are in CSR order and carry their global source
// row, so the workgroup walks them front to back through one descriptor over G'.  The
// workgroups of a round start together with equal work and so sweep the rows of G' side by
// side, which is what lets an XCD's L2 serve a row to all of them; no workgroup waits for
// another.  Inside a workgroup the 16 waves share no data and nothing keeps them together
// (without the barrier below they drift tens of thousands of rows apart and the L2 hit rate
// falls to 43 %), so the walk goes in runs of MAXK_PULL_STREAM_RUN entries with a
// workgroup barrier after each.  The fp64 sums never leave LDS: there are no tile partials and
// no reduce, the workgroup stores its rows of grad_cbsr itself (slot f of part h to l =
// lmap[c * k + h * kp + f]).  XCD x runs part x % H of its buckets, so the workgroups that
// share an L2 gather the same share of every row's columns.
#ifndef MAXK_PULL_STREAM_RUN  // entries between two workgroup barriers (Reddit k = 16: 4096 /
#define MAXK_PULL_STREAM_RUN 16384  // 16384 / 65536 / 262144 / none = 1.93 / 1.81 / 1.84 / 2.22 / 2.84 ms)
#endif
template <int LR, int U, bool FULLD, int VPL, int STREAM>
__global__ __launch_bounds__(1024) void pull_q_kernel(
    const float *__restrict__ Gp, const uint8_t *__restrict__ sel_q,
    const uint8_t *__restrict__ lmap, const int32_t *__restrict__ bucket_col,
    const int32_t *__restrict__ grp_ptr, const uint2 *__restrict__ ent,
    float *__restrict__ grad_cbsr, int64_t num_cols, int n_buckets, int64_t num_rows, int D,
    int k, int kp, int shift) {
    static_assert(STREAM == 1, "the stream form");
    extern __shared__ double acc[];  // [ks << shift], then [kp << shift] selector bytes
    const int tid = threadIdx.x;
    const int ks = pull_ks(kp, shift);
    const int H = k / kp;
    int b, h;
    if (kXcds % H == 0) {
        const int x = blockIdx.x % kXcds, per = gridDim.x / kXcds;
        h = x % H;
        b = (x / H) * per + blockIdx.x / kXcds;
        if (b >= n_buckets) return;  // the XCD grid's padding
    } else {
        const int tp = xcd_contiguous_block(blockIdx.x, gridDim.x);
        if (tp >= n_buckets * H) return;
        b = tp / H, h = tp % H;
    }
    // a bucket wider than the accumulator or past the table cannot come from the plan call;
    // clamped all the same, so no plan can make the kernel write outside LDS or grad_cbsr
    const int64_t c0 = bucket_col[b];
    int64_t c1 = bucket_col[b + 1];
    c1 = c1 > num_cols ? num_cols : c1;
    int width = c1 > c0 && c0 >= 0 ? (int)(c1 - c0) : 0;
    width = width > (1 << shift) ? (1 << shift) : width;
    const int s0 = grp_ptr[b];
    const int n_e = width > 0 && grp_ptr[b + 1] > s0 ? grp_ptr[b + 1] - s0 : 0;
    uint8_t *sel_lds = reinterpret_cast<uint8_t *>(acc + (ks << shift));
    for (int i = tid; i < (ks << shift); i += 1024) acc[i] = 0.0;
    pull_sel_store(sel_lds, pull_sel_load_rows(sel_q, c0, width, k, kp, h), kp, shift);
    __syncthreads();
    const auto grs = wave_buffer(Gp, (uint32_t)num_rows * (uint32_t)D * 4u);
    constexpr int RUN = MAXK_PULL_STREAM_RUN;
    for (int e0 = 0; e0 < n_e; e0 += RUN) {  // n_e is the workgroup's: every wave meets the barrier
        const int n = n_e - e0 < RUN ? n_e - e0 : RUN;
        const auto ers = wave_buffer(ent + s0 + e0, (uint32_t)n * 8u);
        pull_q_entries<LR, U, FULLD, VPL, true>(acc, sel_lds, grs, ers, n, D, kp, shift);
        __syncthreads();
    }
    const int w4 = kp / 4;
    for (int i4 = tid; i4 < width * w4; i4 += 1024) {
        const int d = i4 / w4, s4 = i4 % w4;
        const double *a = &acc[d * ks + 4 * s4];
        const size_t r0 = (size_t)(c0 + d) * k;
        const uint32_t m = *reinterpret_cast<const uint32_t *>(lmap + r0 + h * kp + 4 * s4);
        float *row = grad_cbsr + r0;
        row[m & 255u] = (float)a[0];
        row[(m >> 8) & 255u] = (float)a[1];
        row[(m >> 16) & 255u] = (float)a[2];
        row[m >> 24] = (float)a[3];
    }
}

// grad_cbsr rows of bucket j = the sum of its slices' tiles, in slice order.  With lmap
// (pull_q_kernel's slot order, k % 4 == 0) slot f of row c goes to l = lmap[c * k + f].
// Listed tiles (bucket_ptr != nullptr, k % 4 == 0): bucket j's tiles are the list positions
// bucket_tiles[bucket_ptr[j] .. bucket_ptr[j + 1]), in slice order (none: the sum is 0);
// accumulate adds the sum onto grad_cbsr instead of storing it.
__global__ __launch_bounds__(kBlock) void pull_reduce_kernel(const float *__restrict__ tile_out,
                                                             const uint8_t *__restrict__ lmap,
                                                             float *__restrict__ grad_cbsr,
                                                             int64_t num_cols, int n_buckets,
                                                             int slices, int k, int shift,
                                                             const int32_t *__restrict__ bucket_ptr,
                                                             const int32_t *__restrict__ bucket_tiles,
                                                             int accumulate) {
    const int j = blockIdx.x;
    const int64_t c0 = (int64_t)j << shift;
    const int rows = num_cols - c0 < (1 << shift) ? (int)(num_cols - c0) : (1 << shift);
    const int i = blockIdx.y * kBlock + threadIdx.x;
    const int nf = rows * k;  // floats of this bucket; tiles and c0 * k are 16-B aligned
    if (i * 4 >= nf) return;
    const size_t n4 = ((size_t)k << shift) / 4;
    const float4 *to = reinterpret_cast<const float4 *>(tile_out);
    if (i * 4 + 4 > nf) {  // k % 4 != 0: the bucket's last 1..3 floats
        const int f0 = i * 4;
        for (int f = f0; f < nf; ++f) {
            float a = tile_out[(size_t)j * n4 * 4 + f];
            for (int s = 1; s < slices; ++s) a += tile_out[((size_t)s * n_buckets + j) * n4 * 4 + f];
            grad_cbsr[c0 * k + f] = a;
        }
        return;
    }
    float4 a;
    if (bucket_ptr) {
        a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int q = bucket_ptr[j]; q < bucket_ptr[j + 1]; ++q) {
            const float4 b = to[(size_t)bucket_tiles[q] * n4 + i];
            a.x += b.x;
            a.y += b.y;
            a.z += b.z;
            a.w += b.w;
        }
    } else {
        a = to[(size_t)j * n4 + i];
        for (int s = 1; s < slices; ++s) {
            const float4 b = to[((size_t)s * n_buckets + j) * n4 + i];
            a.x += b.x;
            a.y += b.y;
            a.z += b.z;
            a.w += b.w;
        }
    }
    if (lmap) {  // four slots of one row (k % 4 == 0) back to their l
        const size_t f0 = (size_t)c0 * k + (size_t)i * 4;
        const uint32_t m = *reinterpret_cast<const uint32_t *>(lmap + f0);
        float *row = grad_cbsr + (f0 / k) * k;
        if (accumulate) {
            a.x += row[m & 255u];
            a.y += row[(m >> 8) & 255u];
            a.z += row[(m >> 16) & 255u];
            a.w += row[m >> 24];
        }
        row[m & 255u] = a.x;
        row[(m >> 8) & 255u] = a.y;
        row[(m >> 16) & 255u] = a.z;
        row[m >> 24] = a.w;
        return;
    }
    reinterpret_cast<float4 *>(grad_cbsr + c0 * k)[i] = a;
}

// Parts of pull_q_kernel for k and a plan's bucket shift: the fewest H (k % (4H) == 0) whose
// accumulator [k/H << shift] doubles and selector rows [k/H << shift] bytes fit the LDS; 0 if
// none does.
int pull_parts(int k, int shift) {
    for (int H = 1; H <= k / 4; H *= 2) {
        if (k % (4 * H)) break;
        if (pull_fits(k / H, k / H, shift)) return H;  // unpadded fits
    }
    return 0;
}

// Workspace of the pull for `tiles` tile partials of 2^shift destinations each: G' (row_div)
// at offset 0, the partials, then (k % 4 == 0) the slot-ordered selectors and their l map
// (pull_sel_kernel).  The size functions pass the largest shift any plan may carry (tiles x
// 2^shift never shrinks as the shift grows: the columns are rounded up to whole buckets), a
// call its own plan's shift.
struct PullLayout {
    size_t tile_off, sel_off, lmap_off, total;
};

PullLayout pull_layout(int64_t num_rows, int64_t num_cols, int D, int k, int64_t tiles,
                       int shift) {
    PullLayout L{};
    L.tile_off = al256((size_t)num_rows * D * sizeof(float));
    L.sel_off = L.tile_off + (size_t)tiles * ((size_t)k << shift) * sizeof(float);
    const size_t nsel = k % 4 == 0 ? al256((size_t)num_cols * k) : 0;
    L.lmap_off = L.sel_off + nsel;
    L.total = L.lmap_off + nsel;
    return L;
}

// pull_q_kernel's values per lane: 4 (one u32 selector word per lane; 2 lanes per entry for
// 8-slot parts), 8 for k = 8 (one lane per entry, one u64 selector word; MAXK_PULL_VPL8)
int pull_vpl(int kp, int parts) {
    return kp != 8 ? 4 : MAXK_PULL_VPL8 ? MAXK_PULL_VPL8 : parts == 1 ? 8 : 4;
}

// The slot-ordered selectors sel_q and their l map lm of every destination (pull_sel_kernel).
int launch_pull_sel(const uint8_t *cbsr_idx, uint8_t *sel_q, uint8_t *lm, int64_t num_cols, int k,
                    int kp, int vpl, hipStream_t s) {
    if (MAXK_PULL_SEL4 && (reinterpret_cast<uintptr_t>(cbsr_idx) & 3) == 0) {
        const int nd4 = kBlock / (k / 4);
        hipLaunchKernelGGL(pull_sel4_kernel, dim3((unsigned)ceil_div(num_cols, nd4)),
                           dim3(kBlock), 0, s, cbsr_idx, sel_q, lm, num_cols, k, kp, vpl);
        MAXK_LAUNCHED("pull_sel4_kernel");
    } else {
        const int nd = kBlock / k;
        hipLaunchKernelGGL(pull_sel_kernel, dim3((unsigned)ceil_div(num_cols, nd)),
                           dim3(kBlock), 0, s, cbsr_idx, sel_q, lm, num_cols, k, kp, vpl);
        MAXK_LAUNCHED("pull_sel_kernel");
    }
    return MAXK_OK;
}

int pull_impl(const float *grad_out, const float *row_div, const uint8_t *cbsr_idx,
              const int32_t *tile_ptr, const uint32_t *ent, int32_t bucket_shift, int32_t slices,
              bool listed, const int32_t *tile_list, int32_t n_list, const int32_t *bucket_ptr,
              const int32_t *bucket_tiles, int32_t accumulate, float *grad_cbsr, int64_t num_rows,
              int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k, void *workspace,
              size_t workspace_bytes, void *stream) {
    if (int rc = check_common(num_rows, num_cols, num_e, dim_origin, dim_k, 0)) return rc;
    MAXK_REQUIRE(dim_k % 4 == 0 || dim_k <= 64,
                 "pull backward needs dim_k %% 4 == 0 or dim_k <= 64, got %d", dim_k);
    MAXK_REQUIRE(dim_origin % 4 == 0, "pull backward needs dim_origin %% 4 == 0, got %d",
                 dim_origin);
    const bool v4 = dim_k % 4 == 0;
    // quantile-slot form with H parts (k % 4 == 0), else the one-l-per-lane pull_tile_kernel
    const int parts = MAXK_PULL_Q && v4 && bucket_shift >= 4 && bucket_shift <= 15
                          ? pull_parts(dim_k, bucket_shift)
                          : 0;
    const int max_shift = std::max(maxk_bucket_shift(dim_k), maxk_pull_shift(dim_k));
    MAXK_REQUIRE(bucket_shift >= 4 && bucket_shift <= 15 && bucket_shift <= max_shift &&
                     (parts > 0 || bucket_shift <= maxk_bucket_shift(dim_k)),
                 "bucket_shift %d out of range [4, min(15, %d)] for dim_k %d", bucket_shift,
                 max_shift, dim_k);
    const int64_t nb = maxk_bucket_count(num_cols, bucket_shift);
    MAXK_REQUIRE(slices >= 1 && slices * nb < (1LL << 31), "slices %d out of range", slices);
    const int64_t rps = (num_rows + slices - 1) / slices;
    MAXK_REQUIRE(rps <= 65536, "%d slices leave %lld rows per slice (max 65536)", slices,
                 (long long)rps);
    hipStream_t s = as_stream(stream);
    if (num_cols == 0) return MAXK_OK;
    MAXK_REQUIRE(grad_cbsr && tile_ptr, "grad_cbsr/tile_ptr must not be NULL");
    MAXK_REQUIRE(num_e == 0 || (grad_out && cbsr_idx && ent),
                 "grad/selector/plan pointers must not be NULL");
    MAXK_REQUIRE(!listed || (parts > 0 && bucket_ptr && n_list >= 0 &&
                             (n_list == 0 || (tile_list && bucket_tiles))),
                 "listed tiles need dim_k %% 4 == 0 and tile_list/bucket_ptr/bucket_tiles");
    const int64_t tiles = listed ? (int64_t)n_list : (int64_t)slices * nb;
    const PullLayout L = pull_layout(num_rows, num_cols, dim_origin, dim_k, tiles, bucket_shift);
    MAXK_REQUIRE(workspace && workspace_bytes >= L.total,
                 "workspace too small: need %zu bytes, got %zu", L.total, workspace_bytes);
    char *ws = reinterpret_cast<char *>(workspace);
    // accumulate: bit 0 adds onto grad_cbsr; bit 1 (MAXK_PULL_NO_REDUCE) stops at the tile
    // partials, bit 2 (MAXK_PULL_REDUCE_ONLY) runs only the reduce over a workspace the same
    // call with bit 1 filled (listed tiles only: the hybrid runs the two-phase form between)
    const bool front = !(accumulate & MAXK_PULL_REDUCE_ONLY);
    const bool back = !(accumulate & MAXK_PULL_NO_REDUCE);
    MAXK_REQUIRE(listed || (front && back), "reduce-only / no-reduce need listed tiles");
    MAXK_REQUIRE(front || back, "no-reduce and reduce-only together run nothing");
    const int k = dim_k;
    const float *Gp = grad_out;
    if (front && row_div && num_rows > 0 && num_e > 0) {
        const int64_t n4 = num_rows * dim_origin / 4;
        hipLaunchKernelGGL(gprime_kernel, dim3((unsigned)ceil_div(n4, kBlock)), dim3(kBlock), 0,
                           s, grad_out, row_div, reinterpret_cast<float *>(workspace), n4,
                           dim_origin / 4);
        MAXK_LAUNCHED("gprime_kernel");
        Gp = reinterpret_cast<const float *>(workspace);
    }
    float *tile_out = reinterpret_cast<float *>(ws + L.tile_off);
    const size_t acc_b = ((size_t)(k + 1) << bucket_shift) * sizeof(double);
    const size_t sel_b = ((size_t)k << bucket_shift);
    const bool sel_lds = acc_b + sel_b <= kPullLdsBytes;
    const size_t lds = acc_b + (sel_lds ? sel_b : 0);
    const uint2 *ent2 = reinterpret_cast<const uint2 *>(ent);
    const uint8_t *lmap = nullptr;
    if (parts > 0) {  // quantile-slot form (pull_q_kernel), `parts` workgroups per tile
        const int kp = k / parts;
        const size_t lds_q = pull_lds_bytes(pull_ks(kp, bucket_shift), kp, bucket_shift);
        uint8_t *sel_q = reinterpret_cast<uint8_t *>(ws + L.sel_off);
        uint8_t *lm = reinterpret_cast<uint8_t *>(ws + L.lmap_off);
        const int vpl = pull_vpl(kp, parts);
        lmap = lm;
        if (!front) goto reduce;
        if (int rc = launch_pull_sel(cbsr_idx, sel_q, lm, num_cols, k, kp, vpl, s)) return rc;
        const int64_t work = tiles * parts;
        const bool fulld = dim_origin == kMaxDim;
        const unsigned grid = (unsigned)(MAXK_PULL_XCD ? xcd_grid(work) : work);
        if (work == 0) goto reduce;  // no listed tile: the reduce only permutes / accumulates
        // lanes per entry: vpl 2 and 8 exist for 8-slot parts only (4 lanes, 1 lane)
        const int lr = vpl == 4 ? lanes_per_edge(kp / 4) : kp / vpl;
        const bool ok = with_lanes(lr, [&](auto lr_c) {
            with_const<2, 4, 8>(vpl, [&](auto vpl_c) {
                with_const<0, 1>(fulld, [&](auto fd_c) {
                    constexpr int LR = decltype(lr_c)::value, VPL = decltype(vpl_c)::value;
                    if constexpr (VPL == 4 || LR * VPL == 8)
                        hipLaunchKernelGGL(
                            (pull_q_kernel<LR, MAXK_PULL_QU, decltype(fd_c)::value, VPL>),
                            dim3(grid), dim3(1024), lds_q, s, Gp, sel_q, tile_ptr, ent2, tile_out,
                            num_cols, (int)nb, (int)tiles, (int)rps, num_rows, dim_origin, k, kp,
                            bucket_shift, tile_list);
                });
            });
        });
        if (!ok) return bad_lanes(lr);
        MAXK_LAUNCHED("pull_q_kernel");
    } else {
        // pull_tile_kernel: four l per lane (one u32 selector read) when k % 4 == 0, else one
        const int lr = lanes_per_edge(v4 ? k / 4 : k);
        const bool ok = with_lanes(lr, [&](auto lr_c) {
            with_const<0, 1>(sel_lds, [&](auto sl_c) {
                with_const<1, 4>(v4 ? 4 : 1, [&](auto vpl_c) {
                    hipLaunchKernelGGL(
                        (pull_tile_kernel<decltype(lr_c)::value, MAXK_PULL_U,
                                          decltype(sl_c)::value, decltype(vpl_c)::value>),
                        dim3((unsigned)tiles), dim3(1024), lds, s, Gp, cbsr_idx, tile_ptr, ent2,
                        tile_out, num_cols, (int)nb, (int)rps, dim_origin, k, bucket_shift);
                });
            });
        });
        if (!ok) return bad_lanes(lr);
        MAXK_LAUNCHED("pull_tile_kernel");
    }
reduce:
    if (!back) return MAXK_OK;
    hipLaunchKernelGGL(pull_reduce_kernel,
                       dim3((unsigned)nb, (unsigned)ceil_div(ceil_div((int64_t)k << bucket_shift, 4), kBlock)),
                       dim3(kBlock), 0, s, tile_out, lmap, grad_cbsr, num_cols, (int)nb, slices,
                       k, bucket_shift, listed ? bucket_ptr : nullptr,
                       listed ? bucket_tiles : nullptr, accumulate & 1);
    MAXK_LAUNCHED("pull_reduce_kernel");
    return MAXK_OK;
}

// ---- the stream form -------------------------------------------------------------------
// Largest share, in thousandths, by which the stream form may narrow the mean bucket against
// the tiled form's 2^shift columns (whole rounds of workgroups need more, narrower buckets, and
// a source row then meets more of them).  Measured at 109 (Reddit-sized, 114 -> 128 buckets:
// DESIGN 5.2); nothing wider has been measured, so nothing wider is accepted.
#ifndef MAXK_PULL_STREAM_NARROW
#define MAXK_PULL_STREAM_NARROW 125
#endif

int64_t stream_buckets(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k,
                       int64_t cus) {
    if (!MAXK_PULL_Q || MAXK_PULL_STREAM_NARROW <= 0) return 0;
    if (num_rows <= 0 || num_cols <= 0 || D <= 0 || D > kMaxDim || D % 4 || k <= 0 || k > D || k % 4)
        return 0;
    if (num_rows >= (1LL << 31) || num_cols >= (1LL << 31) || num_cols * (int64_t)k >= (1LL << 31))
        return 0;
    const int shift = maxk_pull_shift(k);
    const int H = shift >= 4 && shift <= 15 ? pull_parts(k, shift) : 0;
    if (H <= 0) return 0;
    // gather offsets row * D * 4 + column * 4 stay below the "no entry" offset 2^31, far inside
    // the 2^32 a descriptor over G' reaches; entry offsets are 32-bit as well
    if (num_rows * D * 4 >= (1LL << 31) || num_e >= (1LL << 28)) return 0;
    int row_bits = 0;
    while ((1LL << row_bits) < num_rows) ++row_bits;
    if (row_bits + shift > 32) return 0;
    if (cus <= 0) cus = device_cus();
    const int64_t nb_min = (num_cols + (1LL << shift) - 1) >> shift;
    const int64_t rounds = (nb_min * H + cus - 1) / cus;
    const int64_t nb = rounds * cus / H;
    if (nb < nb_min || nb * H >= (1LL << 24)) return 0;
    return (nb - nb_min) * 1000 <= nb * MAXK_PULL_STREAM_NARROW ? nb : 0;
}

int pull_stream_impl(const float *grad_out, const float *row_div, const uint8_t *cbsr_idx,
                     const int32_t *bucket_col, const int32_t *grp_ptr, const uint32_t *ent,
                     int32_t n_buckets, float *grad_cbsr, int64_t num_rows, int64_t num_cols,
                     int64_t num_e, int32_t dim_origin, int32_t dim_k, void *workspace,
                     size_t workspace_bytes, void *stream) {
    if (int rc = check_common(num_rows, num_cols, num_e, dim_origin, dim_k, 0)) return rc;
    const int k = dim_k;
    MAXK_REQUIRE(MAXK_PULL_Q && k % 4 == 0 && dim_origin % 4 == 0,
                 "stream pull needs dim_k %% 4 == 0 and dim_origin %% 4 == 0, got %d, %d", k,
                 dim_origin);
    const int shift = maxk_pull_shift(k);
    const int parts = shift >= 4 && shift <= 15 ? pull_parts(k, shift) : 0;
    MAXK_REQUIRE(parts > 0, "no part count fits dim_k %d", k);
    MAXK_REQUIRE(num_rows * dim_origin * 4 < (1LL << 31), "stream pull: G of 2 GiB or more");
    MAXK_REQUIRE(num_e < (1LL << 28), "stream pull: 2^28 entries or more");
    int row_bits = 0;
    while ((1LL << row_bits) < num_rows) ++row_bits;
    MAXK_REQUIRE(row_bits + shift <= 32, "stream pull: %d row bits + %d column bits exceed 32",
                 row_bits, shift);
    MAXK_REQUIRE(n_buckets >= 1 && (int64_t)n_buckets * parts < (1LL << 24) &&
                     ((int64_t)n_buckets << shift) >= num_cols,
                 "n_buckets %d out of range", n_buckets);
    hipStream_t s = as_stream(stream);
    if (num_cols == 0) return MAXK_OK;
    MAXK_REQUIRE(grad_cbsr && bucket_col && grp_ptr && cbsr_idx,
                 "grad_cbsr/bucket_col/grp_ptr/selector pointers must not be NULL");
    MAXK_REQUIRE(num_e == 0 || (grad_out && ent), "grad/plan pointers must not be NULL");
    const PullLayout L = pull_layout(num_rows, num_cols, dim_origin, k, 0, shift);
    MAXK_REQUIRE(workspace && workspace_bytes >= L.total,
                 "workspace too small: need %zu bytes, got %zu", L.total, workspace_bytes);
    char *ws = reinterpret_cast<char *>(workspace);
    const float *Gp = grad_out;
    if (row_div && num_rows > 0 && num_e > 0) {
        const int64_t n4 = num_rows * dim_origin / 4;
        hipLaunchKernelGGL(gprime_kernel, dim3((unsigned)ceil_div(n4, kBlock)), dim3(kBlock), 0,
                           s, grad_out, row_div, reinterpret_cast<float *>(workspace), n4,
                           dim_origin / 4);
        MAXK_LAUNCHED("gprime_kernel");
        Gp = reinterpret_cast<const float *>(workspace);
    }
    const int kp = k / parts;
    const int vpl = pull_vpl(kp, parts);
    uint8_t *sel_q = reinterpret_cast<uint8_t *>(ws + L.sel_off);
    uint8_t *lm = reinterpret_cast<uint8_t *>(ws + L.lmap_off);
    if (int rc = launch_pull_sel(cbsr_idx, sel_q, lm, num_cols, k, kp, vpl, s)) return rc;
    const size_t lds_q = pull_lds_bytes(pull_ks(kp, shift), kp, shift);
    const unsigned grid = (unsigned)xcd_grid((int64_t)n_buckets * parts);
    const bool fulld = dim_origin == kMaxDim;
    const int lr = vpl == 4 ? lanes_per_edge(kp / 4) : kp / vpl;
    const bool ok = with_lanes(lr, [&](auto lr_c) {
        with_const<2, 4, 8>(vpl, [&](auto vpl_c) {
            with_const<0, 1>(fulld, [&](auto fd_c) {
                constexpr int LR = decltype(lr_c)::value, VPL = decltype(vpl_c)::value;
                if constexpr (VPL == 4 || LR * VPL == 8)
                    hipLaunchKernelGGL(
                        (pull_q_kernel<LR, MAXK_PULL_QU, decltype(fd_c)::value, VPL, 1>),
                        dim3(grid), dim3(1024), lds_q, s, Gp, sel_q, lm, bucket_col, grp_ptr,
                        reinterpret_cast<const uint2 *>(ent), grad_cbsr, num_cols, (int)n_buckets,
                        num_rows, dim_origin, k, kp, shift);
            });
        });
    });
    if (!ok) return bad_lanes(lr);
    MAXK_LAUNCHED("pull_q_kernel");
    return MAXK_OK;
}
}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" int64_t maxk_pull_stream_buckets(int64_t num_rows, int64_t num_cols, int64_t num_e,
                                            int32_t dim_origin, int32_t dim_k, int32_t cus) {
    return stream_buckets(num_rows, num_cols, num_e, dim_origin, dim_k, cus);
}

extern "C" size_t maxk_sspmm_backward_pull_stream_workspace_size(int64_t num_rows,
                                                                 int64_t num_cols,
                                                                 int32_t dim_origin,
                                                                 int32_t dim_k) {
    if (num_rows < 0 || num_cols < 0 || dim_origin <= 0 || dim_k <= 0) return 0;
    return pull_layout(num_rows, num_cols, dim_origin, dim_k, 0, 0).total;
}

extern "C" int maxk_sspmm_backward_pull_stream(const float *grad_out, const float *row_div,
                                               const uint8_t *cbsr_idx, const int32_t *bucket_col,
                                               const int32_t *grp_ptr, const uint32_t *ent,
                                               int32_t n_buckets, float *grad_cbsr,
                                               int64_t num_rows, int64_t num_cols, int64_t num_e,
                                               int32_t dim_origin, int32_t dim_k, void *workspace,
                                               size_t workspace_bytes, void *stream) {
    clear_error();
    return pull_stream_impl(grad_out, row_div, cbsr_idx, bucket_col, grp_ptr, ent, n_buckets,
                            grad_cbsr, num_rows, num_cols, num_e, dim_origin, dim_k, workspace,
                            workspace_bytes, stream);
}

extern "C" size_t maxk_sspmm_backward_pull_workspace_size(int64_t num_rows, int64_t num_cols,
                                                          int32_t dim_origin, int32_t dim_k,
                                                          int32_t slices) {
    if (num_rows < 0 || num_cols < 0 || dim_origin <= 0 || dim_k <= 0 || slices <= 0) return 0;
    const int shift = std::max(maxk_bucket_shift(dim_k), maxk_pull_shift(dim_k));
    return pull_layout(num_rows, num_cols, dim_origin, dim_k,
                       (int64_t)slices * maxk_bucket_count(num_cols, shift), shift).total;
}

extern "C" int maxk_sspmm_backward_pull(const float *grad_out, const float *row_div,
                                        const uint8_t *cbsr_idx, const int32_t *tile_ptr,
                                        const uint32_t *ent, int32_t bucket_shift,
                                        int32_t slices, float *grad_cbsr, int64_t num_rows,
                                        int64_t num_cols, int64_t num_e, int32_t dim_origin,
                                        int32_t dim_k, void *workspace, size_t workspace_bytes,
                                        void *stream) {
    clear_error();
    return pull_impl(grad_out, row_div, cbsr_idx, tile_ptr, ent, bucket_shift, slices, false,
                     nullptr, 0, nullptr, nullptr, 0, grad_cbsr, num_rows, num_cols, num_e, dim_origin, dim_k,
                     workspace, workspace_bytes, stream);
}

extern "C" size_t maxk_sspmm_backward_pull_tiles_workspace_size(int64_t num_rows,
                                                                int64_t num_cols,
                                                                int32_t dim_origin,
                                                                int32_t dim_k, int32_t n_tiles) {
    if (num_rows < 0 || num_cols < 0 || dim_origin <= 0 || dim_k <= 0 || n_tiles < 0) return 0;
    return pull_layout(num_rows, num_cols, dim_origin, dim_k, n_tiles,
                       std::max(maxk_bucket_shift(dim_k), maxk_pull_shift(dim_k))).total;
}

extern "C" int maxk_sspmm_backward_pull_tiles(
    const float *grad_out, const float *row_div, const uint8_t *cbsr_idx,
    const int32_t *tile_list, const int32_t *tile_ent, int32_t n_tiles,
    const int32_t *bucket_ptr, const int32_t *bucket_tiles, const uint32_t *ent,
    int32_t bucket_shift, int32_t slices, int32_t accumulate, float *grad_cbsr,
    int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
    void *workspace, size_t workspace_bytes, void *stream) {
    clear_error();
    MAXK_REQUIRE(tile_ent, "tile_ent must not be NULL");
    return pull_impl(grad_out, row_div, cbsr_idx, tile_ent, ent, bucket_shift, slices, true,
                     tile_list, n_tiles, bucket_ptr, bucket_tiles, accumulate, grad_cbsr, num_rows, num_cols,
                     num_e, dim_origin, dim_k, workspace, workspace_bytes, stream);
}
