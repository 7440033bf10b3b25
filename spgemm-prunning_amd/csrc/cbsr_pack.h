// Packed CBSR records and the token-stream item size, shared by the kernels that gather one
// record per edge: the forward (spgemm_fwd.hip), the edge-weight gradient (edge_grad.hip) and
// the multi-head forwards and the attention backwards (through heads_walk.h and piece_walk.h).
// RecordSlot is how every one of them addresses a slot of a record.
// Each translation unit gets its own copy of the pack kernels (anonymous namespace, like
// slab_fixup_kernel in common.h).
#pragma once

#include "common.h"

namespace maxk {
namespace {

// Record stride: one power-of-two slot per vertex while the record
// [k f32 | k u16 selectors] fits a 128-B line, else whole lines.
// Past one line: whole 64-B sectors while the table stays well inside the 256 MiB
// Infinity Cache (a smaller cache-resident table: Reddit k=32 3.60 -> 3.49 ms), whole
// 128-B lines once it does not (every gather is then a random HBM request per line and
// line-aligned records measured better: products k=32 6.53 -> 6.40 ms).
inline int record_stride(int k, int64_t num_cols) {
    const int b = 6 * k;
    if (b <= 128) {
        int s = 16;
        while (s < b) s <<= 1;
        return s;
    }
    const int s64 = (b + 63) / 64 * 64;
    if ((int64_t)s64 * num_cols <= (128LL << 20)) return s64;
    return (b + 127) / 128 * 128;
}

// A graph of at least this average degree is "dense" to the record walkers (long rows).
constexpr int64_t kFwdSparseDegree = 128;

// Packs the records of groups of whole vertices (vpw = min(32, 512 / k) per
// workgroup, one thread per (vertex, l)), grid-stride: a launch of one small
// workgroup per 256 (vertex, l) pairs is bound by workgroup dispatch (products
// k=32: 306k workgroups, 1.65 ms).  Duplicate selectors of a vertex: the first
// occurrence (lowest l, found with an LDS atomicMin per (vertex, selector))
// carries the sum of their values in l order, the others point at the trash
// column with value 0.  Selectors >= D also go to trash.  A record's u16 selector is the
// selector itself when it is kept, else 0x100 | selector: the walkers take min(selector,
// trash) as the LDS column (every index in [D, DS) is a never-flushed pad column of the copy),
// and the low byte stays the caller's selector, which the edge-selector stream of
// maxk_spgemm_forward_sel needs.
constexpr int kPackMaxV = 32;     // vertices per group (LDS: 32 x 256 first-occurrence slots)
constexpr int kPackBlock = 512;   // threads per pack workgroup (products: 0.34 -> 0.21 ms vs 256)

__global__ __launch_bounds__(kPackBlock) void cbsr_pack_kernel(const float *__restrict__ cbsr_val,
                                                           const uint8_t *__restrict__ cbsr_idx,
                                                           uint8_t *__restrict__ rec, int num_cols,
                                                           int k, int RS, int D, int trash) {
    __shared__ uint32_t s_first[kPackMaxV][256];
    __shared__ uint8_t s_sel[kPackBlock];
    __shared__ float s_val[kPackBlock];
    __shared__ int s_dup[kPackMaxV];
    const int vpw = k >= kPackBlock / kPackMaxV ? kPackBlock / k : kPackMaxV;
    const int t = threadIdx.x;
    const int vl = t / k, l = t - vl * k;
    for (int64_t g0 = (int64_t)blockIdx.x * vpw; g0 < num_cols; g0 += (int64_t)gridDim.x * vpw) {
        const int64_t v = g0 + vl;
        const bool act = vl < vpw && v < num_cols;
        int s = 0;
        float val = 0.f;
        if (act) {
            s = cbsr_idx[v * k + l];
            val = cbsr_val[v * k + l];
            s_sel[t] = (uint8_t)s;
            s_val[t] = val;
            s_first[vl][s] = 0xffffffffu;
        }
        if (t < vpw) s_dup[t] = 0;
        __syncthreads();
        if (act) atomicMin(&s_first[vl][s], (uint32_t)l);
        __syncthreads();
        const bool first = act && s_first[vl][s] == (uint32_t)l;
        if (act && !first) s_dup[vl] = 1;
        __syncthreads();
        if (act) {
            float outv = val;
            if (first && s_dup[vl]) {  // rare: fold the later duplicates, in l order
                for (int j = l + 1; j < k; ++j)
                    if (s_sel[vl * k + j] == s) outv += s_val[vl * k + j];
            }
            const bool keep = first && s < D;
            uint8_t *p = rec + v * RS;
            reinterpret_cast<float *>(p)[l] = keep ? outv : 0.f;
            reinterpret_cast<uint16_t *>(p + 4 * k)[l] = (uint16_t)(keep ? s : (0x100 | s));
        }
        __syncthreads();  // LDS is reused by the next group
    }
}

// cbsr_pack_kernel with four l per thread (k % 4 == 0, 16-B aligned values, 4-B aligned
// selectors): one u32 selector load, one float4 value load, one 16-B and one 8-B store per
// thread.  Duplicates are detected with a 256-bit column set per vertex (atomicOr returns
// the bit already set); a vertex with any takes the byte loop of cbsr_pack_kernel's rule
// (the lowest l of a selector carries the sum of its duplicates in l order).
__global__ __launch_bounds__(kPackBlock) void cbsr_pack4_kernel(const float *__restrict__ cbsr_val,
                                                            const uint8_t *__restrict__ cbsr_idx,
                                                            uint8_t *__restrict__ rec,
                                                            int num_cols, int k, int RS, int D,
                                                            int trash) {
    __shared__ uint32_t s_bits[kPackBlock * 8];  // up to kPackBlock vertices (k = 4)
    __shared__ int s_dup[kPackBlock];
    const int tpv = k >> 2;          // threads per vertex
    const int vpw = kPackBlock / tpv;  // vertices per group
    const int t = threadIdx.x;
    const int vl = t / tpv, l0 = (t - vl * tpv) * 4;
    for (int64_t g0 = (int64_t)blockIdx.x * vpw; g0 < num_cols; g0 += (int64_t)gridDim.x * vpw) {
        const int64_t v = g0 + vl;
        const bool act = vl < vpw && v < num_cols;
        for (int i = t; i < vpw * 8; i += kPackBlock) s_bits[i] = 0u;
        if (t < vpw) s_dup[t] = 0;
        __syncthreads();
        uint32_t w = 0u;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (act) {
            w = *reinterpret_cast<const uint32_t *>(cbsr_idx + v * k + l0);
            x = *reinterpret_cast<const float4 *>(cbsr_val + v * k + l0);
            uint32_t dup = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t sj = (w >> (8 * j)) & 255u;
                const uint32_t old = atomicOr(&s_bits[vl * 8 + (sj >> 5)], 1u << (sj & 31));
                dup |= (old >> (sj & 31)) & 1u;
            }
            if (dup) s_dup[vl] = 1;
        }
        __syncthreads();
        if (act) {
            float o[4] = {x.x, x.y, x.z, x.w};
            uint32_t sel[4];
            const bool any_dup = s_dup[vl] != 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t sj = (w >> (8 * j)) & 255u;
                bool first = true;
                if (any_dup) {  // rare
                    const int l = l0 + j;
                    const uint8_t *ci = cbsr_idx + v * k;
                    const float *cv = cbsr_val + v * k;
                    for (int m = 0; m < l; ++m) first = first && ci[m] != sj;
                    if (first)
                        for (int m = l + 1; m < k; ++m)
                            if (ci[m] == sj) o[j] += cv[m];
                }
                const bool keep = first && (int)sj < D;
                o[j] = keep ? o[j] : 0.f;
                sel[j] = keep ? sj : (0x100u | sj);
            }
            uint8_t *p = rec + v * RS;
            *reinterpret_cast<float4 *>(p + 4 * l0) = make_float4(o[0], o[1], o[2], o[3]);
            *reinterpret_cast<uint2 *>(p + 4 * k + 2 * l0) =
                make_uint2(sel[0] | (sel[1] << 16), sel[2] | (sel[3] << 16));
        }
        __syncthreads();  // LDS is reused by the next group
    }
}

// The pack of every column's record into rec (num_cols records of RS bytes): four l per thread
// where k and the CBSR's alignment allow, else one.  Launches nothing for num_cols == 0.
inline int launch_cbsr_pack(const float *cbsr_val, const uint8_t *cbsr_idx, uint8_t *rec,
                            int64_t num_cols, int k, int RS, int D, int trash, hipStream_t s) {
    if (num_cols > 0 && MAXK_PACK4 && k % 4 == 0 && ((uintptr_t)cbsr_val & 15) == 0 &&
        ((uintptr_t)cbsr_idx & 3) == 0) {
        const int vpw = kPackBlock / (k / 4);
        const int64_t groups = ceil_div(num_cols, (int64_t)vpw);
        hipLaunchKernelGGL(cbsr_pack4_kernel,
                           dim3((unsigned)(groups < MAXK_PACK_GRID ? groups : MAXK_PACK_GRID)),
                           dim3(kPackBlock), 0,
                           s, cbsr_val, cbsr_idx, rec, (int)num_cols, k, RS, D, trash);
        MAXK_LAUNCHED("cbsr_pack4_kernel");
    } else if (num_cols > 0) {
        const int vpw = k >= kPackBlock / kPackMaxV ? kPackBlock / k : kPackMaxV;
        const int64_t groups = ceil_div(num_cols, (int64_t)vpw);
        hipLaunchKernelGGL(cbsr_pack_kernel,
                           dim3((unsigned)(groups < MAXK_PACK_GRID ? groups : MAXK_PACK_GRID)),
                           dim3(kPackBlock), 0,
                           s, cbsr_val, cbsr_idx, rec, (int)num_cols, k, RS, D, trash);
        MAXK_LAUNCHED("cbsr_pack_kernel");
    }
    return MAXK_OK;
}

// Records of the streaming walker: cbsr_pack*_kernel's, value at c*RS + 4l, u16 selector at
// c*RS + 4k + 2l (a folded duplicate or a selector >= D is stored as 0x100 | s, so
// min(s, trash) is the LDS column).
struct PackedSrc {
    __amdgpu_buffer_rsrc_t rrs;
    uint32_t vo, so, RS;
    __device__ __forceinline__ void load(int c, float &v, int &s) const {
        const uint32_t ro = __umul24((uint32_t)c, RS);
        v = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrs, (int)(ro + vo), 0, 0));
        s = __builtin_amdgcn_raw_buffer_load_b16(rrs, (int)(ro + so), 0, 0);
    }
    __device__ __forceinline__ int col(int s, int D, int trash) const {
        (void)D;
        return min(s, trash);
    }
};

// Slot l of a k-slot record as a lane reads it.  ok: the record has the slot.  A lane past it
// (l >= k) reads the last slot instead (lc, the clamped slot: no load leaves the record) and
// contributes nothing.  The record's layout is spelled here and in the pack kernels alone.
struct RecordSlot {
    bool ok;
    uint32_t lc;
    __device__ __forceinline__ RecordSlot(int l, int k)
        : ok(l < k), lc((uint32_t)(ok ? l : k - 1)) {}
    __device__ __forceinline__ PackedSrc src(__amdgpu_buffer_rsrc_t rrs, int k, int RS) const {
        return PackedSrc{rrs, 4u * lc, 4u * (uint32_t)k + 2u * lc, (uint32_t)RS};
    }
};

// Long rows (a dense graph, e.g. a Reddit-sized graph's vertex-range shard: 14.4M tokens at
// N = 8, rows of ~490 edges): items of at least two average rows (at most 1024 tokens), so most
// rows are walked whole instead of split into slabs (that shard's forward at 256 / 512 / 1024 /
// 2048 tokens: 0.256 / 0.237 / 0.237 / 0.254 ms; the N = 4 shard at 438 / 1024: 0.449 / 0.440;
// profiles/r05/tune/fwd_chunk_shards/) -- while the items still fill every wave slot (a small
// dense graph keeps the one-round sizing below)
inline int64_t fwd_long_rows(int64_t num_rows, int64_t num_e, int64_t c, int resident) {
    if (num_rows <= 0 || num_e < kFwdSparseDegree * num_rows) return c;
    const int64_t two_rows = (2 * ceil_div(num_e, num_rows) + 63) / 64 * 64;
    const int64_t want = two_rows < 1024 ? two_rows : 1024;
    if (c >= want || (num_rows + num_e) / want < device_cus() * resident) return c;
    return want;
}

inline int fwd_chunk(int64_t num_rows, int64_t num_e, int32_t chunk, int resident) {
    if (chunk > 0) return chunk;
    // ~8 waves of work per resident wave slot on the device's CUs (256 on MI355X), within
    // [256, 2048] tokens
    const int64_t total = num_rows + num_e;
    const int64_t cus = device_cus();
    int64_t c = ceil_div(total, cus * 32 * 8);
    if (c >= 256) return (int)fwd_long_rows(num_rows, num_e, c > 2048 ? 2048 : c, resident);
    // A smaller graph has fewer items than wave slots at 256 tokens: size the items so all of
    // them are resident in one round (90 % of the slots, for uneven block placement), since each
    // wave is a chain of dependent gathers and a second round costs a whole item's latency.
    // Flickr-sized (1.08M tokens, 7168 slots): 151 tokens would fill every slot; the forward at
    // 144 / 160 / 176 / 192 / 256 tokens takes 0.0527 / 0.049 / 0.051 / 0.053 / 0.0585 ms
    // (profiles/r04/tune/flickr_chunk_sweep.txt).
    c = ceil_div(total * 10, cus * resident * 9);
    return (int)fwd_long_rows(num_rows, num_e, c < 64 ? 64 : (c > 256 ? 256 : c), resident);
}

// Capacity, in items, of what a walk sized by fwd_chunk keeps per item (slabs, slots): at least
// the item count and non-decreasing in the token count, which the item count of fwd_chunk's auto
// rule is not (one token more can make the items one token longer and fewer).  The auto rule's
// items hold at least 64 tokens, and at least tokens / (256 items per CU) until they reach 2048:
// at most min(tokens / 64, 256 per CU) items below that size and tokens / 2048 at it.
inline int64_t item_cap(int64_t tokens, int chunk, int n_items) {
    if (chunk > 0) return n_items;
    const int64_t a = ceil_div(tokens, 64), k = device_cus() * 256;
    const int64_t lo = a < k ? a : k, hi = ceil_div(tokens, 2048);
    const int64_t cap = lo > hi ? lo : hi;
    return cap > n_items ? cap : n_items;
}

// LDS row stride per copy: D padded to 16 B, plus one 16-B group holding the
// trash column (index DS-1, never read by the flush).
inline int copy_stride(int D) { return ((D + 3) / 4) * 4 + 4; }

}  // namespace
}  // namespace maxk
