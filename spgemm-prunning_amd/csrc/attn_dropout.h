// The attention-dropout mask: a pure function of (seed, head, edge), recomputed wherever it is
// needed and stored nowhere.
//
//   (r0, r1, r2, r3) = Philox4x32-10(counter = (e, 0, h >> 2, 0), key = (seed lo, seed hi))
//   r    = r[h & 3]
//   drop = r < thr,   thr = min(floor(p * 2^32), 2^32 - 1)      (host, in double)
//   d_he = drop ? 0 : scale,   scale = (float)(1 / (1 - (double)p))
//
// e is the edge's CSR position.  Nothing else enters: not chunk_edges, not the work-item cut, not
// num_heads or the padded head count, not which kernel asks.  One evaluation serves the four
// heads of a quad (drop_bits).  Included by every kernel that masks: attn_dropout.hip (the
// elementwise entry), gat_attention_heads.hip, gat_attention_heads_bwd.hip,
// dot_attention_heads.hip and dot_attention_heads_bwd.hip.
#pragma once
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "common.h"

namespace maxk {

// What a kernel takes of (p, seed): by value, so a captured graph replays the same mask.
struct DropMask {
    uint32_t key0, key1, thr;
    float scale;
};

// A kernel template's mask argument: nothing where it does not mask.
struct NoMask {};
template <bool DROP>
using MaskArg = std::conditional_t<DROP, DropMask, NoMask>;

inline bool dropout_rate_ok(float p) { return p >= 0.f && p < 1.f; }  // a NaN fails both

inline uint32_t dropout_threshold(float p) {
    const double t = std::floor((double)p * 4294967296.0);
    return t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
}

inline float dropout_scale(float p) { return (float)(1.0 / (1.0 - (double)p)); }

inline DropMask drop_mask(float p, uint64_t seed) {
    return DropMask{(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), dropout_threshold(p),
                    dropout_scale(p)};
}

inline int check_dropout(float p) {
    MAXK_REQUIRE(dropout_rate_ok(p), "p must be in [0, 1), got %g", (double)p);
    return MAXK_OK;
}

// Philox4x32-10 (Salmon et al., SC'11): counter c, key k, output r.
__host__ __device__ __forceinline__ void philox4x32_10(const uint32_t (&c)[4],
                                                       const uint32_t (&k)[2], uint32_t (&r)[4]) {
    uint32_t x0 = c[0], x1 = c[1], x2 = c[2], x3 = c[3], k0 = k[0], k1 = k[1];
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t a = (uint64_t)0xD2511F53u * x0;
        const uint64_t b = (uint64_t)0xCD9E8D57u * x2;
        const uint32_t y0 = (uint32_t)(b >> 32) ^ x1 ^ k0;
        const uint32_t y2 = (uint32_t)(a >> 32) ^ x3 ^ k1;
        x1 = (uint32_t)b;
        x3 = (uint32_t)a;
        x0 = y0;
        x2 = y2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = x0;
    r[1] = x1;
    r[2] = x2;
    r[3] = x3;
}

// The mask's counter (c0, 0, c2, 0) under key (k0, k1).
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c2, uint32_t k0,
                                                       uint32_t k1, uint32_t (&r)[4]) {
    const uint32_t c[4] = {c0, 0u, c2, 0u}, k[2] = {k0, k1};
    philox4x32_10(c, k, r);
}

// Bit j: head 4 * quad + j of edge e is dropped.
__device__ __forceinline__ uint32_t drop_bits(const DropMask &dm, uint32_t e, uint32_t quad) {
    uint32_t r[4];
    philox4x32_10(e, quad, dm.key0, dm.key1, r);
    return (r[0] < dm.thr ? 1u : 0u) | (r[1] < dm.thr ? 2u : 0u) | (r[2] < dm.thr ? 4u : 0u) |
           (r[3] < dm.thr ? 8u : 0u);
}

}  // namespace maxk
