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

// ---- the forward walks' mask: once in S wave steps ---------------------------------------------
// A pass of the hub-row heads walk (heads_walk.h) holds EU = EP * U edges per wave step, and its
// heads lie in qp <= 2 quads.  One Philox evaluation per lane -- lane t on the edge at offset
// t % span of the next S = 64 / (EU * qp) steps (span = S * EU; its CSR position is the piece's
// first edge + its index in the piece) and the quad q0 + t / span -- serves S steps: four
// ballots, one per head of a quad, carry the bits, and each group keeps its head's 64 (`mine`).
// The caller's sum of p takes the unmasked weights and its products p * keep (0 or 1): a dropped
// NaN or Inf stays NaN.
struct DropPass {
    int q0, qp, head;  // the pass's first quad of heads and their number; the group's head
};
// The pass over the heads h0 .. min(h0 + HC, H), seen from the group of `head`.
__device__ __forceinline__ DropPass drop_pass(int h0, int HC, int H, int head) {
    return DropPass{h0 >> 2, ((min(h0 + HC, H) - 1) >> 2) - (h0 >> 2) + 1, head};
}
template <bool DROP>
struct PassMask {  // without a mask: nothing
    __device__ __forceinline__ PassMask(const DropPass &, int) {}
    __device__ __forceinline__ void refresh(const NoMask &, const DropPass &, int, int) {}
    __device__ __forceinline__ void next() {}
};
template <>
struct PassMask<true> {
    int EU, S, span_log, js = 0, qsel;
    uint64_t mine = 0;
    __device__ __forceinline__ PassMask(const DropPass &dp, int EU_) : EU(EU_) {
        S = kWave / (EU * dp.qp);  // powers of two, EU * qp <= 64
        span_log = 31 - __clz(S * EU);
        qsel = min(max((dp.head >> 2) - dp.q0, 0), dp.qp - 1);
    }
    // Before the wave step whose first edge has the CSR position e0: every S-th step evaluates
    // the masks of itself and the next S - 1 (js, S: wave-uniform).
    __device__ __forceinline__ void refresh(const DropMask &dm, const DropPass &dp, int e0,
                                            int lane) {
        if (js == 0) {
            const uint32_t bits = drop_bits(dm, (uint32_t)(e0 + (lane & ((1 << span_log) - 1))),
                                            (uint32_t)(dp.q0 + (lane >> span_log)));
            const uint64_t b0 = __ballot(bits & 1u), b1 = __ballot(bits & 2u),
                           b2 = __ballot(bits & 4u), b3 = __ballot(bits & 8u);
            const int hb = dp.head & 3;
            mine = (hb == 0 ? b0 : hb == 1 ? b1 : hb == 2 ? b2 : b3) >> (qsel << span_log);
        }
    }
    // 0 where the group's head of the step's edge slot (u * EP + eg) is dropped, else 1.
    __device__ __forceinline__ float keep(int slot) const {
        return (mine >> (js * EU + slot)) & 1 ? 0.f : 1.f;
    }
    __device__ __forceinline__ void next() { js = js + 1 == S ? 0 : js + 1; }
};

// ---- the backward walks' mask: every wave step -------------------------------------------------
// A backward walk (piece_walk.h) has KG lanes per edge, lane h < HP of a group holding head h of
// the group's U edges of a step.  Lane j < U * QP of a group evaluates the mask of the group's
// edge j % U for the quad of heads j / U, QP = ceil(HP / 4) quads; lane h fetches its head's bit
// with one shuffle per edge.  Returns, in lane h, bit u: head h of the group's edge u -- CSR
// position e0 + u * G + grp, e0 the step's first edge -- is dropped.  0 without a mask.  grp, l0,
// lane0: the lane's group, its place in it and the group's first lane.
template <int KG, int HP, int U, bool DROP>
__device__ __forceinline__ uint32_t step_gone(const MaskArg<DROP> &dm, int e0, int grp, int l0,
                                              int lane0) {
    uint32_t gone = 0u;
    if constexpr (DROP) {
        constexpr int G = kWave / KG, QP = (HP + 3) / 4;
        static_assert(U * QP <= KG, "a group evaluates its step's masks in one round");
        const uint32_t bits =
            drop_bits(dm, (uint32_t)(e0 + (l0 % U) * G + grp), (uint32_t)((l0 / U) % QP));
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t b = __shfl(bits, lane0 + ((l0 >> 2) % QP) * U + u);
            gone |= ((b >> (l0 & 3)) & 1u) << u;
        }
    }
    return gone;
}

// ---- host: the entries' dispatch ----------------------------------------------------------------
// f(const_t<HP>{}, mask) for the padded head count hp (2, 4 or 8), mask = *dm, or NoMask{} where
// dm is null; returns what f returns.  In f, is_drop_v<decltype(mask)> is the DROP of MaskArg.
template <class M>
constexpr bool is_drop_v = std::is_same_v<std::decay_t<M>, DropMask>;
template <class F>
int with_heads_mask(int hp, const DropMask *dm, F &&f) {
    int rc = MAXK_ERR_INVALID;
    const bool ok = with_const<2, 4, 8>(hp, [&](auto hp_c) {
        rc = dm ? f(hp_c, *dm) : f(hp_c, NoMask{});
    });
    if (!ok) set_error("unsupported padded head count %d", hp);
    return rc;
}
// f(dm) for a dropout entry's (p, seed): dm null at p == 0, which drops nothing and scales by 1
// -- the kernels of the entry without dropout.
template <class F>
int with_dropout(float p, uint64_t seed, F &&f) {
    if (int rc = check_dropout(p)) return rc;
    const DropMask dm = drop_mask(p, seed);
    return f(p > 0.f ? &dm : nullptr);
}

}  // namespace maxk
