// The token-stream work partition, stated once for every kernel that walks
// a CSR or a CSC by items: the forward (spgemm_fwd.hip), the push and the csc sum
// (sspmm_push.hip), the dense route's two walks (dense_route.hip), the edge-weight gradient
// (edge_grad.hip) and the multi-head forms of the first and the last (spgemm_fwd_heads.hip).
//
// A pointer array ptr[0..n] is read as a stream of n row tokens and num_e edge tokens: row q's
// token sits at q + ptr[q], edge e of row q at e + q + 1.  Item i is the tokens
// [i * chunk, (i + 1) * chunk), one wave each; a row is owned by the item holding its token.
// Which of a row's edges an item walks is one of two cut rules:
//
//   CutAtEnd    every piece is clipped to the item's tokens [d0, d1): an item walks exactly the
//               edges whose tokens it holds (the push, the csc sum, the edge-weight gradient);
//   CutHubRows  a row of at most `chunk` edges is walked whole by its owner, past d1; only a
//               longer (hub) row is clipped, and leaves a continuation -- and a slab for the
//               fixup -- in every later item it reaches.  An item then walks at most
//               2 * chunk tokens (the forward, both dense-route walks).
//
// The first part (item count, cut rules, the CutAtEnd item driver) is plain C++17 over integers
// and reads nothing but the pointer array: tests/partition_check.cpp includes this header alone
// and checks the rules, through the driver the kernels run, on the CPU.  The device part (item
// range, pointer window, row hand-out) is compiled by hipcc only.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include <type_traits>
#define MAXK_HD __host__ __device__ __forceinline__
#else
#define MAXK_HD inline
#endif

namespace maxk {

// Items of `chunk` tokens covering rows + num_e tokens; at least one (an empty graph still
// launches a wave that writes its slab_row).
inline int token_items(int64_t rows, int64_t num_e, int chunk) {
    const int64_t n = (rows + num_e + chunk - 1) / chunk;
    return (int)(n > 0 ? n : 1);
}

constexpr int kPtrWindow = 64;  // PtrWindow: one pointer entry per lane of a wave

struct CutAtEnd {};
struct CutHubRows {};

// Edges [sb, se) of one row, as an item walks them (empty when sb >= se).  hub (CutHubRows):
// the row is longer than an item and split at item ends; false under CutAtEnd.
struct RowPiece {
    int64_t sb, se;
    bool hub;
};

// Row q = [rb, re) is owned by the item ending at d1 (and at or past the one before it, which
// the callers know from the order they walk in): its token lies below d1.
MAXK_HD bool row_owned(int64_t d1, int q, int64_t rb) { return (int64_t)q + rb < d1; }

// The continuation of row r - 1 = [.., re) in the item ending at d1 whose first owned row is r:
// the row's token precedes the item, so its edges in the item start at the item's first token,
// edge p_lo = d0 - r (ItemRange).
MAXK_HD RowPiece cont_piece(CutAtEnd, int64_t p_lo, int64_t d1, int r, int64_t re) {
    return {p_lo, d1 - r < re ? d1 - r : re, false};
}
// ... of row r - 1 = [rb, re): only a hub row has one; a shorter row was walked by its owner.
MAXK_HD RowPiece cont_piece(CutHubRows, int64_t p_lo, int64_t d1, int r, int64_t rb, int64_t re,
                            int chunk) {
    return {p_lo, d1 - r < re ? d1 - r : re, re - rb > chunk};
}

// The piece of owned row q = [rb, re) in the item ending at d1 (row_owned(d1, q, rb)).
MAXK_HD RowPiece row_piece(CutAtEnd, int64_t d1, int q, int64_t rb, int64_t re) {
    return {rb, d1 - q - 1 < re ? d1 - q - 1 : re, false};
}
// Row q = [rb, re), continued or owned, in one form for a walk that treats both alike (the
// push): equal to cont_piece for q = r - 1 and to row_piece for an owned row.
MAXK_HD RowPiece any_piece(CutAtEnd, int64_t d0, int64_t d1, int q, int64_t rb, int64_t re) {
    return {d0 - q - 1 > rb ? d0 - q - 1 : rb, d1 - q - 1 < re ? d1 - q - 1 : re, false};
}
MAXK_HD RowPiece row_piece(CutHubRows, int64_t d1, int q, int64_t rb, int64_t re, int chunk) {
    const bool hub = re - rb > chunk;
    return {rb, hub && d1 - q - 1 < re ? d1 - q - 1 : re, hub};
}

// An item's tokens [d0, d1), its first owned row r (n when it owns none) and its first edge
// p_lo = d0 - r: the tokens before d0 hold r rows (item_range builds it on the device).
struct ItemRange {
    int64_t d0, d1;
    int r;
    int64_t p_lo;
};

// The CutAtEnd item driver: piece(q, sb, se, re, cont) for the edges [sb, se) of every row the
// item `it` of ptr[0..n] walks, re the row's end.  First the continuation of row r - 1 (cont: its
// token precedes the item), then the rows whose token the item holds, the last one cut at d1.
// Every piece is reported through one call site, so a walk is the same instructions for a
// continuation and an owned row; an empty piece is reported too (an owned row without edges has
// sb == re), and a caller with nothing to do for one skips it.  se == re: the piece ends its row.
template <class Piece>
MAXK_HD void walk_cut_item(const int32_t *ptr, int n, const ItemRange &it, Piece &&piece) {
    int q = it.r - 1;
    bool cont = true;
    int64_t re = 0;
    RowPiece p{0, 0, false};
    if (it.r > 0) {
        re = ptr[it.r];
        p = cont_piece(CutAtEnd{}, it.p_lo, it.d1, it.r, re);
    }
    for (;;) {
        if (q >= 0) piece(q, p.sb, p.se, re, cont);
        cont = false;
        ++q;
        if (q >= n) break;
        const int64_t rb = ptr[q];
        if (!row_owned(it.d1, q, rb)) break;  // row q's token belongs to a later item
        re = ptr[q + 1];
        p = row_piece(CutAtEnd{}, it.d1, q, rb, re);
    }
}

#if defined(__HIPCC__)

// Returns the first r in [0, n] whose token is >= d (ptr[n] + n >= d required).  64-ary search
// by the whole wave; the result is wave-uniform.
__device__ __forceinline__ int wave_first_row_token(const int32_t *__restrict__ row_ptr, int n,
                                                    int64_t d) {
    const int lane = __lane_id();
    int lo = 0, hi = n;  // answer in [lo, hi]
    while (hi - lo > 63) {
        const int step = (hi - lo + 62) / 63;  // lo + 63*step >= hi
        int p = lo + lane * step;
        p = p > hi ? hi : p;
        const uint64_t m = __ballot((int64_t)row_ptr[p] + p >= d);  // lane 63 probes hi: true
        const int f = __builtin_ctzll(m);
        if (f == 0) {
            hi = lo;
        } else {
            const int pf = lo + f * step;
            lo = lo + (f - 1) * step + 1;
            hi = pf > hi ? hi : pf;
        }
    }
    const int p = lo + lane;
    const int pc = p > hi ? hi : p;
    const uint64_t m = __ballot(p <= hi && (int64_t)row_ptr[pc] + pc >= d) | (1ull << 63);
    const int r = lo + __builtin_ctzll(m);
    return r > hi ? hi : r;
}

// One wave; every member of the result is wave-uniform.
__device__ __forceinline__ ItemRange item_range(const int32_t *__restrict__ ptr, int n,
                                                int64_t num_e, int item, int chunk) {
    const int64_t total = (int64_t)n + num_e;
    const int64_t d0 = (int64_t)item * chunk;
    const int64_t d1 = d0 + chunk < total ? d0 + chunk : total;
    const int r = wave_first_row_token(ptr, n, d0);
    return {d0, d1, r, d0 - r};
}

// ptr[wb .. wb + 64) of consecutive rows, one entry per lane (clamped to ptr[n]), read with
// readlane: a walk over rows pays one load per 63 rows instead of a dependent load per row.
struct PtrWindow {
    const int32_t *ptr;
    int n;
    int wb, v;  // v: this lane's entry, ptr[min(wb + lane, n)]
    __device__ __forceinline__ void load(int row, int lane) {
        wb = row;
        v = ptr[wb + lane <= n ? wb + lane : n];
    }
    // before reading begin(q) .. end(q + span - 1): true when the window moved (to start at q)
    __device__ __forceinline__ bool slide(int q, int lane, int span = 1) {
        if (q + span < wb + kPtrWindow) return false;
        load(q, lane);  // slide the window (wave-uniform)
        return true;
    }
    __device__ __forceinline__ int begin(int q) const {
        return __builtin_amdgcn_readlane(v, q - wb);
    }
    __device__ __forceinline__ int end(int q) const {
        return __builtin_amdgcn_readlane(v, q + 1 - wb);
    }
};

// The hand-out of an item's rows to the lane groups of its wave.  Rows are taken in order from
// `next` while the next one is owned by the item and the piece of it the rule gives the item
// holds at most lmax edges; the first row that is not stops the hand-out for good, and the
// caller walks it with the whole wave (next, wave-uniform: the first row not taken).  Under
// CutHubRows lmax must not exceed the item size, so a row the groups take is no hub and is
// handed out whole.
template <class Rule>
struct RowHandout {
    PtrWindow win;
    int64_t d1;
    int lmax;
    int next;
    bool stop;
    __device__ __forceinline__ RowHandout(const int32_t *__restrict__ ptr, int n, int first,
                                          int64_t d1_, int lmax_, int lane)
        : win{ptr, n, 0, 0}, d1(d1_), lmax(lmax_), next(first), stop(false) {
        win.load(first, lane);
    }
    // One round: every idle group (`idle`: this lane's group holds no row), in group order,
    // takes the next row; take(row, begin, end) runs in the lanes of the group that took it.
    // ng groups of lr lanes; g: this lane's group.  UNROLL: ng to unroll the group loop fully,
    // 1 to keep it rolled -- stated by the caller, not left to the compiler's size estimate:
    // past 8 groups the unrolled loop's window reads exhaust the SGPRs and spill.
    template <int UNROLL, class Take>
    __device__ __forceinline__ void assign(bool idle, int ng, int lr, int g, int lane,
                                           Take &&take) {
        const uint64_t m = __ballot(idle);
#pragma unroll UNROLL
        for (int gi = 0; gi < ng && !stop; ++gi) {
            if (!((m >> (gi * lr)) & 1ull)) continue;
            win.slide(next, lane);
            const int b = win.begin(next);
            int e = win.end(next);
            if constexpr (std::is_same_v<Rule, CutAtEnd>)
                e = (int)row_piece(CutAtEnd{}, d1, next, b, e).se;
            if (next < win.n && row_owned(d1, next, b) && e - b <= lmax) {
                if (g == gi) take(next, b, e);
                ++next;
            } else {
                stop = true;
            }
        }
    }
};

#endif  // __HIPCC__

}  // namespace maxk

#undef MAXK_HD
