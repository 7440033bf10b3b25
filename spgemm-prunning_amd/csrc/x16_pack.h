// What the x16 kernels share (x16_topk.hip, x16_fwd.hip, x16_bwd.hip, x16_heads.hip): the shape
// range of the 16-bit-selector path, its packed record (packed by x16_fwd.hip's x16_pack_kernel,
// launched through launch_x16_pack), the LDS row stride and the item size rule.  DESIGN.md 5.20.
//
// Record of one source vertex: [k f32 values | k u16 columns | pad], RS bytes.  The u16 is the LDS
// column the walker accumulates into: the selector itself when it is kept, else the trash column
// DS - 1 = the padded D + 3 (x16_copy_stride).  The u8 record (cbsr_pack.h) marks a trash slot
// with bit 0x100 of the u16; with up to 1024 columns that bit is part of a real column index, so
// the marker here is a column no selector can name.  As there, a repeated selector's first
// occurrence carries the sum of its values in l order and the later ones go to trash with value
// 0, which makes the walker's non-atomic LDS accumulation exact for any input; selectors >= D go
// to trash too.
#pragma once

#include "common.h"

namespace maxk {

constexpr int kMaxDimX16 = 1024;  // columns a 16-bit-selector row may have
constexpr int kMaxKX16 = 256;     // winners per row: the top-k's LDS slots, csc_sum_rows' widest row

// The argument rule of every x16 entry.
inline int x16_check_dims(int32_t D, int32_t k) {
    MAXK_REQUIRE(D >= 1 && D <= kMaxDimX16, "dim_origin must be in [1,1024], got %d", D);
    MAXK_REQUIRE(k >= 1 && k <= D && k <= kMaxKX16,
                 "dim_k must be in [1,min(dim_origin,256)], got %d (dim_origin %d)", k, D);
    return MAXK_OK;
}
inline bool x16_dims_ok(int32_t D, int32_t k) {
    return D >= 1 && D <= kMaxDimX16 && k >= 1 && k <= D && k <= kMaxKX16;
}

// LDS row stride of a D-column row: D padded to 16 B, plus one 16-B group whose last float is
// the trash column (never read by a flush).  At most 1028.
inline int x16_copy_stride(int D) { return ((D + 3) / 4) * 4 + 4; }

// Record stride: a power-of-two slot while the record fits a 128-B line, else whole 64-B sectors.
inline int x16_record_stride(int k) {
    const int b = 6 * k;
    if (b <= 128) {
        int s = 16;
        while (s < b) s <<= 1;
        return s;
    }
    return (b + 63) / 64 * 64;
}

// Lanes per edge: pow2ceil(k) within [lo, 64]; past 64 slots a lane takes several.
inline int x16_lanes(int k, int lo) {
    int g = lo;
    while (g < k && g < kWave) g <<= 1;
    return g;
}

// x16_pack_kernel (x16_fwd.hip) on the stream: rec[v] = vertex v's record, num_cols > 0.
int launch_x16_pack(const float *cbsr_val, const uint16_t *cbsr_idx, uint8_t *rec, int64_t num_cols,
                    int k, int RS, int D, int trash, hipStream_t s);

// Dense rows of DS floats a wave stages side by side in the budget of the forward's copies, about
// 8 KB: 2 at D = 1024, 4 at D = 508, more for narrower rows, at most MAXK_MAX_HEADS (x16_heads.hip).
inline int x16_rows_in_budget(int DS) {
    const int n = 2056 / DS;
    return n < 2 ? 2 : (n > MAXK_MAX_HEADS ? MAXK_MAX_HEADS : n);
}

// Auto item size: about eight items per resident wave slot (16 slots per CU assumed: the LDS
// rows of a wave are ~8 KB), within [64, 2048] tokens.
constexpr int64_t kX16ItemsPerCu = 16 * 8;
inline int x16_chunk(int64_t rows, int64_t num_e, int32_t chunk) {
    if (chunk > 0) return chunk;
    const int64_t c = ceil_div(rows + num_e, device_cus() * kX16ItemsPerCu);
    return (int)(c < 64 ? 64 : (c > 2048 ? 2048 : c));
}
// Items to size per-item buffers for: at least the item count, and non-decreasing in the token
// count, which the item count of the auto rule is not (one more token can make the items longer
// and fewer).  The auto items hold at least 64 tokens, and at least tokens / (items per CU * CUs)
// until they reach 2048.
inline int64_t x16_item_cap(int64_t tokens, int chunk, int n_items) {
    if (chunk > 0) return n_items;
    const int64_t a = ceil_div(tokens, 64), b = device_cus() * kX16ItemsPerCu;
    const int64_t lo = a < b ? a : b, hi = ceil_div(tokens, 2048);
    const int64_t cap = lo > hi ? lo : hi;
    return cap > n_items ? cap : n_items;
}

}  // namespace maxk
