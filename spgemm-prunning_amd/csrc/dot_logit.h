// The logit of the dot-product attention on CBSR keys, stated once for the walks that form it: both
// sweeps of the fused forward and the alpha entry (dot_attention_heads.hip) and the fused backward
// (dot_attention_heads_bwd.hip).  It is the record's dot product of piece_walk.h -- dot_term and
// lane_tree<KG, Sum> with one slot per lane, record_dots for k > 64 -- against the row scale * q
// that stage_query stages.  Every one of them calls those device functions on that same staged
// row, so a logit has the same bits wherever it is formed: the forward's row maximum is the exact
// maximum of what the alpha entry and the backward exponentiate, and exp(l - row_max) <= 1 holds
// in all of them.  With it the argument checks the entries share.
// Device code in an anonymous namespace (each translation unit instantiates what it launches).
#pragma once

#include <cmath>

#include "piece_walk.h"

namespace maxk {
namespace {

constexpr int kMaxH = MAXK_MAX_HEADS;

// qrow[h * DS + j] = scale * q[h, row, j] for the H heads (the pad columns [D, DS) hold zeros and
// are never staged over).  One wave.
__device__ __forceinline__ void stage_query(float *qrow, const float *__restrict__ q, int64_t row,
                                            int64_t num_rows, int H, int D, int DS, float scale,
                                            bool vec, int lane) {
    for (int h = 0; h < H; ++h) {
        const float *g = q + ((int64_t)h * num_rows + row) * D;
        float *d = qrow + h * DS;
        if (vec) {
            for (int j = lane * 4; j < D; j += kWave * 4) {
                float4 x = *reinterpret_cast<const float4 *>(&g[j]);
                x.x *= scale;
                x.y *= scale;
                x.z *= scale;
                x.w *= scale;
                *reinterpret_cast<float4 *>(&d[j]) = x;
            }
        } else {
            for (int j = lane; j < D; j += kWave) d[j] = g[j] * scale;
        }
    }
}

inline bool dot_shape_ok(int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin,
                         int32_t dim_k, int32_t num_heads, int32_t chunk_edges) {
    return sizes_ok(num_rows, num_cols, num_e) && dim_origin >= 1 && dim_origin <= kMaxDim &&
           dim_k >= 1 && dim_k <= dim_origin && chunk_edges >= 0 && num_heads >= 1 &&
           num_heads <= MAXK_MAX_HEADS;
}

// The argument checks the entries share, in the order the header states them.
inline int check_dot(int64_t num_rows, int64_t num_cols, int64_t num_e, float scale,
                     int32_t dim_origin, int32_t dim_k, int32_t num_heads, int32_t chunk_edges) {
    if (int rc = check_heads(num_heads)) return rc;
    if (int rc = check_sizes(num_rows, num_cols, num_e, chunk_edges)) return rc;
    MAXK_REQUIRE(std::isfinite(scale) && scale > 0.f, "scale must be finite and > 0, got %g",
                 (double)scale);
    return check_cbsr_dims(dim_origin, dim_k, num_cols);
}

}  // namespace
}  // namespace maxk
