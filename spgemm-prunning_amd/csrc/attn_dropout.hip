// Elementwise attention dropout over head-major edge weights for gfx950:
//
//   out[h, e] = w[h, e] * d_he        d_he = the mask of attn_dropout.h, 0 or scale
//
// One thread per (edge, quad of heads): one Philox evaluation gives the four heads' draws, the
// loads and stores of a head are coalesced over the edges.  out may be w.  It serves the stored
// path's forward (alpha), its backward (grad_alpha) and the rebuilt backward of the fused path
// (the rebuilt alpha and grad_alpha): the same call on each, the mask recomputed every time.
#include "attn_dropout.h"

namespace maxk {
namespace {

__global__ __launch_bounds__(kBlock) void edge_dropout_heads_kernel(
    const float *__restrict__ w, float *__restrict__ out, int H, int64_t num_e, DropMask dm) {
    const int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (e >= num_e) return;
    const int quad = blockIdx.y;
    const uint32_t bits = drop_bits(dm, (uint32_t)e, (uint32_t)quad);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int h = quad * 4 + j;
        if (h < H) {
            const int64_t o = (int64_t)h * num_e + e;
            out[o] = w[o] * ((bits >> j) & 1u ? 0.f : dm.scale);
        }
    }
}

}  // namespace
}  // namespace maxk

using namespace maxk;

extern "C" int maxk_edge_dropout_heads(const float *w, float *out, int32_t num_heads,
                                       int64_t num_e, float p, uint64_t seed, void *stream) {
    clear_error();
    MAXK_REQUIRE(num_heads >= 1 && num_heads <= MAXK_MAX_HEADS,
                 "num_heads must be in [1,%d], got %d", MAXK_MAX_HEADS, num_heads);
    MAXK_REQUIRE(num_e >= 0 && num_e < (1LL << 31), "num_e out of range: %lld", (long long)num_e);
    if (int rc = check_dropout(p)) return rc;
    if (num_e == 0) return MAXK_OK;  // no edge, nothing to write
    MAXK_REQUIRE(w && out, "w / out must not be NULL");
    MAXK_REQUIRE(((uintptr_t)w & 3) == 0 && ((uintptr_t)out & 3) == 0,
                 "float buffers must be 4-B aligned");
    hipLaunchKernelGGL(edge_dropout_heads_kernel,
                       dim3((unsigned)ceil_div(num_e, kBlock), (unsigned)((num_heads + 3) / 4)),
                       dim3(kBlock), 0, as_stream(stream), w, out, num_heads, num_e,
                       drop_mask(p, seed));
    MAXK_LAUNCHED("edge_dropout_heads_kernel");
    return MAXK_OK;
}
