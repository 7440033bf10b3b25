// Library-level C ABI: version, per-thread error message, device probe.
#include <cstdarg>
#include <cstdio>

#include "common.h"
#include "spgemm_max.h"

namespace maxk {
namespace {
thread_local char g_err[512] = {0};
}

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

void clear_error() { g_err[0] = '\0'; }

__global__ void zero_words_kernel(uint32_t *__restrict__ p, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = 0u;
}

int zero_words(void *p, int64_t n, hipStream_t s) {
    if (n <= 0) return MAXK_OK;
    const int64_t blocks = ceil_div(n, kBlock);
    hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)),
                       dim3(kBlock), 0, s, reinterpret_cast<uint32_t *>(p), n);
    MAXK_LAUNCHED("zero_words_kernel");
    return MAXK_OK;
}

}  // namespace maxk

extern "C" int maxk_version(void) { return 100; }

#ifndef MAXK_SRC_DIGEST
#define MAXK_SRC_DIGEST "unknown"
#endif
extern "C" const char *maxk_source_digest(void) { return MAXK_SRC_DIGEST; }

// EXTRA_HIPFLAGS the library was built with ("" for the product build): every MAXK_* tuning
// or ablation macro set away from its default in common.h shows here.
#ifndef MAXK_BUILD_FLAGS
#define MAXK_BUILD_FLAGS "unknown"
#endif
extern "C" const char *maxk_build_config(void) { return MAXK_BUILD_FLAGS; }

extern "C" const char *maxk_last_error(void) { return maxk::g_err; }

extern "C" int maxk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

// ---- max aggregation (spgemm_max.hip) ----
extern "C" size_t maxk_spgemm_max_forward_workspace_size(int64_t num_rows, int64_t num_cols,
                                                         int64_t num_e, int32_t dim_origin,
                                                         int32_t dim_k, int32_t chunk_edges) {
    return maxk::max_forward_workspace_size(num_rows, num_cols, num_e, dim_origin, dim_k,
                                            chunk_edges);
}

extern "C" int maxk_spgemm_max_forward(const int32_t *row_ptr, const int32_t *col_idx,
                                       const float *cbsr_val, const uint8_t *cbsr_idx, float *out,
                                       int32_t *arg, int64_t num_rows, int64_t num_cols,
                                       int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                       int32_t chunk_edges, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    maxk::clear_error();
    return maxk::max_forward(row_ptr, col_idx, cbsr_val, cbsr_idx, out, arg, num_rows, num_cols,
                             num_e, dim_origin, dim_k, chunk_edges, workspace, workspace_bytes,
                             stream);
}

extern "C" size_t maxk_spgemm_max_backward_workspace_size(int64_t num_rows, int64_t num_cols,
                                                          int64_t num_e, int32_t dim_origin,
                                                          int32_t dim_k) {
    return maxk::max_backward_workspace_size(num_rows, num_cols, num_e, dim_origin, dim_k);
}

extern "C" int maxk_spgemm_max_backward(const int32_t *row_ptr, const int32_t *col_idx,
                                        const int32_t *col_ptr, const int32_t *csc_eid,
                                        const uint8_t *cbsr_idx, const int32_t *arg,
                                        const float *grad_out, float *grad_cbsr, int64_t num_rows,
                                        int64_t num_cols, int64_t num_e, int32_t dim_origin,
                                        int32_t dim_k, void *workspace, size_t workspace_bytes,
                                        void *stream) {
    maxk::clear_error();
    return maxk::max_backward(row_ptr, col_idx, col_ptr, csc_eid, cbsr_idx, arg, grad_out,
                              grad_cbsr, num_rows, num_cols, num_e, dim_origin, dim_k, workspace,
                              workspace_bytes, stream);
}
