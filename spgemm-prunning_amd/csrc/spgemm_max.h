// Max aggregation on CBSR features (spgemm_max.hip): the host entries behind the C ABI of
// capi.cpp.  Arguments as maxk_spgemm_max_forward / maxk_spgemm_max_backward in maxk_hip.h.
#pragma once

#include <cstddef>
#include <cstdint>

namespace maxk {

size_t max_forward_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e, int D, int k,
                                  int chunk);
int max_forward(const int32_t *row_ptr, const int32_t *col_idx, const float *cbsr_val,
                const uint8_t *cbsr_idx, float *out, int32_t *arg, int64_t num_rows,
                int64_t num_cols, int64_t num_e, int D, int k, int chunk, void *workspace,
                size_t workspace_bytes, void *stream);
size_t max_backward_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e, int D,
                                   int k);
int max_backward(const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr,
                 const int32_t *csc_eid, const uint8_t *cbsr_idx, const int32_t *arg,
                 const float *grad_out, float *grad_cbsr, int64_t num_rows, int64_t num_cols,
                 int64_t num_e, int D, int k, void *workspace, size_t workspace_bytes,
                 void *stream);

}  // namespace maxk
