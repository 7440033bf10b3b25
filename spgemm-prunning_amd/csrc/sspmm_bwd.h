// Backward outer-product sampled SpMM (SSpMM) for gfx950:
//   grad_cbsr[c, l] = sum_{e=(r->c)} val[e] * G[r, sel[c, l]] / row_div[r]
//
// Semantics: kernels/spmm_maxk_backward.cu:15-115 (push from the CSR of A, which
// yields the A^T product) and the /out_degrees of maxk_spgemm_function.py:154-155.
//
// Every edge needs the k values of its source row's G picked by its destination's
// selectors, summed per destination c.  Four forms of that sum, in three files that share
// only what this header holds:
//  * pull (sspmm_pull.hip, the default for k % 4 == 0 on dense graphs): the edges' values
//    are gathered straight from G / row_div; no per-edge contribution rows.
//  * atomic (sspmm_push.hip): the push, one global fp32 atomic per (edge, l).
//  * two-phase: phase 1 (the push) stores each edge's contribution row, then
//    - csc (sspmm_push.hip): per destination, the rows are gathered through the CSC
//      permutation and summed in a fixed order; bitwise deterministic;
//    - bsort (sspmm_bsort.hip): phase 1 writes each window of CSR edges' rows ordered by
//      destination bucket, and the rows are summed per bucket of destinations.
#pragma once

#include "common.h"

namespace maxk {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));  // a 16-B buffer store's data

// The argument checks every backward entry starts with.
inline int check_common(int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t D, int32_t k,
                        int32_t chunk) {
    MAXK_REQUIRE(num_rows >= 0 && num_rows < (1LL << 31), "num_rows out of range");
    MAXK_REQUIRE(num_cols >= 0 && num_cols < (1LL << 31), "num_cols out of range");
    MAXK_REQUIRE(num_e >= 0 && num_e < (1LL << 31), "num_e out of range");
    MAXK_REQUIRE(D >= 1 && D <= kMaxDim, "dim_origin must be in [1,256], got %d", D);
    MAXK_REQUIRE(k >= 1 && k <= D, "dim_k must be in [1,dim_origin], got %d", k);
    MAXK_REQUIRE(chunk >= 0, "chunk_edges must be >= 0");
    MAXK_REQUIRE(num_cols * (int64_t)k < (1LL << 31), "num_cols*k too large");
    return MAXK_OK;
}

// The csc phase 2 on its own (sspmm_push.hip), for a phase 1 that lives in another file (the
// fused attention backward): `ws` starts with the contribution rows T [num_e + 1, k] in CSR edge
// order (the last one the dummy row of masked lanes), which the caller has written; the rest of
// it is phase 2's slabs.  csc_sum_workspace_size: the bytes of `ws`, non-decreasing in num_e
// (the item count of the auto item size is not, so the slabs are sized by its largest).
// csc_sum_rows: grad_cbsr[c, :] = the sum of T[csc_eid[t], :] over column c's CSC slots t, in
// slot order, every row written; launches only.
size_t csc_sum_workspace_size(int64_t num_cols, int64_t num_e, int k, int chunk);
int csc_sum_rows(hipStream_t s, const int32_t *col_ptr, const int32_t *csc_eid, void *ws,
                 float *grad_cbsr, int64_t num_cols, int64_t num_e, int k, int chunk);

}  // namespace maxk
