/*
 * maxk_hip.h -- C ABI of the MI355X-native MaxK-GNN aggregation hot path
 * (libmaxk_hip.so, built from spgemm-prunning_amd/csrc for gfx950).
 *
 * Plain pointers and sizes only.  Every device pointer is caller-owned device
 * memory; every launch goes on the caller's stream (a hipStream_t passed as
 * void*; NULL = the default stream).  Launch functions never allocate, copy to
 * the host or synchronise, so they can be captured into a hipGraph; the setup
 * helpers marked "synchronous" do.
 *
 * Return value: MAXK_OK (0) or a negative MAXK_ERR_*; maxk_last_error() then
 * holds a message for the calling thread.
 *
 * Layouts (all row-major, C-contiguous):
 *   CSR     row_ptr int32 [num_rows+1], col_idx int32 [num_e] (< num_cols),
 *           edge_val f32 [num_e]
 *   CBSR    cbsr_val f32 [num_cols, k], cbsr_idx u8 [num_cols, k] (< dim_origin)
 *   dense   f32 [rows, dim_origin]
 *   warp4   int32 [W, 4] = (row, loc, len, 0)
 * Limits: 1 <= k <= dim_origin <= 256 (the selector is uint8).
 *
 * Numerics (tests/numerics.py, tests/test_numerics_gpu.py): every element of the forward and
 * of the backward matches exact arithmetic to within (n + 8) * 2^-24 * sum|terms|, n its number
 * of addends (edges times repeated selectors, plus one for an accumulate prefill) -- at any
 * magnitude, fp32 subnormals included, not only near 1; an element without addends is exactly
 * 0.  Inf and NaN in cbsr_val and grad_out propagate as the IEEE sum of the selected terms:
 * terms behind skipped, repeated or out-of-range selectors follow the same rule as finite
 * values (a NaN behind a selector >= dim_origin or in a vertex no edge reads reaches nothing),
 * and any NaN bit pattern is handled, the transport records' own skip marker included.
 * Non-finite edge weights or row_div are outside the contract (the dense route multiplies
 * unselected zeros by the weight).  The forward (every form), the csc and dense backwards and
 * the edge-weight gradient sum in a fixed order: bitwise repeatable, and bitwise equivariant under a power-of-two scale
 * of the values away from overflow and underflow.
 *
 * Memory (tests/memguard.py, tests/test_memguard_gpu.py): a workspace, a plan buffer and an
 * output may hold anything when a call starts -- zeros, 0xFF bytes, what an earlier call left
 * there -- and nothing needs zero-initialising by the caller; the result does not depend on it
 * (bitwise, where the sum order is fixed).  A workspace of exactly the documented size (the
 * call's *_workspace_size query; 8 bytes for maxk_pull_locality; 0, so NULL, for the atomic
 * maxk_sspmm_backward) is sufficient, and it is required: a shorter one is rejected with
 * MAXK_ERR_INVALID ("workspace too small") on the host, before anything is launched or written.
 * Outputs are fully written (an accumulate form's `out` fully updated), inputs are never
 * written (except where an output is documented to alias one: maxk_topk_backward's grad_x ==
 * grad_dense), and nothing is written outside the buffers passed, not by a byte.
 */
#ifndef MAXK_HIP_H_
#define MAXK_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAXK_OK 0
#define MAXK_ERR_INVALID (-1)  /* bad argument (shape, null pointer, k/D range, workspace) */
#define MAXK_ERR_HIP (-2)      /* a HIP runtime call or launch failed */
#define MAXK_ERR_NODEVICE (-3) /* no HIP device visible */
#define MAXK_ERR_LIBRARY (-4)  /* rocSPARSE failure (baseline only) */

/* ABI version (major*100 + minor). */
int maxk_version(void);

/* Message for the last failing call on this thread ("" if none). */
const char *maxk_last_error(void);

/* Number of visible HIP devices (0 without a GPU; never fails). */
int maxk_device_count(void);

/* First 16 hex digits of the SHA-256 of the sources this library was built from
 * (spgemm-prunning_amd/Makefile: the .hip, .cpp and .h files of csrc and this header, in
 * C-locale path order), so a test can tell a stale binary from one built from the tree. */
const char *maxk_source_digest(void);

/* The extra compiler flags (EXTRA_HIPFLAGS: MAXK_* tuning / ablation macros) this library was
 * built with; "" for the product build.  The digest above covers them too. */
const char *maxk_build_config(void);

/* ---------------------------------------------------------------------------
 * Forward row-wise-product SpGEMM:  out = diag(1/row_div) . A . scatter(cbsr)
 *   out[r, cbsr_idx[c,l]] += edge_val[e] * cbsr_val[c,l]   (e in row r, c = col_idx[e])
 * Every output row is written (rows without edges get zeros): no zero-init of
 * `out` is needed.  row_div may be NULL (no normalisation).  Duplicate
 * selectors within a CBSR row accumulate; selectors >= dim_origin are ignored.
 * Replaces: spmm_kernel_opt2_sparse_v3 (kernels/spmm_maxk.cu:17-106),
 *           its launcher spmm_kernel_opt2_sparse_v3_wrapper
 *           (cuda_kernel_wrappers.cu:38-56) and the /in_degrees of
 *           maxk_spgemm_function.py:85-86.
 * chunk_edges: tokens (rows + edges) per wavefront work item (0 = auto: about 8 items per
 *              resident wave slot in [256, 2048], or on a smaller graph all items resident
 *              in one round, down to 64).
 * workspace: >= maxk_spgemm_forward_workspace_size(...) bytes, 256-B aligned
 *            (packed CBSR records + split-row slabs).
 * ------------------------------------------------------------------------- */
size_t maxk_spgemm_forward_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e,
                                          int32_t dim_origin, int32_t dim_k, int32_t chunk_edges);
int maxk_spgemm_forward(const int32_t *row_ptr, const int32_t *col_idx, const float *edge_val,
                        const float *cbsr_val, const uint8_t *cbsr_idx, const float *row_div,
                        float *out, int64_t num_rows, int64_t num_cols, int64_t num_e,
                        int32_t dim_origin, int32_t dim_k, int32_t chunk_edges,
                        void *workspace, size_t workspace_bytes, void *stream);
/* The same forward, also writing each edge's selectors: edge_sel[e, l] = cbsr_idx[col_idx[e], l]
 * (u8 [num_e, k]), the stream maxk_sspmm_backward_csc_sel reads.  The forward gathers every
 * edge's CBSR record anyway, so the stream costs one coalesced write of num_e * k bytes
 * (tables past 2^24 columns or 4 GiB of records: a separate gather, maxk_edge_selectors). */
int maxk_spgemm_forward_sel(const int32_t *row_ptr, const int32_t *col_idx, const float *edge_val,
                            const float *cbsr_val, const uint8_t *cbsr_idx, const float *row_div,
                            float *out, int64_t num_rows, int64_t num_cols, int64_t num_e,
                            int32_t dim_origin, int32_t dim_k, int32_t chunk_edges,
                            void *workspace, size_t workspace_bytes, void *stream,
                            uint8_t *edge_sel);
/* The same product added onto out (out += ...; out must hold valid values): a row range's
 * result summed over several column ranges of A, e.g. the sharded forward's pipelined halves
 * (maxk_dist.py), without a separate pass over out.  Same arguments and workspace. */
int maxk_spgemm_forward_accumulate(const int32_t *row_ptr, const int32_t *col_idx,
                                   const float *edge_val, const float *cbsr_val,
                                   const uint8_t *cbsr_idx, const float *row_div, float *out,
                                   int64_t num_rows, int64_t num_cols, int64_t num_e,
                                   int32_t dim_origin, int32_t dim_k, int32_t chunk_edges,
                                   void *workspace, size_t workspace_bytes, void *stream);
/* Both: the product added onto out and the edge-selector stream written (the sharded forward's
 * later pipelined parts, whose backward reads their own part's stream). */
int maxk_spgemm_forward_accumulate_sel(const int32_t *row_ptr, const int32_t *col_idx,
                                       const float *edge_val, const float *cbsr_val,
                                       const uint8_t *cbsr_idx, const float *row_div, float *out,
                                       int64_t num_rows, int64_t num_cols, int64_t num_e,
                                       int32_t dim_origin, int32_t dim_k, int32_t chunk_edges,
                                       void *workspace, size_t workspace_bytes, void *stream,
                                       uint8_t *edge_sel);
/* Transport records (the sharded forward, r05): [k f32 | k u8] per vertex at a stride of 5k bytes,
 * the bytes a vertex-range shard all-gathers anyway, built by each owner for its own rows
 * (maxk_cbsr_records) so the receivers walk the gathered buffer (maxk_spgemm_forward_records)
 * with no record pack over every gathered vertex.  Selectors stay the caller's bytes; a repeated
 * selector's first occurrence carries the sum of its values in l order and the later ones, like
 * selectors >= dim_origin, a skip marker (a NaN payload; a kept NaN value is stored as the
 * canonical quiet NaN) -- the same sums as maxk_spgemm_forward.  maxk_records_ok says whether
 * the records forward applies: the streaming walker of a sparse graph (average degree < 128) or
 * the deep-batch walker of a dense one, dim_k % 4 == 0 in [24, 32], num_cols * 5 * dim_k < 2^32 (where the 5k-byte stride costs no
 * extra line per gather against the packed record).  rec 4-B aligned; workspace as
 * maxk_spgemm_forward_workspace_size; accumulate adds onto out.  Replaces the same reference
 * kernel as maxk_spgemm_forward (spmm_maxk.cu:17-113). */
int maxk_records_ok(int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin,
                    int32_t dim_k);
int maxk_cbsr_records(const float *cbsr_val, const uint8_t *cbsr_idx, uint8_t *rec,
                      int64_t num_rows, int32_t dim_origin, int32_t dim_k, void *stream);
int maxk_spgemm_forward_records(const int32_t *row_ptr, const int32_t *col_idx,
                                const float *edge_val, const uint8_t *rec, const float *row_div,
                                float *out, int64_t num_rows, int64_t num_cols, int64_t num_e,
                                int32_t dim_origin, int32_t dim_k, int32_t chunk_edges,
                                void *workspace, size_t workspace_bytes, void *stream,
                                int32_t accumulate);

/* ---------------------------------------------------------------------------
 * Gradient of the forward with respect to the edge weights (an SDDMM sampled by the CBSR):
 *   grad_edge[e] = ( sum_l cbsr_val[c,l] * grad_out[r, cbsr_idx[c,l]] ) / row_div[r]
 *                  r = the CSR row holding e, c = col_idx[e]
 * the adjoint of out = diag(1/row_div) . A . scatter(cbsr) in edge_val, which it does not read.
 * The reference has no counterpart (its autograd returns no gradient for the edge weights).
 * One packed record gathered per edge, as in the forward; no atomics.
 * Shapes: any 1 <= dim_k <= dim_origin <= 256 (dim_k % 4 != 0, odd dim_origin, and the pairs
 *   where the forward takes its dense route: this function has no such route), any alignment
 *   of grad_out and cbsr_* the plain forward accepts; row_div may be NULL; num_e == 0 launches
 *   nothing and succeeds.
 * Numerics, in the words of the top comment: every element is within (n + 8) * 2^-24 *
 *   sum|terms| of exact arithmetic (plus the (n + 8) * 2^-149 floor for subnormal inputs), n
 *   the number of column c's selectors below dim_origin; an edge with n = 0 gets exactly 0.
 *   Inf and NaN in cbsr_val and grad_out propagate as the IEEE sum of the selected terms; a NaN
 *   behind a selector >= dim_origin, or in a column of grad_out the vertex does not select,
 *   reaches nothing.  Repeated selectors are summed (their values first, as the forward's pack
 *   folds them): for them only the finite bound is promised.  The sum order is fixed: bitwise
 *   repeatable, and bitwise equivariant under a power-of-two scale of cbsr_val or grad_out away
 *   from overflow and underflow.
 * Memory, as the top comment: the workspace (the packed records) is exactly the queried size,
 *   256-B aligned, and may hold anything; a shorter one is rejected with MAXK_ERR_INVALID
 *   ("workspace too small") on the host before anything is launched; grad_edge [num_e] is fully
 *   written, in CSR order; inputs are never written; nothing else is touched.
 * Argument errors (null pointer, k / D range, negative sizes): MAXK_ERR_INVALID with a message.
 * chunk_edges: tokens per wavefront work item, 0 = the forward's auto rule.
 * ------------------------------------------------------------------------- */
size_t maxk_edge_weight_grad_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e,
                                            int32_t dim_origin, int32_t dim_k,
                                            int32_t chunk_edges);
int maxk_edge_weight_grad(const int32_t *row_ptr, const int32_t *col_idx, const float *cbsr_val,
                          const uint8_t *cbsr_idx, const float *grad_out, const float *row_div,
                          float *grad_edge, int64_t num_rows, int64_t num_cols, int64_t num_e,
                          int32_t dim_origin, int32_t dim_k, int32_t chunk_edges,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Multi-head aggregation: H = num_heads forwards, and their edge-weight gradients, over one
 * graph and one CBSR, differing only in the edge weights -- the attention heads of a GAT.  One
 * packed record is gathered per edge and serves every head, where H single-head calls gather it
 * H times.  The reference has no counterpart (it has no attention at all).
 * Layout, head-major, so every head's slice is a contiguous array the single-head entries take:
 *   edge_val, grad_edge  f32 [num_heads, num_e], CSR order inside a head;
 *   out, grad_out        f32 [num_heads, num_rows, dim_origin];
 *   row_div              f32 [num_rows] shared by the heads, or NULL.
 * 1 <= num_heads <= MAXK_MAX_HEADS, any value in the range.
 * ------------------------------------------------------------------------- */
#define MAXK_MAX_HEADS 8

/* out[h, r, cbsr_idx[c,l]] += edge_val[h, e] * cbsr_val[c,l] / row_div[r]   for every head h
 * (e in row r, c = col_idx[e]): maxk_spgemm_forward per head.  The reference has no counterpart.
 * Every output row of every head is written (rows without edges get zeros; num_e == 0 writes
 * zeros to all of out): no zero-init of out is needed.  No global and no LDS atomics; a hub row
 * cut over work items is merged from per-item partials in item order.
 * Shapes: any 1 <= dim_k <= dim_origin <= 256 (dim_k % 4 != 0, odd dim_origin, dim_k > 64).
 *   There is no dense route and no _sel / _accumulate / records form; a table past 2^24 columns
 *   or 4 GiB of packed records is rejected with MAXK_ERR_INVALID.
 * Numerics, in the words of the top comment: every element is within (n + 8) * 2^-24 *
 *   sum|terms| of exact arithmetic (plus the subnormal floor); the sum order is fixed by the
 *   graph, chunk_edges, dim_k and num_heads, so the result is bitwise repeatable; the slice of
 *   head h holds only products with head h's weights and does not depend, bitwise, on the other
 *   heads' weights; Inf and NaN in cbsr_val propagate per head as in maxk_spgemm_forward.
 * Memory, as the top comment: the workspace (packed records, per-head split-row slabs) is
 *   exactly the queried size, 256-B aligned, and may hold anything; a shorter one is rejected
 *   ("workspace too small") on the host before any launch; nothing is written outside out and
 *   the workspace.
 * Argument errors (num_heads outside [1, MAXK_MAX_HEADS], a null pointer, k / D range, negative
 *   sizes): MAXK_ERR_INVALID with a message naming the argument, before any launch.
 * chunk_edges: tokens per wavefront work item, 0 = the forward's auto rule. */
size_t maxk_spgemm_forward_heads_workspace_size(int64_t num_rows, int64_t num_cols,
                                                int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                                int32_t num_heads, int32_t chunk_edges);
int maxk_spgemm_forward_heads(const int32_t *row_ptr, const int32_t *col_idx,
                              const float *edge_val, const float *cbsr_val,
                              const uint8_t *cbsr_idx, const float *row_div, float *out,
                              int64_t num_rows, int64_t num_cols, int64_t num_e,
                              int32_t dim_origin, int32_t dim_k, int32_t num_heads,
                              int32_t chunk_edges, void *workspace, size_t workspace_bytes,
                              void *stream);

/* grad_edge[h, e] = ( sum_l cbsr_val[c,l] * grad_out[h, r, cbsr_idx[c,l]] ) / row_div[r]   for
 * every head h: maxk_edge_weight_grad per head, the adjoint of maxk_spgemm_forward_heads in
 * edge_val.  The reference has no counterpart.  Per row piece the H rows grad_out[h, r, :] are
 * staged in LDS; per edge one record load, then one fma and one fixed-shape sum per head.
 * Shapes, numerics and memory are maxk_edge_weight_grad's, per head (the same tree in the same
 *   order: at num_heads == 1 the result equals maxk_edge_weight_grad's bitwise), except that a
 *   table past 2^24 columns or 4 GiB of packed records is rejected with MAXK_ERR_INVALID.
 *   num_e == 0 launches nothing and succeeds.  grad_edge [num_heads, num_e] is fully written.
 * Argument errors as maxk_spgemm_forward_heads. */
size_t maxk_edge_weight_grad_heads_workspace_size(int64_t num_rows, int64_t num_cols,
                                                  int64_t num_e, int32_t dim_origin,
                                                  int32_t dim_k, int32_t num_heads,
                                                  int32_t chunk_edges);
int maxk_edge_weight_grad_heads(const int32_t *row_ptr, const int32_t *col_idx,
                                const float *cbsr_val, const uint8_t *cbsr_idx,
                                const float *grad_out, const float *row_div, float *grad_edge,
                                int64_t num_rows, int64_t num_cols, int64_t num_e,
                                int32_t dim_origin, int32_t dim_k, int32_t num_heads,
                                int32_t chunk_edges, void *workspace, size_t workspace_bytes,
                                void *stream);

/* ---------------------------------------------------------------------------
 * Edge softmax: the weights of a destination's incoming edges, normalised over its CSR row,
 * and their backward -- what produces the edge weights maxk_spgemm_forward takes and consumes
 * the gradient maxk_edge_weight_grad returns.  The reference has no counterpart.
 * Edge e lies in CSR row r, c = col_idx[e].
 *   GAT form      z_e = s_dst[r] + s_src[c],  l_e = z_e > 0 ? z_e : negative_slope * z_e
 *   plain form    l_e = logits[e]
 *   forward       w_e = exp(l_e - m_r) / sum_{j in r} exp(l_j - m_r),  m_r = max_{j in r} l_j
 *   backward      t_r = sum_{e in r} w_e * grad_w_e,   gl_e = w_e * (grad_w_e - t_r)
 *                 plain form: grad_logits[e] = gl_e
 *                 GAT form:   gz_e = gl_e * (z_e > 0 ? 1 : negative_slope), z recomputed from
 *                             the scores; grad_s_dst[r] = sum_{e in r} gz_e;
 *                             grad_s_src[c] = sum_{e: col_idx[e] = c} gz_e, through the graph's
 *                             transpose plan (col_ptr, csc_eid) in CSC slot order
 * s_dst f32 [num_rows], s_src f32 [num_cols], logits / w / grad_w / grad_logits f32 [num_e] in
 * CSR order; negative_slope in [0, 1].  The plain form reads no column, num_cols only has to be
 * >= 0.  num_e < 2^31, any num_rows and num_cols; num_e == 0 launches nothing and succeeds (the
 * GAT backward then writes zeros to both gradients).
 * Work partition: token-stream items of chunk_edges tokens, one wavefront each; a row cut over
 *   items is merged from per-item partials in item order, so a hub row costs no wave more than
 *   one item.  chunk_edges: 0 = the forward's auto rule for large graphs, about 8 items per
 *   resident wave slot in [256, 2048] tokens.
 * Numerics (tests/edge_softmax_ref.py; u = 2^-24, n_r the row's degree, A_r = max_e |z_e| or
 *   max_e |logits[e]|):
 *     |w - exact| <= (n_r + 16 + 16 A_r) * u * exact + (n_r + 16) * 2^-149
 *   (the exponent's argument is rounded three times, each at most 2 A_r u; exp is good to a
 *   few ulp; n_r terms; one division; the floor covers weights that underflow), gl within
 *   (n_r + 8) * u * |w_e| * (|grad_w_e| + sum_j |w_j grad_w_j|) plus w's own bound carried
 *   through, and each score gradient within (n + 8) * u * sum|terms| on top of its terms'
 *   bounds, n its number of addends; an element without addends (a row without edges, a
 *   column no edge reads) is exactly 0.  A row of one edge gives exactly w = 1 and gl = 0.
 *   Every sum has a fixed order and nothing is added atomically: both directions are bitwise
 *   repeatable for equal arguments, chunk_edges included; another chunk_edges groups a cut
 *   row's sums differently, so results may differ between chunk sizes within the bound.
 * Non-finite values follow the IEEE evaluation of the formulas, as torch.softmax does: a row
 *   holding a NaN or a +Inf logit is all NaN; a -Inf logit gives exactly 0 unless every logit of
 *   the row is -Inf, then the row is all NaN; a NaN in s_src[c] reaches every row that reads
 *   column c and no other, and a NaN in a column no edge reads reaches nothing.
 * Memory, as the top comment: the workspace (per-item partials of the cut rows; for the GAT
 *   backward also gz [num_e] and the column side's partials) is exactly the queried size, 256-B
 *   aligned, and may hold anything; a shorter one is rejected with MAXK_ERR_INVALID ("workspace
 *   too small") on the host before anything is launched; w, grad_logits, grad_s_dst [num_rows]
 *   and grad_s_src [num_cols] are fully written (w: every edge; rows without edges write
 *   nothing); inputs are never written; nothing else is touched; no output may alias an input.
 *   The forward stages the logits in w before it normalises them.
 * Argument errors (null pointer, negative size, negative_slope outside [0, 1] or NaN):
 *   MAXK_ERR_INVALID with a message, before any launch.
 * ------------------------------------------------------------------------- */
size_t maxk_edge_softmax_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e,
                                        int32_t chunk_edges);
int maxk_edge_softmax(const int32_t *row_ptr, const float *logits, float *w, int64_t num_rows,
                      int64_t num_cols, int64_t num_e, int32_t chunk_edges, void *workspace,
                      size_t workspace_bytes, void *stream);
size_t maxk_edge_softmax_backward_workspace_size(int64_t num_rows, int64_t num_cols,
                                                 int64_t num_e, int32_t chunk_edges);
int maxk_edge_softmax_backward(const int32_t *row_ptr, const float *w, const float *grad_w,
                               float *grad_logits, int64_t num_rows, int64_t num_cols,
                               int64_t num_e, int32_t chunk_edges, void *workspace,
                               size_t workspace_bytes, void *stream);
size_t maxk_gat_edge_softmax_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e,
                                            int32_t chunk_edges);
int maxk_gat_edge_softmax(const int32_t *row_ptr, const int32_t *col_idx, const float *s_dst,
                          const float *s_src, float negative_slope, float *w, int64_t num_rows,
                          int64_t num_cols, int64_t num_e, int32_t chunk_edges, void *workspace,
                          size_t workspace_bytes, void *stream);
size_t maxk_gat_edge_softmax_backward_workspace_size(int64_t num_rows, int64_t num_cols,
                                                     int64_t num_e, int32_t chunk_edges);
int maxk_gat_edge_softmax_backward(const int32_t *row_ptr, const int32_t *col_idx,
                                   const int32_t *col_ptr, const int32_t *csc_eid,
                                   const float *s_dst, const float *s_src, float negative_slope,
                                   const float *w, const float *grad_w, float *grad_s_dst,
                                   float *grad_s_src, int64_t num_rows, int64_t num_cols,
                                   int64_t num_e, int32_t chunk_edges, void *workspace,
                                   size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Multi-head GAT edge softmax: maxk_gat_edge_softmax and its backward for H = num_heads heads
 * over one walk of the graph -- the attention coefficients edge_val [num_heads, num_e] that
 * maxk_spgemm_forward_heads takes, and the gradient of the scores from the grad_edge that
 * maxk_edge_weight_grad_heads returns.  The reference has no counterpart.
 * Layout, head-major, so every head's slice is an array the single-head entries take:
 *   s_dst, grad_s_dst  f32 [num_heads, num_rows];   s_src, grad_s_src  f32 [num_heads, num_cols];
 *   w, grad_w          f32 [num_heads, num_e], CSR order inside a head.
 * 1 <= num_heads <= MAXK_MAX_HEADS, any value in the range.
 * What the heads share: col_idx[e] is read once per edge; s_src is first copied to
 *   ss_t [num_cols, HP] in the workspace, HP = num_heads rounded up to 2, 4 or 8 (pad heads 0,
 *   never stored to an output), so the random read of a column's scores is one aligned
 *   4 * HP-byte vector inside one 64-B sector for all heads; the backward writes gz edge-major,
 *   gzT [num_e, HP], and the column sums read csc_eid once and gather one vector per CSC slot.
 *   num_heads == 1 has nothing to share and is the single-head entry, workspace size included.
 * Partition, item rule (chunk_edges, 0 = the same auto rule), lane assignment, sum orders and
 *   slot merges are the single-head entries'.  For equal chunk_edges head h of w equals
 *   maxk_gat_edge_softmax on head h's slices bitwise; the gradients equal
 *   maxk_gat_edge_softmax_backward's within the bounds above (the same sums in the same order,
 *   but the compiler contracts a multiply and the add it feeds differently in the two kernels),
 *   bitwise at num_heads == 1.  Numerics, repeatability and the non-finite rules are those
 *   stated above, per head, and head h's outputs hold head h's inputs only: they do not depend,
 *   bitwise, on the other heads' scores or grad_w, and a NaN in s_src[h, c] reaches head h's
 *   rows that read c and nothing else.
 * Memory: as the single-head entries (exactly the queried size, 256-B aligned, any content, a
 *   shorter one rejected on the host before any launch; every output element written, exact 0
 *   for a row without edges and a column no edge reads; num_e == 0 launches nothing forward and
 *   writes zeros backward; inputs never written; no atomics, no allocation).  The workspace
 *   holds ss_t and num_heads times the row slots, and for the backward gzT and num_heads times
 *   the column slots.  gzT is 4 * HP * num_e bytes, num_heads times the single-head gz that H
 *   calls would reuse (3.7 GB against 458 MB at 8 heads and 114.6 M edges): the price of one
 *   sector per CSC slot.
 * Argument errors (num_heads outside [1, MAXK_MAX_HEADS], a null pointer, negative sizes,
 *   negative_slope outside [0, 1] or NaN): MAXK_ERR_INVALID with a message, before any launch.
 * ------------------------------------------------------------------------- */
size_t maxk_gat_edge_softmax_heads_workspace_size(int32_t num_heads, int64_t num_rows,
                                                  int64_t num_cols, int64_t num_e,
                                                  int32_t chunk_edges);
int maxk_gat_edge_softmax_heads(const int32_t *row_ptr, const int32_t *col_idx,
                                const float *s_dst, const float *s_src, float negative_slope,
                                float *w, int32_t num_heads, int64_t num_rows, int64_t num_cols,
                                int64_t num_e, int32_t chunk_edges, void *workspace,
                                size_t workspace_bytes, void *stream);
size_t maxk_gat_edge_softmax_heads_backward_workspace_size(int32_t num_heads, int64_t num_rows,
                                                           int64_t num_cols, int64_t num_e,
                                                           int32_t chunk_edges);
int maxk_gat_edge_softmax_heads_backward(const int32_t *row_ptr, const int32_t *col_idx,
                                         const int32_t *col_ptr, const int32_t *csc_eid,
                                         const float *s_dst, const float *s_src,
                                         float negative_slope, const float *w,
                                         const float *grad_w, float *grad_s_dst,
                                         float *grad_s_src, int32_t num_heads, int64_t num_rows,
                                         int64_t num_cols, int64_t num_e, int32_t chunk_edges,
                                         void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Fused multi-head GAT attention: the edge softmax inside the aggregation walk,
 *   out[h, r, cbsr_idx[c,l]] += alpha[h,e] * cbsr_val[c,l]        e in row r, c = col_idx[e]
 *   alpha[h,e] = exp(l_he - m_hr) / z_hr,   l_he = leaky_relu(s_dst[h,r] + s_src[h,c]),
 *   m_hr = max_e l_he,   z_hr = sum_e exp(l_he - m_hr)
 * -- maxk_gat_edge_softmax_heads followed by maxk_spgemm_forward_heads in one walk of the graph.
 * alpha [num_heads, num_e] exists nowhere, not in an output and not in the workspace: the
 * outputs are out [num_heads, num_rows, dim_origin] and the row statistics row_max = m and
 * row_sum = z, f32 [num_heads, num_rows], from which maxk_gat_edge_alpha_heads rebuilds
 *   w[h,e] = exp(l_he - row_max[h,r]) / row_sum[h,r]          f32 [num_heads, num_e], CSR order
 * for the backward (one col_idx read and one score-vector gather per edge, no reductions).  The
 * reference has no counterpart.  Head-major layout as above; 1 <= num_heads <= MAXK_MAX_HEADS,
 * any value, one head included (there is no single-head entry to hand off to).  There is no
 * row_div: attention rows are normalised by z.
 * Per row piece the kernel sweeps the scores once for the piece's maximum per head, then
 *   gathers one record per edge for all heads with p = exp(l - m_piece), summing p * value in
 *   LDS and p per head: nothing is rescaled per edge.  A row inside one work item is stored as
 *   sum / z; a hub row cut over items leaves unnormalised pieces with their (m, z), merged in
 *   item order: m = max m_i, each piece scaled by exp(m_i - m), one division.  No global and no
 *   LDS atomics.
 * Shapes: any 1 <= dim_k <= dim_origin <= 256 (dim_k % 4 != 0, odd dim_origin, dim_k > 64), any
 *   num_rows != num_cols; num_e == 0 writes zeros to all of out and both statistics; a table
 *   past 2^24 columns or 4 GiB of packed records is rejected with MAXK_ERR_INVALID.  There is
 *   no dense route and no _sel / records form.
 * Writes: every element of out, row_max and row_sum (the alpha entry: every edge of w;
 *   num_e == 0 launches nothing).  A row without edges gives exact zeros in all three; a column
 *   of out that no edge of the row selects is exactly 0.
 * Numerics (tests/gat_attention_ref.py; u = 2^-24): the composition of the two bounds above.
 *   Each weight is within (n_r + 24 + 16 A_r) * u * alpha + (n_r + 16) * 2^-149 -- the edge
 *   softmax's bound with 8 u more for a cut row's second exp and scale product -- carried
 *   through the sum, plus (n + 8) * u * sum|alpha * value| with the subnormal floor, n the
 *   element's number of addends.  row_max is within 2 A_r u of exact, row_sum within the
 *   weight bound's relative part.  w from the statistics is within the edge softmax's bound.
 * Non-finite values follow the IEEE evaluation of the formulas, as the two entries composed:
 *   a row with a NaN or +Inf logit is NaN wherever it has an addend (and 0 elsewhere), a -Inf
 *   logit contributes exactly 0, a row of only -Inf is NaN wherever it has an addend; a NaN in
 *   s_src[h, c] reaches head h's rows that read c and nothing else.
 * Bitwise repeatable for equal arguments whatever the workspace held (every sum's order is
 *   fixed by the graph, chunk_edges, dim_k and num_heads); head h's slices of the three outputs
 *   do not depend, bitwise, on the other heads' scores.
 * Memory, as the top comment: the workspace (packed records, ss_t [num_cols, HP], per-head
 *   slabs and statistics of the cut rows; for the alpha entry ss_t alone) is exactly the queried
 *   size, 256-B aligned, and may hold anything; a shorter one is rejected ("workspace too
 *   small") on the host before any launch; nothing is written outside the outputs and the
 *   workspace, inputs are never written; no allocation, copy or synchronisation.
 * Argument errors (num_heads outside [1, MAXK_MAX_HEADS], a null pointer, negative sizes,
 *   negative_slope outside [0, 1] or NaN, k / D range): MAXK_ERR_INVALID with a message naming
 *   the argument, before any launch.
 * chunk_edges: tokens per wavefront work item, 0 = the forward's auto rule.
 * ------------------------------------------------------------------------- */
size_t maxk_gat_attention_heads_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e,
                                               int32_t dim_origin, int32_t dim_k,
                                               int32_t num_heads, int32_t chunk_edges);
int maxk_gat_attention_heads(const int32_t *row_ptr, const int32_t *col_idx, const float *s_dst,
                             const float *s_src, float negative_slope, const float *cbsr_val,
                             const uint8_t *cbsr_idx, float *out, float *row_max, float *row_sum,
                             int64_t num_rows, int64_t num_cols, int64_t num_e,
                             int32_t dim_origin, int32_t dim_k, int32_t num_heads,
                             int32_t chunk_edges, void *workspace, size_t workspace_bytes,
                             void *stream);
size_t maxk_gat_edge_alpha_heads_workspace_size(int32_t num_heads, int64_t num_rows,
                                                int64_t num_cols, int64_t num_e);
int maxk_gat_edge_alpha_heads(const int32_t *row_ptr, const int32_t *col_idx, const float *s_dst,
                              const float *s_src, float negative_slope, const float *row_max,
                              const float *row_sum, float *w, int32_t num_heads,
                              int64_t num_rows, int64_t num_cols, int64_t num_e, void *workspace,
                              size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Fused backward of maxk_gat_attention_heads: the three gradients from one walk of the graph,
 *   alpha_he = exp(l_he - row_max[h,r]) / row_sum[h,r]           (as maxk_gat_edge_alpha_heads)
 *   ga_he    = sum_l cbsr_val[c,l] * grad_out[h, r, cbsr_idx[c,l]]
 *   t_hr     = sum_{j : out[h,r,j] != 0} out[h,r,j] * grad_out[h,r,j]
 *   gz_he    = alpha_he * (ga_he - t_hr) * (z_he > 0 ? 1 : negative_slope),  z = s_dst + s_src
 *   grad_s_dst[h,r] = sum_{e in r} gz_he       grad_s_src[h,c] = sum_{e: col = c} gz_he
 *   grad_cbsr[c,l]  = sum_h sum_{e -> c} alpha_he * grad_out[h, r, cbsr_idx[c,l]]
 * -- what maxk_gat_edge_alpha_heads, maxk_edge_weight_grad_heads,
 * maxk_gat_edge_softmax_heads_backward and maxk_sspmm_backward_heads compute in four walks, with
 * no tensor of num_heads * num_e elements in an input, an output or the workspace beside the
 * edge-major gz [num_e, HP] the column sums read.  out, row_max and row_sum are what the forward
 * returned; t, the softmax backward's sum over the row of alpha * ga, is the dot product of the
 * two dense rows out[h,r,:] and grad_out[h,r,:], which every work item forms for itself, so a
 * row cut over items is walked once.  The terms with out == 0 are skipped: the forward stores
 * an exact 0 in every column no edge of the row selects, and a NaN or Inf of grad_out there
 * reaches nothing (the rule of maxk_edge_weight_grad_heads).
 * col_ptr / csc_eid: the graph's maxk_transpose_plan.  grad_s_dst [num_heads, num_rows],
 *   grad_s_src [num_heads, num_cols] (summed in CSC slot order) and grad_cbsr [num_cols, dim_k]
 *   (the heads summed per edge in head order, the edges in CSC slot order).  The reference has no
 *   counterpart.
 * Per edge the walk loads col_idx once, one packed record (value and selector) and one score
 *   vector; alpha and gz are computed once per edge and head.  No global and no LDS atomics.
 * Shapes: any 1 <= dim_k <= dim_origin <= 256 (dim_k % 4 != 0, odd dim_origin, dim_k > 64),
 *   1 <= num_heads <= MAXK_MAX_HEADS, any value, one head included; num_rows != num_cols
 *   allowed; num_e == 0 writes zeros to all three outputs; a table past 2^24 columns or 4 GiB
 *   of packed records is rejected with MAXK_ERR_INVALID.
 * Writes: every element of the three outputs.  A row without edges, a column no edge reads and
 *   a slot whose selector is >= dim_origin give an exact 0; a repeated selector's slots each
 *   receive the column's gradient.
 * Numerics (tests/gat_attention_bwd_ref.py): alpha within the edge softmax's bound, ga within
 *   the edge gradient's, t within (n_t + 8) u sum|out g| plus the error of `out` carried through
 *   grad_out; gz the product bound of the three; the sums the sum bounds.  The one difference
 *   from the stored path: there t is summed over the row's edges, here over its columns, so a
 *   row of a single edge gives gz within the bound, not the exact 0 of ga - ga.
 * Non-finite values follow the IEEE evaluation of the formulas: a NaN in s_src[h, c] reaches
 *   head h's grad_s_dst rows that read c, the grad_s_src columns those rows read and grad_cbsr
 *   of those columns; a -Inf logit gives gz = 0; a NaN of grad_out in a column the row does not
 *   select reaches nothing.
 * Bitwise repeatable for equal arguments whatever the workspace held (every sum's order is
 *   fixed by the graph, chunk_edges, dim_k and num_heads); head h's slices of grad_s_dst and
 *   grad_s_src do not depend, bitwise, on the other heads' scores (grad_cbsr sums the heads).
 * Memory, as the top comment: the workspace (contribution rows T [num_e + 1, dim_k] and the
 *   phase-2 slabs, the packed records, ss_t [num_cols, HP], gz [num_e, HP], the row and column
 *   slots x num_heads) is exactly the queried size, 256-B aligned, and may hold anything; a
 *   shorter one is rejected ("workspace too small") on the host before any launch; nothing is
 *   written outside the outputs and the workspace, inputs are never written; no allocation, copy
 *   or synchronisation.  The size is non-decreasing in num_e.
 * Argument errors (num_heads outside [1, MAXK_MAX_HEADS], a null pointer, negative sizes,
 *   negative_slope outside [0, 1] or NaN, k / D range): MAXK_ERR_INVALID with a message naming
 *   the argument, before any launch.
 * chunk_edges: tokens per wavefront work item of every walk, 0 = each walk's auto rule.
 * ------------------------------------------------------------------------- */
size_t maxk_gat_attention_heads_backward_workspace_size(int64_t num_rows, int64_t num_cols,
                                                        int64_t num_e, int32_t dim_origin,
                                                        int32_t dim_k, int32_t num_heads,
                                                        int32_t chunk_edges);
int maxk_gat_attention_heads_backward(
    const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr,
    const int32_t *csc_eid, const float *s_dst, const float *s_src, float negative_slope,
    const float *cbsr_val, const uint8_t *cbsr_idx, const float *out, const float *row_max,
    const float *row_sum, const float *grad_out, float *grad_s_dst, float *grad_s_src,
    float *grad_cbsr, int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin,
    int32_t dim_k, int32_t num_heads, int32_t chunk_edges, void *workspace,
    size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Attention dropout: the GAT's dropout of the coefficients between the edge softmax and the
 * aggregation, by a mask that is a pure function of (seed, head, edge) and is stored nowhere.
 * The mask of head h and edge e (its CSR position, 0 <= e < num_e), for a rate p and a 64-bit
 * seed:
 *   (r0, r1, r2, r3) = Philox4x32-10(counter (e, 0, h >> 2, 0),
 *                                    key (seed & 0xffffffff, seed >> 32))
 *     -- multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, ten
 *     rounds;
 *   r = r[h & 3];  thr = min(floor(p * 2^32), 2^32 - 1), in double on the host;
 *   the edge is dropped iff r < thr;  d_he = dropped ? 0 : scale,
 *   scale = (float)(1 / (1 - (double)p)).
 * Nothing else enters: not chunk_edges, not the work-item cut, not num_heads or the padded head
 * count, not which entry evaluates it, so the three entries below and every call of them agree
 * on the mask.  seed travels by value: a captured graph replays the same mask on every replay;
 * a training loop that wants a fresh mask per step passes a fresh seed outside the capture.
 * 0 <= p < 1 and not NaN, otherwise MAXK_ERR_INVALID naming p.  The reference has no counterpart.
 *
 * maxk_edge_dropout_heads: out[h,e] = w[h,e] * d_he, head-major f32 [num_heads, num_e]; out may
 *   be w.  One elementwise kernel, no workspace.  It serves the stored path's forward (on
 *   alpha), its backward (on grad_alpha) and the rebuilt backward of the fused path.  The stored
 *   path therefore keeps two [num_heads, num_e] tensors for its backward, alpha for the softmax
 *   backward and the dropped alpha for the aggregation: a known limit, the fused entries below
 *   keep none.  Writes every element of out; num_e == 0 launches nothing.  A kept weight is the
 *   correctly rounded w * scale, a dropped one w * 0 (a NaN or Inf stays NaN).
 * maxk_gat_attention_heads_dropout: maxk_gat_attention_heads with
 *   out[h, r, cbsr_idx[c,l]] += alpha[h,e] * d_he * cbsr_val[c,l].
 *   row_max and row_sum are the statistics of the undropped softmax, bitwise those of
 *   maxk_gat_attention_heads at the same chunk_edges: dropout follows the normalisation.  The
 *   lane that computes an edge's weight evaluates its mask; the kernel sums p * (0 or 1) * value
 *   and multiplies the row by scale after the division by z.
 * maxk_gat_attention_heads_dropout_backward: maxk_gat_attention_heads_backward with
 *   gz_he = alpha_he * (d_he * ga_he - t_hr) * (z_he > 0 ? 1 : negative_slope),
 *   grad_cbsr[c,l] = sum_h sum_{e -> c} alpha_he * d_he * grad_out[h, r, cbsr_idx[c,l]],
 *   t_hr as there, from the dropped out: sum_e alpha_he * d_he * ga_he is still the dot product
 *   of out[h,r,:] and grad_out[h,r,:].  Same p and seed as the forward that produced out.
 * Both take the arguments, shapes, workspace (the _workspace_size queries return the sizes of
 *   the entries without dropout), memory contract, argument errors and repeatability of the
 *   entries they extend; p == 0 runs those entries' kernels and is bitwise equal to them.
 * Numerics (tests/attn_dropout_ref.py): the bounds of the entries without dropout carried
 *   through the factor d <= scale, plus one rounding (u = 2^-24, relative) for the product by
 *   scale.  Non-finite values follow the IEEE evaluation of the formulas with d as a factor:
 *   0 * NaN and 0 * Inf are NaN, dropping does not shield.  For finite inputs a row all of whose
 *   edges are dropped in head h has exact zeros in out[h, r, :].
 * No global and no LDS atomics.
 * ------------------------------------------------------------------------- */
int maxk_edge_dropout_heads(const float *w, float *out, int32_t num_heads, int64_t num_e, float p,
                            uint64_t seed, void *stream);
size_t maxk_gat_attention_heads_dropout_workspace_size(int64_t num_rows, int64_t num_cols,
                                                       int64_t num_e, int32_t dim_origin,
                                                       int32_t dim_k, int32_t num_heads,
                                                       int32_t chunk_edges);
int maxk_gat_attention_heads_dropout(
    const int32_t *row_ptr, const int32_t *col_idx, const float *s_dst, const float *s_src,
    float negative_slope, const float *cbsr_val, const uint8_t *cbsr_idx, float *out,
    float *row_max, float *row_sum, int64_t num_rows, int64_t num_cols, int64_t num_e,
    int32_t dim_origin, int32_t dim_k, int32_t num_heads, int32_t chunk_edges, float p,
    uint64_t seed, void *workspace, size_t workspace_bytes, void *stream);
size_t maxk_gat_attention_heads_dropout_backward_workspace_size(
    int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
    int32_t num_heads, int32_t chunk_edges);
int maxk_gat_attention_heads_dropout_backward(
    const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr,
    const int32_t *csc_eid, const float *s_dst, const float *s_src, float negative_slope,
    const float *cbsr_val, const uint8_t *cbsr_idx, const float *out, const float *row_max,
    const float *row_sum, const float *grad_out, float *grad_s_dst, float *grad_s_src,
    float *grad_cbsr, int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin,
    int32_t dim_k, int32_t num_heads, int32_t chunk_edges, float p, uint64_t seed,
    void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Fused multi-head dot-product attention on CBSR keys: the scaled dot-product score and its edge
 * softmax inside the aggregation walk,
 *   l_he = scale * sum_l cbsr_val[c,l] * q[h, r, cbsr_idx[c,l]]      e in row r, c = col_idx[e]
 *   m_hr = max_e l_he,   z_hr = sum_e exp(l_he - m_hr),   alpha[h,e] = exp(l_he - m_hr) / z_hr
 *   out[h, r, cbsr_idx[c,l]] += alpha[h,e] * cbsr_val[c,l]
 * -- maxk_edge_weight_grad_heads with grad_out := q, the scale, num_heads edge softmaxes and
 * maxk_spgemm_forward_heads in one walk of the graph.  q is f32 [num_heads, num_rows,
 * dim_origin], the query of destination r already mapped into the feature space
 * (q_r . k_c = x_r^T W_q^T W_k x_c = q[h, r] . x_c, and x_c is the CBSR row); selectors
 * >= dim_origin add nothing.  Neither the logits nor alpha [num_heads, num_e] exist anywhere,
 * not in an output and not in the workspace: the outputs are out [num_heads, num_rows,
 * dim_origin] and the row statistics row_max = m and row_sum = z, f32 [num_heads, num_rows], from
 * which maxk_dot_edge_alpha_heads rebuilds
 *   w[h,e] = exp(l_he - row_max[h,r]) / row_sum[h,r]          f32 [num_heads, num_e], CSR order
 * for the backward (one record gather per edge for all heads, no reductions over edges).  The
 * reference has no counterpart.  Head-major layout as above; 1 <= num_heads <= MAXK_MAX_HEADS,
 * any value, one head included.  There is no row_div: attention rows are normalised by z.
 * Per row piece the kernel stages the num_heads rows scale * q[h, r, :] in LDS, sweeps the
 *   records once for the piece's maximum per head, then gathers each record again (from the
 *   caches) with p = exp(l - m_piece), l recomputed by the same device functions, summing
 *   p * value in LDS and p per head: nothing is rescaled per edge.  A row inside one work item is
 *   stored as sum / z; a hub row cut over items leaves unnormalised pieces with their (m, z),
 *   merged in item order: m = max m_i, each piece scaled by exp(m_i - m), one division.  No
 *   global and no LDS atomics.
 * Shapes: any 1 <= dim_k <= dim_origin <= 256 (dim_k % 4 != 0, odd dim_origin, dim_k > 64), any
 *   num_rows != num_cols; num_e == 0 writes zeros to all of out and both statistics (the alpha
 *   entry launches nothing); a table past 2^24 columns or 4 GiB of packed records is rejected
 *   with MAXK_ERR_INVALID.  scale: finite and > 0.
 * Writes: every element of out, row_max and row_sum (the alpha entry: every edge of w).  A row
 *   without edges gives exact zeros in all three; a column of out that no edge of the row selects
 *   is exactly 0.
 * Numerics (tests/dot_attention_ref.py; u = 2^-24): a logit is within
 *   d = (n_c + 8) * u * scale * sum|value * q| + 2^-149 of exact, n_c its number of kept slots;
 *   each weight is within (n_r + 24 + 16 A_r) * u * alpha + 2 d * alpha + (n_r + 16) * 2^-149,
 *   A_r = max|l| -- the edge softmax's bound, 8 u for a cut row's merge and the logit error
 *   carried through the exponent -- and out within that carried through the sum plus
 *   (n + 8) * (u * sum|alpha * value| + 2^-149), n the element's number of addends.  row_max is
 *   within the logit bound, row_sum within the weight bound's relative part.
 * Non-finite values follow the IEEE evaluation of the formulas: a row with a NaN or +Inf logit is
 *   NaN wherever it has an addend (and 0 elsewhere), a -Inf logit contributes exactly 0, a row
 *   of only -Inf is NaN wherever it has an addend; a NaN in q[h, r, j] at a column j that none of
 *   row r's neighbours selects reaches nothing (maxk_edge_weight_grad_heads' rule).
 * Bitwise repeatable for equal arguments whatever the workspace held (every sum's order is
 *   fixed by the graph, chunk_edges, dim_k and num_heads); head h's slices of the three outputs
 *   do not depend, bitwise, on the other heads' q.
 * Memory, as the top comment: the workspace (packed records, per-head slabs and statistics of
 *   the cut rows -- the only term that grows with num_heads * num_e; for the alpha entry the
 *   records alone) is exactly the queried size, 256-B aligned, and may hold anything; a shorter
 *   one is rejected ("workspace too small") on the host before any launch; nothing is written
 *   outside the outputs and the workspace, inputs are never written; no allocation, copy or
 *   synchronisation.  The size is non-decreasing in num_e.
 * Argument errors (num_heads outside [1, MAXK_MAX_HEADS], a null pointer, negative sizes, scale
 *   not finite or <= 0, k / D range): MAXK_ERR_INVALID with a message naming the argument,
 *   before any launch.
 * chunk_edges: tokens per wavefront work item, 0 = the auto rule, sized for the waves a CU holds
 *   beside the staged query rows.
 * ------------------------------------------------------------------------- */
size_t maxk_dot_attention_heads_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e,
                                               int32_t dim_origin, int32_t dim_k,
                                               int32_t num_heads, int32_t chunk_edges);
int maxk_dot_attention_heads(const int32_t *row_ptr, const int32_t *col_idx, const float *q,
                             float scale, const float *cbsr_val, const uint8_t *cbsr_idx,
                             float *out, float *row_max, float *row_sum, int64_t num_rows,
                             int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
                             int32_t num_heads, int32_t chunk_edges, void *workspace,
                             size_t workspace_bytes, void *stream);
size_t maxk_dot_edge_alpha_heads_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e,
                                                int32_t dim_origin, int32_t dim_k,
                                                int32_t num_heads, int32_t chunk_edges);
int maxk_dot_edge_alpha_heads(const int32_t *row_ptr, const int32_t *col_idx, const float *q,
                              float scale, const float *cbsr_val, const uint8_t *cbsr_idx,
                              const float *row_max, const float *row_sum, float *w,
                              int64_t num_rows, int64_t num_cols, int64_t num_e,
                              int32_t dim_origin, int32_t dim_k, int32_t num_heads,
                              int32_t chunk_edges, void *workspace, size_t workspace_bytes,
                              void *stream);

/* ---------------------------------------------------------------------------
 * Fused backward of maxk_dot_attention_heads: both gradients in one walk of the graph,
 *   l_he     = scale * sum_l cbsr_val[c,l] * q[h, r, s]           e in row r, c = col_idx[e],
 *   alpha_he = exp(l_he - row_max[h,r]) / row_sum[h,r]            s = cbsr_idx[c,l]
 *                                                                (as maxk_dot_edge_alpha_heads)
 *   ga_he    = sum_l cbsr_val[c,l] * grad_out[h, r, s]
 *   t_hr     = sum_{j : out[h,r,j] != 0} out[h,r,j] * grad_out[h,r,j]
 *   gl_he    = alpha_he * (ga_he - t_hr)
 *   grad_q[h,r,j]  = scale * sum_{e in r} gl_he * x_c[j]          x_c the scattered CBSR row
 *   grad_cbsr[c,l] = sum_h sum_{e -> c} (alpha_he * grad_out[h,r,s] + scale * gl_he * q[h,r,s])
 * -- what maxk_dot_edge_alpha_heads, maxk_edge_weight_grad_heads, num_heads
 * maxk_edge_softmax_backward calls, maxk_spgemm_forward_heads and two maxk_sspmm_backward_heads
 * calls compute in six record gathers per edge, with no tensor of num_heads * num_e elements in
 * an input, an output or the workspace beside the edge-major gl [num_e, HP] the aggregation of
 * grad_q reads.  out, row_max and row_sum are what the forward returned; t, the softmax
 * backward's sum over the row of alpha * ga, is the dot product of the two dense rows out[h,r,:]
 * and grad_out[h,r,:], which every work item forms for itself, so a row cut over items is walked
 * once.  The terms with out == 0 are skipped: the forward stores an exact 0 in every column no
 * edge of the row selects, and a NaN or Inf of grad_out there reaches nothing (the rule of
 * maxk_gat_attention_heads_backward).
 * col_ptr / csc_eid: the graph's maxk_transpose_plan.  grad_q [num_heads, num_rows, dim_origin]
 *   and grad_cbsr [num_cols, dim_k] (the heads summed per edge in head order, the edges in CSC
 *   slot order).  The reference has no counterpart.
 * Per edge the first walk loads col_idx once and one packed record (value and selector); the
 *   logit is formed by the forward's device functions on the same staged row scale * q, so
 *   exp(l - row_max) <= 1 as in the alpha entry; alpha and gl are computed once per edge and
 *   head.  The second walk is the multi-head forward's with gl as the weights and a product by
 *   scale at the end; a hub row's pieces are added in item order.  No global and no LDS atomics.
 * Shapes: any 1 <= dim_k <= dim_origin <= 256 (dim_k % 4 != 0, odd dim_origin, dim_k > 64),
 *   1 <= num_heads <= MAXK_MAX_HEADS, any value, one head included; num_rows != num_cols
 *   allowed; num_e == 0 writes zeros to both outputs; a table past 2^24 columns or 4 GiB of
 *   packed records is rejected with MAXK_ERR_INVALID.  scale: finite and > 0.
 * Writes: every element of both outputs.  An element of a row without edges, a column of grad_q
 *   that no neighbour of the row selects, a column of the table no edge reads and a slot whose
 *   selector is >= dim_origin give an exact 0; a repeated selector's slots each receive the
 *   column's gradient.
 * Numerics (tests/dot_attention_bwd_ref.py): alpha within the forward's weight bound, ga within
 *   the edge gradient's, t within (n_t + 8) u sum|out g| plus the error of `out` carried through
 *   grad_out; gl the product bound of the three; the sums the sum bounds, with one more rounding
 *   for the staged scale * q and one for the product by scale.  The one difference from the
 *   stored path: there t is summed over the row's edges, here over its columns, so a row of a
 *   single edge gives gl within the bound, not the exact 0 of ga - ga.
 * Non-finite values follow the IEEE evaluation of the formulas: a NaN in q[h, r, j] at a column
 *   a neighbour of r selects reaches head h's grad_q row r and grad_cbsr of the columns r reads,
 *   at a column none selects it reaches nothing; a -Inf logit gives alpha = 0 and contributes 0
 *   for a finite ga; a NaN of grad_out in a column the row does not select reaches nothing.
 * Bitwise repeatable for equal arguments whatever the workspace held (every sum's order is
 *   fixed by the graph, chunk_edges, dim_k and num_heads); head h's slice of grad_q does not
 *   depend, bitwise, on the other heads' q, out, statistics or grad_out (grad_cbsr sums the
 *   heads).
 * Memory, as the top comment: the workspace (contribution rows T [num_e + 1, dim_k] and the
 *   phase-2 slabs, the packed records, gl [num_e, HP] and the second walk's per-head slabs of the
 *   cut rows -- one array of HP * num_e floats and never room for a second) is exactly the
 *   queried size, 256-B aligned, and may hold anything; a shorter one is rejected ("workspace too
 *   small") on the host before any launch; nothing is written outside the outputs and the
 *   workspace, inputs are never written; no allocation, copy or synchronisation.  The size is
 *   non-decreasing in num_e.
 * Argument errors (num_heads outside [1, MAXK_MAX_HEADS], a null pointer, negative sizes, scale
 *   not finite or <= 0, k / D range): MAXK_ERR_INVALID with a message naming the argument,
 *   before any launch.
 * chunk_edges: tokens per wavefront work item of every walk, 0 = each walk's auto rule.
 * ------------------------------------------------------------------------- */
size_t maxk_dot_attention_heads_backward_workspace_size(int64_t num_rows, int64_t num_cols,
                                                        int64_t num_e, int32_t dim_origin,
                                                        int32_t dim_k, int32_t num_heads,
                                                        int32_t chunk_edges);
int maxk_dot_attention_heads_backward(
    const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr, const int32_t *csc_eid,
    const float *q, float scale, const float *cbsr_val, const uint8_t *cbsr_idx, const float *out,
    const float *row_max, const float *row_sum, const float *grad_out, float *grad_q,
    float *grad_cbsr, int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin,
    int32_t dim_k, int32_t num_heads, int32_t chunk_edges, void *workspace,
    size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Attention dropout inside the fused dot-product attention: the mask of the attention-dropout
 * block above (head h of edge e is dropped iff word h & 3 of Philox4x32-10(counter
 * (e, 0, h >> 2, 0), key (seed lo, seed hi)) is < thr; d_he = dropped ? 0 : scale), word for word:
 * maxk_edge_dropout_heads and both entries below agree on it whatever chunk_edges, the work-item
 * cut, num_heads or the padded head count are, and seed travels by value (a captured graph
 * replays the same mask).  0 <= p < 1 and not NaN, otherwise MAXK_ERR_INVALID naming p, before
 * any launch.
 * maxk_dot_attention_heads_dropout: maxk_dot_attention_heads with
 *   out[h, r, cbsr_idx[c,l]] += alpha[h,e] * d_he * cbsr_val[c,l].
 *   row_max and row_sum are the statistics of the undropped softmax, bitwise those of
 *   maxk_dot_attention_heads at the same chunk_edges: dropout follows the normalisation.  The
 *   first sweep is unchanged; in the second the sum of p takes the unmasked p, the kernel sums
 *   p * (0 or 1) * value and multiplies the row by scale once, after the division by z (a hub
 *   row: in the merge of its pieces).  One Philox evaluation serves a quad of heads and several
 *   wave steps.
 * maxk_dot_attention_heads_dropout_backward: maxk_dot_attention_heads_backward with
 *   gl_he = alpha_he * (d_he * ga_he - t_hr),
 *   grad_cbsr[c,l] = sum_h sum_{e -> c} (alpha_he * d_he * grad_out[h,r,s] + scale * gl_he * q[h,r,s]),
 *   grad_q and t_hr as there, t from the dropped out: sum_e alpha_he * d_he * ga_he is still the
 *   dot product of out[h,r,:] and grad_out[h,r,:], so a cut row is still walked once.  Same p and
 *   seed as the forward that produced out.
 * maxk_dot_edge_alpha_heads has no masked form: a rebuilt backward masks its result (for the
 *   aggregation's coefficients) and grad_alpha with maxk_edge_dropout_heads.
 * Both take the arguments, shapes, writes, workspace (the _workspace_size queries return the
 *   sizes of the entries without dropout), memory contract, argument errors and repeatability of
 *   the entries they extend; p == 0 runs those entries' kernels and is bitwise equal to them.
 * Numerics (tests/dot_attn_dropout_ref.py): the bounds of the entries without dropout carried
 *   through the factor d <= scale, plus one rounding (u = 2^-24, relative) for the product by
 *   scale.  Non-finite values follow the IEEE evaluation of the formulas with d as a factor:
 *   0 * NaN and 0 * Inf are NaN, dropping does not shield.  For finite inputs a row all of whose
 *   edges are dropped in head h has exact zeros in out[h, r, :].
 * No global and no LDS atomics.
 * ------------------------------------------------------------------------- */
size_t maxk_dot_attention_heads_dropout_workspace_size(int64_t num_rows, int64_t num_cols,
                                                       int64_t num_e, int32_t dim_origin,
                                                       int32_t dim_k, int32_t num_heads,
                                                       int32_t chunk_edges);
int maxk_dot_attention_heads_dropout(
    const int32_t *row_ptr, const int32_t *col_idx, const float *q, float scale,
    const float *cbsr_val, const uint8_t *cbsr_idx, float *out, float *row_max, float *row_sum,
    int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
    int32_t num_heads, int32_t chunk_edges, float p, uint64_t seed, void *workspace,
    size_t workspace_bytes, void *stream);
size_t maxk_dot_attention_heads_dropout_backward_workspace_size(
    int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
    int32_t num_heads, int32_t chunk_edges);
int maxk_dot_attention_heads_dropout_backward(
    const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr, const int32_t *csc_eid,
    const float *q, float scale, const float *cbsr_val, const uint8_t *cbsr_idx, const float *out,
    const float *row_max, const float *row_sum, const float *grad_out, float *grad_q,
    float *grad_cbsr, int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin,
    int32_t dim_k, int32_t num_heads, int32_t chunk_edges, float p, uint64_t seed,
    void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Backward outer-product sampled SpMM (SSpMM):
 *   grad_cbsr[c,l] = sum_{e=(r->c)} edge_val[e] * grad_out[r, cbsr_idx[c,l]] / row_div[r]
 *                  = (A^T diag(1/row_div) G)[c, cbsr_idx[c,l]]     (from the CSR of A)
 * grad_cbsr [num_cols, k] is fully overwritten.  row_div may be NULL.
 * Replaces: spmm_kernel_opt2_sparse_backward_v3 (kernels/spmm_maxk_backward.cu:15-115),
 *           spmm_kernel_opt2_sparse_backward_v3_wrapper (cuda_kernel_wrappers.cu:58-76)
 *           and the /out_degrees of maxk_spgemm_function.py:154-155.
 * This entry point (the "atomic" mode) adds with fp32 global atomics, built with
 * -munsafe-fp-atomics: measured on gfx950, they keep fp32 subnormals (gradients at 2^-130 meet
 * the bound of the top comment with its 2^-149 floor; nothing resolvable is flushed to 0).
 * ------------------------------------------------------------------------- */
size_t maxk_sspmm_backward_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e,
                                          int32_t dim_origin, int32_t dim_k, int32_t chunk_edges);
int maxk_sspmm_backward(const int32_t *row_ptr, const int32_t *col_idx, const float *edge_val,
                        const float *grad_out, const float *row_div, const uint8_t *cbsr_idx,
                        float *grad_cbsr, int64_t num_rows, int64_t num_cols, int64_t num_e,
                        int32_t dim_origin, int32_t dim_k, int32_t chunk_edges,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Same backward, two-phase and atomic-free (bitwise deterministic): phase 1
 * stores each edge's k-float contribution in CSR edge order, phase 2 gathers
 * and sums the contributions of every destination through the CSC permutation.  Needs the transpose plan of the graph
 * (maxk_transpose_plan) and a workspace of
 * maxk_sspmm_backward_csc_workspace_size(...) bytes (about num_e*k*4).
 * ------------------------------------------------------------------------- */
size_t maxk_sspmm_backward_csc_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e,
                                              int32_t dim_origin, int32_t dim_k,
                                              int32_t chunk_edges);
int maxk_sspmm_backward_csc(const int32_t *row_ptr, const int32_t *col_idx, const float *edge_val,
                            const float *grad_out, const float *row_div, const uint8_t *cbsr_idx,
                            const int32_t *col_ptr, const int32_t *csc_eid, float *grad_cbsr,
                            int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin,
                            int32_t dim_k, int32_t chunk_edges, void *workspace,
                            size_t workspace_bytes, void *stream);

/* The same csc backward with the selectors given per edge: edge_sel[num_e, k] (u8, 4-B
 * aligned, dim_k % 4 == 0) with edge_sel[e, l] = cbsr_idx[col_idx[e], l].  Phase 1 then reads
 * them in CSR order beside the weights instead of gathering a random cbsr_idx row (a whole
 * 128-B line) per edge -- the step that bounds phase 1 on large sparse graphs.  A forward that
 * gathered each edge's CBSR record anyway writes the stream for free
 * (maxk_spgemm_forward_sel); maxk_edge_selectors builds it by a gather otherwise. */
int maxk_sspmm_backward_csc_sel(const int32_t *row_ptr, const int32_t *col_idx,
                                const float *edge_val, const float *grad_out, const float *row_div,
                                const uint8_t *edge_sel, const int32_t *col_ptr,
                                const int32_t *csc_eid, float *grad_cbsr, int64_t num_rows,
                                int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                int32_t chunk_edges, void *workspace, size_t workspace_bytes,
                                void *stream);
/* edge_sel[e, l] = cbsr_idx[col_idx[e], l]: any dim_k in [1, 256] and any alignment (16-B words
 * when dim_k % 16 == 0 and both arrays are 16-B aligned, 4-B words for % 4 / 4-B aligned, else
 * bytes) -- also the fallback of maxk_spgemm_forward_sel past 2^24 columns or 4 GiB of records,
 * so a stream that works on a small graph works on a large one. */
int maxk_edge_selectors(const int32_t *col_idx, const uint8_t *cbsr_idx, int64_t num_e,
                        int32_t dim_k, uint8_t *edge_sel, void *stream);
/* Workgroups (256 threads) maxk_edge_selectors launches for n_words words: capped at 64 per
 * CU and walked grid-stride, so num_e * k one-byte words past 2^32 still launch. */
int64_t maxk_edge_selectors_blocks(int64_t n_words);

/* ---------------------------------------------------------------------------
 * The csc backward for H = num_heads heads (the multi-head layout above: edge_val f32
 * [num_heads, num_e], grad_out f32 [num_heads, num_rows, dim_origin], one row_div), summed over
 * the heads:
 *   grad_cbsr[c,l] = sum_h sum_{e=(r->c)} edge_val[h,e] * grad_out[h, r, cbsr_idx[c,l]] / row_div[r]
 * the adjoint of maxk_spgemm_forward_heads in cbsr_val; what H maxk_sspmm_backward_csc calls and
 * H - 1 additions give.  The reference has no counterpart.  Phase 1 sums the heads per edge
 * before it stores (per row piece the H rows grad_out[h, r, :] / row_div[r] are staged in LDS;
 * per edge one column load, one selector gather, H weights, and one contribution row
 * T[e, l] = sum_h edge_val[h,e] * g_h[cbsr_idx[c,l]], formed in head order with one fma per
 * further head); phase 2 and the fix-up are maxk_sspmm_backward_csc's, over the same workspace
 * layout.  col_ptr / csc_eid: the graph's maxk_transpose_plan.
 * Shapes: any 1 <= dim_k <= dim_origin <= 256 (dim_k % 4 != 0, odd dim_origin, dim_k > 64).
 *   There is no edge_sel, bsort, pull or dense form; a table of 2^24 columns or more is rejected
 *   with MAXK_ERR_INVALID.  num_e == 0 writes zeros to all of grad_cbsr and succeeds; num_cols
 *   == 0 launches nothing.
 * Numerics, in the words of the top comment: every element is within (n + 8) * 2^-24 *
 *   sum|terms| of exact arithmetic (plus the 2^-149 floor), n = num_heads times the number of
 *   edges into column c and sum|terms| over every head's terms.  A slot without addends (a
 *   column no edge reads, a selector >= dim_origin) is exactly 0; repeated selectors each
 *   receive the same sum.  Inf and NaN in grad_out propagate as the IEEE sum of the selected
 *   terms; a NaN in a column of grad_out the destination does not select, or in a row without
 *   an edge to it, reaches nothing.  Non-finite weights and row_div are outside the contract.
 *   The sum order is fixed by the graph, chunk_edges, dim_k and num_heads: bitwise repeatable,
 *   and bitwise equivariant under a power-of-two scale of grad_out or of the weights away from
 *   overflow and underflow.  At num_heads == 1 the result equals maxk_sspmm_backward_csc's
 *   bitwise for the same chunk_edges (each T element is the same single product, phase 2 the
 *   same code).
 * Memory, as the top comment: the workspace is exactly the queried size -- what
 *   maxk_sspmm_backward_csc_workspace_size returns for the same graph, dim_k and chunk_edges --
 *   256-B aligned, and may hold anything; a shorter one is rejected ("workspace too small") on
 *   the host before any launch; grad_cbsr [num_cols, dim_k] is fully written; inputs are never
 *   written; nothing else is touched.  No atomics.
 * Argument errors (num_heads outside [1, MAXK_MAX_HEADS], a null pointer, k / D range, negative
 *   sizes): MAXK_ERR_INVALID with a message naming the argument, before any launch.
 * chunk_edges: tokens per wavefront work item of both phases, 0 = the csc backward's auto rule.
 * ------------------------------------------------------------------------- */
size_t maxk_sspmm_backward_heads_workspace_size(int64_t num_rows, int64_t num_cols,
                                                int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                                int32_t num_heads, int32_t chunk_edges);
int maxk_sspmm_backward_heads(const int32_t *row_ptr, const int32_t *col_idx,
                              const float *edge_val, const float *grad_out, const float *row_div,
                              const uint8_t *cbsr_idx, const int32_t *col_ptr,
                              const int32_t *csc_eid, float *grad_cbsr, int64_t num_rows,
                              int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
                              int32_t num_heads, int32_t chunk_edges, void *workspace,
                              size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Max aggregation on CBSR features.  With X = scatter(CBSR) [num_cols, dim_origin] (zeros where
 * a row keeps nothing):
 *   out[r, j] = max over the edges e of row r of X[col_idx[e], j]     0 for a row without edges
 *   arg[r, j] = the CSR edge index of the winner, or -1
 * Candidates of (r, j): the row's edges whose column keeps j, in CSR order.  A repeated selector
 * is folded into its first occurrence, which carries the sum of the values in l order (as for
 * the sums); a selector >= dim_origin is no candidate.  The first candidate with the largest
 * value wins (strict >: the lower edge index wins a tie, and -0.0 ties +0.0).  If at least one
 * edge of the row does not keep j, its implicit +0.0 competes: it wins only when 0 > best
 * strictly, or when there is no candidate at all -- an explicit value wins a tie against it --
 * and then arg = -1 and out = +0.0; a row without edges has arg = -1 too.  out carries the
 * winner's bits (the sign of a winning -0.0 is kept).  A NaN candidate wins over everything, the
 * first NaN in edge order (torch's amax rule); out is then a quiet NaN, not the candidate's
 * payload.  +Inf and -Inf order as values.
 * arg may be NULL: no winners are stored (inference; saves 4 * num_rows * dim_origin bytes).
 * Every element of out and, when given, of arg is written; num_e == 0 writes zeros and -1.
 * Contract: the maximum is exact and the tie rule is stated in edge order, so out and arg are
 * bitwise independent of chunk_edges, of where a hub row is cut over work items and of what
 * the workspace held.
 * Shapes: any 1 <= dim_k <= dim_origin <= 256, num_rows != num_cols allowed; a table past 2^24
 * columns or 4 GiB of packed records is rejected.  chunk_edges as maxk_spgemm_forward.
 * workspace: packed CBSR records + two key rows (8 * dim_origin bytes each) per work item.
 *
 * Backward:
 *   grad_cbsr[c, l] = sum over the edges e = (r <- c), in CSC slot order, of
 *                     [arg[r, cbsr_idx[c,l]] == e] * grad_out[r, cbsr_idx[c,l]]
 * Every slot of the winning edge's column whose selector is j receives the gradient (a repeated
 * selector's slots each do, as in the sums' backward).  A slot with a selector >= dim_origin, a
 * column no edge reads and a slot that never won give an exact 0; a NaN of grad_out at an (r, j)
 * whose arg names another edge or -1 reaches nothing.  Every element of grad_cbsr is written.
 * Bitwise repeatable: no atomics in global memory, each sum runs in CSC slot order in fp32.
 * col_ptr / csc_eid: maxk_transpose_plan's.  The row of every CSC slot is not a planned input:
 * the call derives it from row_ptr into its workspace (4 * num_e bytes).  col_idx is unused and
 * may be NULL.
 * ------------------------------------------------------------------------- */
size_t maxk_spgemm_max_forward_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e,
                                              int32_t dim_origin, int32_t dim_k,
                                              int32_t chunk_edges);
int maxk_spgemm_max_forward(const int32_t *row_ptr, const int32_t *col_idx, const float *cbsr_val,
                            const uint8_t *cbsr_idx, float *out, int32_t *arg, int64_t num_rows,
                            int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
                            int32_t chunk_edges, void *workspace, size_t workspace_bytes,
                            void *stream);
size_t maxk_spgemm_max_backward_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e,
                                               int32_t dim_origin, int32_t dim_k);
int maxk_spgemm_max_backward(const int32_t *row_ptr, const int32_t *col_idx,
                             const int32_t *col_ptr, const int32_t *csc_eid,
                             const uint8_t *cbsr_idx, const int32_t *arg, const float *grad_out,
                             float *grad_cbsr, int64_t num_rows, int64_t num_cols, int64_t num_e,
                             int32_t dim_origin, int32_t dim_k, void *workspace,
                             size_t workspace_bytes, void *stream);

/* Transpose plan of a CSR graph (once per graph): col_ptr[num_cols+1] of the
 * CSC and csc_eid[num_e] = the CSR edge id held by CSC slot t (stable in CSR order).
 * Replaces the CSC side files of generate_meta_csc.py:14-93 /
 * load_warp4_metadata_csc (binding_v2.py:320-351). */
size_t maxk_transpose_plan_workspace_size(int64_t num_cols, int64_t num_e);
int maxk_transpose_plan(const int32_t *col_idx, int64_t num_cols, int64_t num_e,
                        int32_t *col_ptr, int32_t *csc_eid, void *workspace,
                        size_t workspace_bytes, void *stream);

/* Destination buckets (the pull's tiles, the bsort plan, the hybrid plan): buckets of
 * 2^bucket_shift consecutive columns, nb = maxk_bucket_count(num_cols, shift) of them;
 * maxk_bucket_shift(k) is the largest shift the fp64 LDS accumulator of the bucketed phase 2
 * allows for k (-1 for k <= 0).  (r06: the "bucket" backward mode and its plan entry points,
 * which no BASELINE configuration reached, left the library; bsort keeps the bucketed
 * phase 2.) */
int maxk_bucket_shift(int32_t dim_k);
int64_t maxk_bucket_count(int64_t num_cols, int32_t bucket_shift);

/* ---------------------------------------------------------------------------
 * Same backward, two-phase with window-sorted contribution rows ("bsort", dim_k % 4 == 0),
 * for large sparse graphs at small k, where every contribution row phase 2 reads would
 * otherwise cost a whole random 128-B line (ogbn-products k = 8: 32-B rows).  The CSR edges
 * are cut into windows of W = maxk_bsort_window(dim_k) consecutive edges; phase 1 builds a
 * window's rows in LDS (one workgroup per window) and writes them to the window's range of T
 * ordered by destination bucket, so the bucketed phase 2 (one workgroup per part of a
 * bucket's entry list, fp64 LDS sums) reads a bucket's rows of one window as one run.  edge_sel (optional, u8
 * [num_e, k], 4-B aligned; as maxk_sspmm_backward_csc_sel) replaces the cbsr_idx row
 * gathers; cbsr_idx may be NULL when it is given, col_idx when edge_sel is given.
 * Plan (once per graph and k): maxk_bsort_plan with the shift maxk_bucket_shift(k) --
 * bucket_ptr[nb + 1] the start of each bucket's entries, bucket_dst[num_e] (u16) each entry's
 * column minus its bucket's first column, bucket_pos[num_e] the T row of each bucket entry, win_src[num_e] (u16) the edge (relative to its window) whose row T row p holds,
 * edge_row[num_e] the source row of every CSR edge.
 * Meant for dim_k <= MAXK_BSORT_KMAX (8; the auto rule's limit): W * 4 * dim_k bytes fill the LDS
 * stage, so larger k leaves fewer rows per window and bucket (k = 16 on ogbn-products: one
 * row per run, 5.88 ms against 5.07 for csc) down to W = 160 at dim_k = 256, where the mode is
 * correct (tested) but only slower than csc.
 * Replaces the same reference kernels as maxk_sspmm_backward.
 * ------------------------------------------------------------------------- */
int32_t maxk_bsort_window(int32_t dim_k); /* -1 unless dim_k % 4 == 0 in [4, 256] */
size_t maxk_bsort_plan_workspace_size(int64_t num_cols, int64_t num_e);
int maxk_bsort_plan(const int32_t *row_ptr, const int32_t *col_idx, int64_t num_rows,
                    int64_t num_cols, int64_t num_e, int32_t dim_k, int32_t bucket_shift,
                    int32_t *bucket_ptr, int32_t *bucket_pos, uint16_t *bucket_dst,
                    uint16_t *win_src, int32_t *edge_row, void *workspace,
                    size_t workspace_bytes, void *stream);
size_t maxk_sspmm_backward_bsort_workspace_size(int64_t num_rows, int64_t num_cols,
                                                int64_t num_e, int32_t dim_origin,
                                                int32_t dim_k);
int maxk_sspmm_backward_bsort(const int32_t *row_ptr, const int32_t *col_idx,
                              const float *edge_val, const float *grad_out, const float *row_div,
                              const uint8_t *cbsr_idx, const uint8_t *edge_sel,
                              const int32_t *bucket_ptr, const int32_t *bucket_pos,
                              const uint16_t *bucket_dst, const uint16_t *win_src,
                              const int32_t *edge_row, int32_t bucket_shift, float *grad_cbsr,
                              int64_t num_rows,
                              int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
                              void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Backward, pull form (no contribution rows): the same result as maxk_sspmm_backward,
 * summed per tile (row slice x destination bucket of 2^shift columns) from G / row_div
 * gathered directly, fp64 LDS accumulation, then the slices of a bucket added in slice
 * order.  The fp64 tile sums make two runs agree except in rare rounding ties (bitwise
 * repeatability: maxk_sspmm_backward_csc).  For dim_k % 4 == 0 each destination's selectors
 * are first re-ordered by column (quantile slots, sspmm_pull.hip pull_sel_kernel) so one
 * gather instruction touches fewer lines of a row; the sums return to CBSR order at the
 * end.  With dim_k % 4 == 0 a tile's destination slots may be split by sorted rank into
 * parts of kp = dim_k / H slots, one workgroup each, so a bucket holds H times the
 * destinations (kp >= 8 below dim_k = 32, >= 16 from 32; maxk_pull_shift(dim_k) gives the
 * matching shift).  A selector >= dim_origin contributes 0.  Needs dim_k % 4 == 0 or
 * dim_k <= 64, dim_origin % 4 == 0, bucket_shift in [4, min(15, max(maxk_bucket_shift(dim_k),
 * maxk_pull_shift(dim_k)))] (above maxk_bucket_shift(dim_k) only with dim_k % 4 == 0), the pull
 * plan of the graph built with the same shift, slices and edge_val (maxk_pull_plan), and a
 * workspace of maxk_sspmm_backward_pull_workspace_size(...) bytes (G / row_div, slices x
 * num_cols x k floats of tile partials, and 2 x num_cols x k bytes of slot-ordered
 * selectors).  Replaces the same reference kernels as maxk_sspmm_backward
 * (kernels/spmm_maxk_backward.cu:15-121).
 * ------------------------------------------------------------------------- */
size_t maxk_sspmm_backward_pull_workspace_size(int64_t num_rows, int64_t num_cols,
                                               int32_t dim_origin, int32_t dim_k, int32_t slices);
int maxk_sspmm_backward_pull(const float *grad_out, const float *row_div,
                             const uint8_t *cbsr_idx, const int32_t *tile_ptr,
                             const uint32_t *ent, int32_t bucket_shift, int32_t slices,
                             float *grad_cbsr, int64_t num_rows, int64_t num_cols, int64_t num_e,
                             int32_t dim_origin, int32_t dim_k, void *workspace,
                             size_t workspace_bytes, void *stream);

/* The pull over a listed subset of a plan's tiles (dim_k % 4 == 0), for graphs where only
 * some tiles are dense enough to pull (a community-ordered graph: the tiles near the
 * diagonal) and the rest of the edges go through the two-phase backward (the "hybrid" mode
 * of the Python binding).  tile_list[n_tiles]: tile ids t = s*nb + j, increasing;
 * tile_ent[n_tiles + 1]: their entry ranges in ent; bucket_ptr[nb + 1] / bucket_tiles[n_tiles]:
 * per bucket, the positions in tile_list of its tiles in slice order.  accumulate bit 0 adds
 * the result onto grad_cbsr (which then holds the other edges' sum), else stores it;
 * MAXK_PULL_NO_REDUCE stops once the tile partials are in the workspace and
 * MAXK_PULL_REDUCE_ONLY, with otherwise the same arguments and workspace, runs only the
 * reduce onto grad_cbsr, so the tile kernels can run on another stream beside the two-phase
 * form of the other edges, joined before the reduce.  The
 * workspace holds n_tiles tile partials: maxk_sspmm_backward_pull_tiles_workspace_size.
 * Replaces the same reference kernels as maxk_sspmm_backward (spmm_maxk_backward.cu:15-121). */
#define MAXK_PULL_NO_REDUCE 2
#define MAXK_PULL_REDUCE_ONLY 4
size_t maxk_sspmm_backward_pull_tiles_workspace_size(int64_t num_rows, int64_t num_cols,
                                                     int32_t dim_origin, int32_t dim_k,
                                                     int32_t n_tiles);
int maxk_sspmm_backward_pull_tiles(const float *grad_out, const float *row_div,
                                   const uint8_t *cbsr_idx, const int32_t *tile_list,
                                   const int32_t *tile_ent, int32_t n_tiles,
                                   const int32_t *bucket_ptr, const int32_t *bucket_tiles,
                                   const uint32_t *ent, int32_t bucket_shift, int32_t slices,
                                   int32_t accumulate, float *grad_cbsr, int64_t num_rows,
                                   int64_t num_cols, int64_t num_e, int32_t dim_origin,
                                   int32_t dim_k, void *workspace, size_t workspace_bytes,
                                   void *stream);

/* Pull plan of a CSR graph and its edge values (once per graph, shift and slices):
 * tile_ptr[slices*nb + 1] over tiles t = s*nb + j (rows cut into `slices` slices of
 * ceil(num_rows/slices) <= 65536 rows, nb = maxk_bucket_count(num_cols, shift)); per tile,
 * in CSR order, ent[2*num_e] = one uint32 pair per edge: {row - first row of its slice |
 * (column - first column of its bucket) << 16, bits of edge_val}; bucket_shift in [4, 15]
 * (the backward's 16-B selector copies need 16 | 2^shift * k).  maxk_pull_shift(k) is the
 * bucket shift to use (at least 4); maxk_pull_slices(num_rows, num_cols, dim_origin, dim_k) the
 * default
 * slice count (about 3.5 MiB of G rows per slice and rank part of k -- at most 3 parts' worth
 * -- at least num_rows/65536, 1..256; when that makes at most 5 rounds of workgroups, one per
 * CU of the current device, over num_cols' buckets, the count in [ceil(S/2), S] with the
 * fewest rounds; num_cols <= 0 means num_rows). */
int maxk_pull_shift(int32_t dim_k);
int maxk_pull_slices(int64_t num_rows, int64_t num_cols, int32_t dim_origin, int32_t dim_k);
size_t maxk_pull_plan_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e,
                                     int32_t bucket_shift, int32_t slices);
int maxk_pull_plan(const int32_t *row_ptr, const int32_t *col_idx, const float *edge_val,
                   int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t bucket_shift,
                   int32_t slices, int32_t *tile_ptr, uint32_t *ent, void *workspace,
                   size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Backward, pull form, stream path (dim_k % 4 == 0): the same sums as maxk_sspmm_backward_pull
 * with one workgroup per (destination bucket, part) for the whole call.  A bucket's entries
 * are walked front to back in CSR order, the fp64 sums stay in LDS until the workgroup stores
 * its own rows of grad_cbsr: no tile partials, no reduce kernel.  Every row of grad_cbsr is
 * written (zeros where no edge arrives).  Two runs agree as for the tiled pull; against it the
 * result differs by one fp32 rounding of an fp64 sum (the tiled pull rounds each slice's sum).
 *
 * maxk_pull_stream_buckets: the number of buckets the path uses for a shape, or 0 where it does
 *   not apply and the tiled pull stays.  With cap = 2^maxk_pull_shift(dim_k) and H parts per
 *   bucket, the fewest workgroups are ceil(num_cols / cap) * H; they are rounded up to whole
 *   rounds of `cus` workgroups (cus <= 0: the current device's CU count), which narrows the mean
 *   bucket; 0 when that narrows it by more than 12.5 %, when dim_k % 4 or dim_origin % 4 != 0,
 *   when G has 2^31 bytes or more (num_rows * dim_origin * 4), when num_e >= 2^28 (num_e < 0:
 *   unknown, not checked) or when the bits of num_rows - 1 plus maxk_pull_shift(dim_k) exceed
 *   32.  Callable without a device when cus > 0.
 * maxk_pull_stream_plan (once per graph, edge_val, dim_k, n_buckets and slices):
 *   bucket_col[n_buckets + 1], increasing from 0 to num_cols, every width <= cap, chosen on the
 *   prefix sum of the in-degrees so that the buckets hold as nearly as possible equal edge
 *   counts (a width that balance would push past cap is clamped); grp_ptr[n_buckets + 1], the
 *   buckets' entry ranges; ent[2 * num_e], per bucket the edges ordered by (slice of
 *   ceil(num_rows / slices) source rows, CSR order), one uint32 pair each: {row <<
 *   maxk_pull_shift(dim_k) | column - bucket_col[b], bits of edge_val}.  n_buckets * cap >=
 *   num_cols.  The slices only widen the sort key (CSR order is row order, so a bucket's
 *   entries come out in CSR order whatever their count); maxk_pull_stream_slices gives 1.
 * maxk_pull_stream_entries_scale: ent_out = ent with every weight divided by its row's
 *   row_div, once per (plan, divisor), so the backward gathers G itself.
 * maxk_sspmm_backward_pull_stream: the backward over such a plan; n_buckets need not come from
 *   maxk_pull_stream_buckets.  With row_div != NULL it gathers from a G / row_div copy in the
 *   workspace, as the tiled pull.
 * Memory: the workspace (maxk_sspmm_backward_pull_stream_workspace_size) holds the G / row_div
 *   copy (num_rows x dim_origin floats) and 2 x num_cols x dim_k bytes of slot-ordered selectors
 *   and their map; the tiled pull's slices x num_cols x dim_k floats of tile partials (417 MB
 *   for a Reddit-sized graph at dim_k = 16) are not needed.  The plan takes what a pull plan
 *   takes (8 bytes per edge) plus 8 bytes per bucket.
 * Replaces the same reference kernels as maxk_sspmm_backward (spmm_maxk_backward.cu:15-121).
 * ------------------------------------------------------------------------- */
int64_t maxk_pull_stream_buckets(int64_t num_rows, int64_t num_cols, int64_t num_e,
                                 int32_t dim_origin, int32_t dim_k, int32_t cus);
int maxk_pull_stream_slices(int64_t num_rows, int64_t num_cols, int32_t dim_origin,
                            int32_t dim_k);
size_t maxk_pull_stream_plan_workspace_size(int64_t num_cols, int64_t num_e, int32_t n_buckets,
                                            int32_t slices);
int maxk_pull_stream_plan(const int32_t *row_ptr, const int32_t *col_idx, const float *edge_val,
                          int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_k,
                          int32_t n_buckets, int32_t slices, int32_t *bucket_col,
                          int32_t *grp_ptr, uint32_t *ent, void *workspace,
                          size_t workspace_bytes, void *stream);
int maxk_pull_stream_entries_scale(const uint32_t *ent, int64_t num_e, int64_t num_rows,
                                   int32_t dim_k, const float *row_div, uint32_t *ent_out,
                                   void *stream);
size_t maxk_sspmm_backward_pull_stream_workspace_size(int64_t num_rows, int64_t num_cols,
                                                      int32_t dim_origin, int32_t dim_k);
int maxk_sspmm_backward_pull_stream(const float *grad_out, const float *row_div,
                                    const uint8_t *cbsr_idx, const int32_t *bucket_col,
                                    const int32_t *grp_ptr, const uint32_t *ent,
                                    int32_t n_buckets, float *grad_cbsr, int64_t num_rows,
                                    int64_t num_cols, int64_t num_e, int32_t dim_origin,
                                    int32_t dim_k, void *workspace, size_t workspace_bytes,
                                    void *stream);

/* ---------------------------------------------------------------------------
 * Dense route (r05): wide top-k, dim_k >= dim_origin / 2 at dim_origin % 4 == 0,
 * dim_origin <= 128 (MAXK_DENSE_DMAX), dim_k % 4 == 0.  A CBSR row then carries as many bytes as
 * the dense row, so both directions aggregate dense rows.  Replaces the same reference kernels
 * as maxk_spgemm_forward / maxk_sspmm_backward (spmm_maxk.cu:17-106,
 * spmm_maxk_backward.cu:15-121) for those widths; results within fp32 rounding of them.
 *
 * maxk_dense_route: 1 when (dim_origin, dim_k) takes the route.  maxk_spgemm_forward takes it
 *   by itself there (16-B aligned cbsr_val and out, 4-B aligned cbsr_idx; not the _sel forms):
 *   the CBSR scattered into a dense [num_cols, dim_origin] table in the workspace, then one
 *   dense row walk (maxk_spgemm_forward_workspace_size covers it).
 * maxk_dense_plan: the graph's transpose with source rows -- for every CSC slot t of
 *   maxk_transpose_plan (col_ptr, csc_eid), t_src[t] = the CSR row holding edge csc_eid[t] and
 *   t_w[t] = edge_val[csc_eid[t]] (int32 / float [num_e]).  Once per graph and weights.
 * maxk_sspmm_backward_dense: grad_cbsr[c, l] = (A^T diag(1/row_div) G)[c, cbsr_idx[c, l]] from
 *   the transpose plan, walked destination by destination: at dim_k >= dim_origin / 2 over dense
 *   G rows, each finished row stored as its k selected columns; below that (dim_k <= 64) one
 *   selected column per lane, G[src, sel[c, l]] gathered per edge (selectors >= dim_origin read
 *   0).  Any dim_k % 4 == 0 <= dim_origin; the route's rule (maxk_dense_route) is where "auto"
 *   takes it.  Bitwise repeatable.  16-B aligned grad_out and grad_cbsr, 4-B aligned cbsr_idx.
 * ------------------------------------------------------------------------- */
int maxk_dense_route(int32_t dim_origin, int32_t dim_k);
int maxk_dense_plan(const int32_t *row_ptr, const float *edge_val, const int32_t *csc_eid,
                    int64_t num_rows, int64_t num_e, int32_t *t_src, float *t_w, void *stream);
size_t maxk_sspmm_backward_dense_workspace_size(int64_t num_rows, int64_t num_cols,
                                                int64_t num_e, int32_t dim_origin, int32_t dim_k,
                                                int32_t chunk_edges);
int maxk_sspmm_backward_dense(const int32_t *col_ptr, const int32_t *t_src, const float *t_w,
                              const float *grad_out, const float *row_div,
                              const uint8_t *cbsr_idx, float *grad_cbsr, int64_t num_rows,
                              int64_t num_cols, int64_t num_e, int32_t dim_origin, int32_t dim_k,
                              int32_t chunk_edges, void *workspace, size_t workspace_bytes,
                              void *stream);

/* ---------------------------------------------------------------------------
 * Hybrid backward and the "auto" backward rule through the C ABI (the Python binding's
 * hybrid_plan / pull_locality / _bwd_mode / _scaled_entries, maxk_cuda_kernels/__init__.py,
 * rest on these).  Replaces the same reference kernels as maxk_sspmm_backward
 * (spmm_maxk_backward.cu:15-121, launched by cuda_kernel_wrappers.cu:58-76).
 *
 * maxk_backward_mode_auto: the backward a graph should use (pure host arithmetic):
 *   MAXK_BWD_DENSE where maxk_dense_route(dim_origin, dim_k), or (its selected-column form)
 *   for a G of at most 64 MiB on a graph below the pull's density test at dim_origin <= 64,
 *   dim_origin / 4 <= dim_k < dim_origin / 2, both % 4 == 0; else MAXK_BWD_PULL where
 *   dim_k % 4 == 0 or dim_k <= 64, dim_origin % 4 == 0 and the graph has at
 *   least ~1/2 edge per (source row, bucket of 2^maxk_bucket_shift(dim_k) columns) or a G of at
 *   most 64 MiB (and at most 256 x 65536 rows); else MAXK_BWD_HYBRID
 *   when pull_locality (maxk_pull_locality at maxk_pull_shift(dim_k); < 0 = unknown) reaches
 *   MAXK_HYBRID_LOCALITY and dim_k % 4 == 0; else MAXK_BWD_BSORT at dim_k % 4 == 0,
 *   dim_k <= MAXK_BSORT_KMAX when a window of maxk_bsort_window(dim_k) edges holds at least 2
 *   rows per destination bucket on average (W * 2^maxk_bucket_shift(dim_k) >= 2 * num_cols;
 *   ogbn-products k = 8: 4.3); else MAXK_BWD_CSC.  Only csc and dense are bitwise
 *   repeatable.
 * maxk_pull_locality (synchronous): num_e / occupied (source row, bucket of 2^bucket_shift
 *   columns) pairs, columns sorted within rows; workspace >= 8 bytes.
 * maxk_hybrid_plan (synchronous): from the graph's pull plan (maxk_pull_plan with bucket_shift,
 *   slices), the tiles holding at least density x (rows of their slice) entries --
 *   tile_list[S*nb] (increasing tile ids), tile_ent[S*nb+1] (their runs in ent_pull[2*num_e]),
 *   bucket_ptr[nb+1] / bucket_tiles[S*nb] (per bucket, positions in tile_list in slice order)
 *   -- and every other edge as a CSR off_row_ptr[num_rows+1] / off_col[num_e] / off_val[num_e]
 *   (CSR order kept).  counts[3] = {tiles pulled, entries pulled, edges off}.  Buffers are
 *   sized for the worst case; the counts say how much of each holds the plan.
 * maxk_pull_entries_scale: ent_out = ent with each weight divided by its source row's
 *   row_div, for n_runs tile runs (tile_ids[i], or i when NULL; entries tile_ent[i] ..
 *   tile_ent[i+1]) -- once per (plan, divisor), so the pull gathers G instead of G / row_div.
 * maxk_sspmm_backward_hybrid: the csc backward over the off-tile CSR (its transpose plan:
 *   maxk_transpose_plan of off_col) and the listed-tile pull over the rest, accumulated into
 *   grad_cbsr.  With side_stream (and two caller-created events ev_fork / ev_join, as void*)
 *   the tile kernels run beside the csc and are joined before the final reduce; NULL runs
 *   everything on `stream`.  flags: MAXK_HYBRID_PRESCALED when ent_pull carries row_div.
 * ------------------------------------------------------------------------- */
#define MAXK_BWD_PULL 0
#define MAXK_BWD_CSC 1
/* 2 was MAXK_BWD_BUCKET (removed in r06); the code stays unused */
#define MAXK_BWD_HYBRID 3
#define MAXK_BWD_ATOMIC 4
#define MAXK_BWD_BSORT 5
#define MAXK_BWD_DENSE 6
#define MAXK_BSORT_KMAX 8
#define MAXK_HYBRID_LOCALITY 1.5
#define MAXK_HYBRID_DENSITY 0.5f
#define MAXK_HYBRID_PRESCALED 1
int maxk_backward_mode_auto(int64_t num_rows, int64_t num_cols, int64_t num_e, int32_t dim_origin,
                            int32_t dim_k, double pull_locality);
int maxk_pull_locality(const int32_t *row_ptr, const int32_t *col_idx, int64_t num_rows,
                       int64_t num_e, int32_t bucket_shift, double *locality, void *workspace,
                       size_t workspace_bytes, void *stream);
size_t maxk_hybrid_plan_workspace_size(int64_t num_rows, int64_t num_cols, int64_t num_e,
                                       int32_t bucket_shift, int32_t slices);
int maxk_hybrid_plan(const int32_t *row_ptr, const int32_t *col_idx, const float *edge_val,
                     const int32_t *tile_ptr, const uint32_t *ent, int64_t num_rows,
                     int64_t num_cols, int64_t num_e, int32_t bucket_shift, int32_t slices,
                     float density, int32_t *tile_list, int32_t *tile_ent, int32_t *bucket_ptr,
                     int32_t *bucket_tiles, uint32_t *ent_pull, int32_t *off_row_ptr,
                     int32_t *off_col, float *off_val, int64_t *counts, void *workspace,
                     size_t workspace_bytes, void *stream);
int maxk_pull_entries_scale(const uint32_t *ent, const int32_t *tile_ids, const int32_t *tile_ent,
                            int64_t n_runs, int64_t num_rows, int64_t num_cols,
                            int32_t bucket_shift, int32_t slices, const float *row_div,
                            uint32_t *ent_out, void *stream);
size_t maxk_sspmm_backward_hybrid_workspace_size(int64_t num_rows, int64_t num_cols,
                                                 int64_t n_off_e, int32_t dim_origin,
                                                 int32_t dim_k, int64_t n_tiles);
int maxk_sspmm_backward_hybrid(
    const float *grad_out, const float *row_div, const uint8_t *cbsr_idx,
    const int32_t *tile_list, const int32_t *tile_ent, int32_t n_tiles, const int32_t *bucket_ptr,
    const int32_t *bucket_tiles, const uint32_t *ent_pull, int64_t n_pull_e, int32_t bucket_shift,
    int32_t slices, const int32_t *off_row_ptr, const int32_t *off_col, const float *off_val,
    int64_t n_off_e, const int32_t *off_col_ptr, const int32_t *off_csc_eid, int32_t flags,
    float *grad_cbsr, int64_t num_rows, int64_t num_cols, int32_t dim_origin, int32_t dim_k,
    void *workspace, size_t workspace_bytes, void *stream, void *side_stream, void *ev_fork,
    void *ev_join);

/* ---------------------------------------------------------------------------
 * CBSR encode (MaxK top-k): per row the k largest of dim_origin values, in
 * torch.topk(largest=True, sorted=True) order (value descending; NaN largest;
 * equal values by ascending column).  x has leading dimension ld_x (elements).
 * Replaces: torch.topk + .to(uint8) in maxk_spgemm_function.py:51-57 and the
 *           uint8 kernel topk (kernels/maxk_kernel.cu:23-96) behind
 *           cuda_topk_maxk / cuda_topk_maxk_float (cuda_kernel_bindings.cpp:164-238).
 * maxk_topk_cbsr_u8: the same on uint8 input (values copied as uint8).
 * idx32 (optional, may be NULL): the same indices widened to int32.
 * ------------------------------------------------------------------------- */
int maxk_topk_cbsr(const float *x, int64_t ld_x, float *cbsr_val, uint8_t *cbsr_idx,
                   int32_t *idx32, int64_t num_rows, int32_t dim_origin, int32_t dim_k,
                   void *stream);
int maxk_topk_cbsr_u8(const uint8_t *x, int64_t ld_x, uint8_t *cbsr_val, uint8_t *cbsr_idx,
                      int32_t *idx32, int64_t num_rows, int32_t dim_origin, int32_t dim_k,
                      void *stream);
/* The reference uint8 top-k's intended per-row convention (kernels/maxk_kernel.cu:23-94,
 * behind cuda_topk_maxk / cuda_topk_maxk_float, cuda_kernel_bindings.cpp:164-238), for callers
 * that depend on its layout: rows of dim_origin == 256 bytes; each row's threshold from 8
 * bisection steps on [0, 255] over its own bytes; the bytes strictly above it in ascending
 * column order, 32 columns per step, at most dim_k, a pick in column 32s + 31 overwritten by the
 * next step's first pick (the reference counts a step's picks without its lane 31); slots never
 * filled are 0.  val / idx uint8 [num_rows, dim_k].  NOT the CUDA kernel's as-built output: that
 * kernel thresholds every row on its block's first row, per lane (:42, :44-48), racily, and
 * leaves unfilled slots uninitialised; parity with it is unpinned (oracle/oracle.py
 * topk_u8_reference_as_built models it).  Not torch.topk: maxk_topk_cbsr_u8 is the exact one. */
int maxk_topk_u8_reference(const uint8_t *x, uint8_t *val, uint8_t *idx, int64_t num_rows,
                           int32_t dim_origin, int32_t dim_k, void *stream);
/* Rows (over every top-k launch on the current device since the last reset) whose threshold
 * search took other than dim_k winners -- a kernel bug, never expected.  The kernels count such
 * rows, and such a row never writes past its own k winner slots (r02's fault: a dead row's
 * extra winners overwrote another wave's); its own output row is then undefined.  Read (and,
 * with reset != 0, zeroed) in order on `stream`, which it synchronises (not the device, so a
 * hipGraph capture on another stream is left alone).  The Python binding zeroes it before
 * and reads it after every top-k under MAXK_VALIDATE=1, so a count is the launch's own. */
int maxk_topk_error_rows(int64_t *rows, int32_t reset, void *stream);

/* dense[r,:] = 0; dense[r, cbsr_idx[r,l]] = cbsr_val[r,l]  (all of dense written).
 * Replaces: zeros(V,D).scatter_(1, sel, grad_sparse), maxk_spgemm_function.py:152,175. */
int maxk_cbsr_scatter_dense(const float *cbsr_val, const uint8_t *cbsr_idx, float *dense,
                            int64_t num_rows, int32_t dim_origin, int32_t dim_k, void *stream);

/* Fused MaxK activation, forward: maxk_topk_cbsr plus the masked dense output
 * dense[r, j] = x[r, j] if j is among row r's k winners, else 0 (row stride dim_origin),
 * written by the same kernel from the row it already holds.
 * Replaces: MaxK.forward, topk + zeros_like + scatter_ (model_integrated_v3.py:28-38),
 *           i.e. the top-k pass plus two dense V x D passes. */
int maxk_topk_cbsr_dense(const float *x, int64_t ld_x, float *cbsr_val, uint8_t *cbsr_idx,
                         float *dense, int64_t num_rows, int32_t dim_origin, int32_t dim_k,
                         void *stream);

/* Fused MaxK activation, backward, in one pass over the rows:
 *   grad_x[r, :] = 0;  grad_x[r, j] = grad_val[r, l] + grad_dense[r, j]  for j = cbsr_idx[r, l].
 * grad_val [V,k] and grad_dense [V,D] are each optional (NULL = zero); grad_x may alias
 * grad_dense.  Selectors of a row are distinct (top-k output); with duplicates one of them wins.
 * Replaces: OPTMaxK.backward's mask multiply (model_integrated_v3.py:39-43) together with
 *           zeros(V,D).scatter_(1, sel, grad_sparse) (maxk_spgemm_function.py:152,175). */
int maxk_topk_backward(const float *grad_val, const float *grad_dense, const uint8_t *cbsr_idx,
                       float *grad_x, int64_t num_rows, int32_t dim_origin, int32_t dim_k,
                       void *stream);

/* ---------------------------------------------------------------------------
 * warp4 schedule (drop-in for kernels/generate_meta.py:30-48 / generate_meta_csc.py:14-93
 * and the .warp4 files read by load_warp4_metadata, cuda_kernel_bindings.cpp:287-317).
 * maxk_warp4_count: synchronous; number of entries W = sum over rows of ceil(deg/warp_max_nz).
 * maxk_warp4_build: fills warp4[W*4] on the stream; needs
 *   maxk_warp4_build_workspace_size(num_rows) bytes of workspace.
 * maxk_warp4_to_row_ptr: recovers the CSR row_ptr[num_rows+1] a warp4 array
 *   describes (rows absent from it are empty); lets the reference's
 *   spmm_maxk_forward(warp4, ...) signature drive the CSR kernels.
 * ------------------------------------------------------------------------- */
int maxk_warp4_count(const int32_t *row_ptr, int64_t num_rows, int32_t warp_max_nz,
                     int64_t *num_entries, void *stream);
size_t maxk_warp4_build_workspace_size(int64_t num_rows);
int maxk_warp4_build(const int32_t *row_ptr, int64_t num_rows, int32_t warp_max_nz,
                     int32_t *warp4, int64_t num_entries, void *workspace,
                     size_t workspace_bytes, void *stream);
int maxk_warp4_to_row_ptr(const int32_t *warp4, int64_t num_entries, int64_t num_rows,
                          int32_t *row_ptr, void *stream);

/* ---------------------------------------------------------------------------
 * Dense SpMM baseline Y = A . X on rocSPARSE (the speed-up denominator; the
 * MI355X equivalent of spmm_cusparse, kernels/spmm_cusparse.cu:6-62, and of
 * the cusparse_spmm binding, cuda_kernel_bindings.cpp:253-284).
 * A plan owns the rocSPARSE handle, descriptors and buffer (synchronous to
 * create); maxk_dense_spmm_run only launches (alpha=1, beta=0).
 * ------------------------------------------------------------------------- */
typedef struct maxk_dense_spmm_plan maxk_dense_spmm_plan;
int maxk_dense_spmm_plan_create(maxk_dense_spmm_plan **plan, const int32_t *row_ptr,
                                const int32_t *col_idx, const float *edge_val, const float *x,
                                float *y, int64_t num_rows, int64_t num_cols, int64_t num_e,
                                int32_t dim, int32_t alg, void *stream);
int maxk_dense_spmm_run(maxk_dense_spmm_plan *plan, void *stream);
/* Point the plan at new X / Y buffers of the same shape (one plan per graph serves every
 * call, as cusparseSpMM's descriptors do in the reference's callers). */
int maxk_dense_spmm_bind(maxk_dense_spmm_plan *plan, const float *x, float *y);
int maxk_dense_spmm_plan_destroy(maxk_dense_spmm_plan *plan);

#ifdef __cplusplus
}
#endif

#endif /* MAXK_HIP_H_ */
