"""maxk_spgemm_function -- drop-in autograd surface of the MaxK-GNN aggregation.

Mirrors the reference module of the same name (maxk_spgemm_function.py) and its
v4 successor (spgemmfunction_v4): `MAXK_KERNELS_AVAILABLE`,
`MaxKSpGEMMFunction`, `maxk_spgemm`, `MaxKSpmmWrapper`.  Both call shapes are
accepted, told apart by the 4th argument:

  v1  (graph_indices, graph_values, input_features, k_value:int,
       warp4_metadata=None, num_warps=0, graph_indptr=None, in_degrees=None,
       out_degrees=None, graph_indices_T=None, graph_values_T=None)
      -> dense [V, D] = A . topk_scatter(input_features) / in_degrees;
         grad w.r.t. input_features (maxk_spgemm_function.py:26-184)
  v4  (graph_indices, graph_values, topk_values, topk_indices:Tensor,
       warp4_metadata, num_warps, graph_indptr, degrees[, dim_origin])
      -> dense [V, 256] = A . scatter(topk) / degrees;
         grad w.r.t. topk_values (spgemmfunction_v4:26-101)

All compute runs in the HIP kernels of maxk_cuda_kernels (libmaxk_hip.so):
top-k/CBSR encode, forward SpGEMM with the degree division fused into its
write-back, backward SSpMM with the division fused into its G staging, and the
CBSR->dense gradient scatter.  When the extension is missing,
MAXK_KERNELS_AVAILABLE is False and every call raises -- there is no
torch.sparse / cuSPARSE fallback (a CPU fallback would void parity).

Fixed caller-visible defects of the reference (DESIGN.md "Boundary"):
  * v1 backward unpacked 7 saved tensors out of 3 (ValueError); here it works;
  * the v1 backward divides by the same per-row divisor the forward used, so the
    gradient is the exact adjoint; the reference divides G by out_degrees instead
    (maxk_spgemm_function.py:154-159), which is the same on the symmetric graphs it
    targets (in == out).  `backward_divisor="reference"` (keyword of maxk_spgemm /
    MaxKSpmmWrapper.spmm, or the 12th apply() argument) reproduces the reference's
    rule on any graph: G / out_degrees when given, else G undivided;
  * graph_indices_T / graph_values_T are accepted and unused: the kernel forms
    the A^T product from the CSR itself.

Edge weights that require grad (attention coefficients, learned gates, a learnable
normalisation): both call shapes return d out / d graph_values, in graph_values' dtype and
shape (maxk_cuda_kernels.edge_weight_grad; the reference returns None).  The forward then also
saves the CBSR values and its own divisor -- nothing extra otherwise.  The weight gradient
always divides by the forward's divisor: it is the exact adjoint, and
`backward_divisor="reference"` changes only the feature gradient.  With such weights and no
mode forced through MAXK_BWD_MODE, the feature backward is resolved among the modes whose plans
depend on the graph alone ("bsort" where its rule holds, else "csc":
maxk_cuda_kernels.graph_only_mode), because the pull, dense and hybrid plans embed the weights
and would be rebuilt on every step.
"""
from __future__ import annotations

import weakref
from typing import Optional

import torch
from torch.autograd import Function

try:
    import maxk_cuda_kernels
    MAXK_KERNELS_AVAILABLE = True
except ImportError as _exc:  # the reference prints and degrades; we refuse to compute
    maxk_cuda_kernels = None
    MAXK_KERNELS_AVAILABLE = False
    _IMPORT_ERROR = str(_exc)

FULL_DIM = 256


def _require_kernels():
    if not MAXK_KERNELS_AVAILABLE:
        raise RuntimeError("MaxK HIP kernels (maxk_cuda_kernels / libmaxk_hip.so) are not "
                           f"available: {_IMPORT_ERROR}")


_CONVERTED: dict = {}


def _converted(src, tag, make):
    """make(src), cached per source tensor object and version: the backward's plans and the
    auto mode's locality pass are cached on the identity of the int32 / fp32 tensors they see,
    so an int64 indptr, a warp4 array or float64 values converted afresh every step would
    rebuild them (and re-synchronise the host) on every call.  Graph-side tensors
    only (indices, indptr, edge values, warp4, degrees): activations are converted uncached
    (_f32_act), so no fp32 copy of a [V, D] input outlives its call.

    Under torch.inference_mode (an evaluation pass over a graph loaded outside it) the
    conversion is made with inference mode off: a normal tensor, versioned, so this cache and
    the plan / graph-check caches keyed on it hit on every later call.  An
    inference tensor itself (a graph built inside inference mode) has no version counter and
    can still change in place there: it is converted afresh on every call, and the caches
    downstream of it miss -- one conversion, one host-synchronising graph check and, for the
    pull / csc backward, one plan build per call; build the graph outside inference mode to
    avoid that."""
    if src.is_inference():
        return make(src)
    key = (id(src), tag)
    hit = _CONVERTED.get(key)
    if hit is not None:
        ref, ver, out = hit
        if ref() is src and ver == src._version:
            return out
    if torch.is_inference_mode_enabled():
        with torch.inference_mode(False):
            out = make(src)
    else:
        out = make(src)
    if out is src:  # nothing converted: the caller's own tensor, no cache entry needed
        return out
    if key not in _CONVERTED:
        weakref.finalize(src, _CONVERTED.pop, key, None)
    _CONVERTED[key] = (weakref.ref(src), src._version, out)
    return out


def _i32(t):
    if t.dtype == torch.int32 and t.is_contiguous():
        return t
    return _converted(t, "i32", lambda u: u.int().contiguous())


def _indptr_for(graph_indptr, warp4_metadata, num_warps, num_v):
    if graph_indptr is not None:
        return _i32(graph_indptr)
    if warp4_metadata is None:
        raise RuntimeError("MaxK SpGEMM needs graph_indptr or warp4_metadata")
    return _converted(warp4_metadata, ("warp4", int(num_v), int(num_warps or 0)),
                      lambda w: maxk_cuda_kernels.warp4_to_indptr(w, num_v, num_warps or None))


def _f32(t):
    """Graph-side fp32 tensor (edge values, degrees), conversion cached per source tensor."""
    if t is None:
        return None
    if t.dtype == torch.float32 and t.is_contiguous():
        return t
    return _converted(t, "f32", lambda u: u.float().contiguous())


def _f32_act(t):
    """Activation (input features, top-k values): converted afresh, never cached."""
    if t.dtype == torch.float32 and t.is_contiguous():
        return t
    return t.float().contiguous()


def _edge_sel_for(indptr, indices, k, num_cols, D, bwd_mode=None):
    """(buffer, mode): the [E, k] u8 buffer the forward writes each edge's selectors into
    when the backward will be a two-phase form reading them ("csc" or "bsort",
    maxk_cuda_kernels.edge_selector_mode), else (None, None).  bwd_mode: the backward's mode
    where the forward has fixed it already (_weight_grad_mode)."""
    mode = maxk_cuda_kernels.edge_selector_mode(indptr, indices, k, num_cols, D, bwd_mode)
    if mode is None:
        return None, None
    return torch.empty(indices.numel(), k, dtype=torch.uint8, device=indices.device), mode


def _weight_grad_mode(ctx, indices, k, num_cols):
    """ctx.wgrad: the edge weights (apply() argument 1) require grad; ctx.bwd_mode: then the
    feature backward's mode among those whose plans depend on the graph alone
    (maxk_cuda_kernels.graph_only_mode), None otherwise or when MAXK_BWD_MODE forces one."""
    ctx.wgrad = bool(ctx.needs_input_grad[1])
    ctx.bwd_mode = (maxk_cuda_kernels.graph_only_mode(k, indices.numel(), num_cols)
                    if ctx.wgrad else None)
    return ctx.bwd_mode


def _save(ctx, base, cbsr_val, fwd_div):
    """The backward's operands; with differentiable edge weights also the CBSR values and the
    forward's own divisor (the weight gradient is the exact adjoint whatever divides G)."""
    ctx.has_fwd_div = fwd_div is not None
    if ctx.wgrad:
        base = base + (cbsr_val, fwd_div if fwd_div is not None else torch.empty(0))
    ctx.save_for_backward(*base)


class MaxKSpGEMMFunction(Function):
    """Autograd function over the HIP forward SpGEMM / backward SSpMM (both call shapes)."""

    @staticmethod
    def forward(ctx, graph_indices, graph_values, a3, a4, *rest):
        _require_kernels()
        graph_indices = _i32(graph_indices)
        if isinstance(a4, torch.Tensor):
            out = MaxKSpGEMMFunction._forward_v4(ctx, graph_indices, graph_values, a3, a4, *rest)
        else:
            out = MaxKSpGEMMFunction._forward_v1(ctx, graph_indices, graph_values, a3, a4, *rest)
        ctx.n_inputs = 4 + len(rest)  # backward returns one grad per apply() argument
        return out

    # ---- v1: dense input + int k ------------------------------------------------
    @staticmethod
    def _forward_v1(ctx, graph_indices, graph_values, input_features, k_value,
                    warp4_metadata=None, num_warps=0, graph_indptr=None, in_degrees=None,
                    out_degrees=None, graph_indices_T=None, graph_values_T=None,
                    backward_divisor=None):
        x = _f32_act(input_features)
        V, D = x.shape
        k = int(k_value)
        if k < D:
            sparse_data, sparse_selector = maxk_cuda_kernels.topk_cbsr(x, k)
        else:  # k >= D: all features, identity selector (maxk_spgemm_function.py:58-63)
            k = D
            sparse_data = x
            sparse_selector = torch.arange(D, device=x.device, dtype=torch.uint8) \
                .unsqueeze(0).expand(V, -1).contiguous()
        indptr = _indptr_for(graph_indptr, warp4_metadata, num_warps, V)
        row_div = _f32(in_degrees)
        if backward_divisor not in (None, "adjoint", "reference"):
            raise ValueError(f"backward_divisor must be 'adjoint' or 'reference', "
                             f"got {backward_divisor!r}")
        # the backward's divisor of G's rows: the forward's own (the exact adjoint), or the
        # reference's rule, G / out_degrees when given and G undivided otherwise (:154-159)
        bwd_div = _f32(out_degrees) if backward_divisor == "reference" else row_div
        es, ctx.es_mode = _edge_sel_for(indptr, graph_indices, k, V, D,
                                        _weight_grad_mode(ctx, graph_indices, k, V))
        out = maxk_cuda_kernels.spgemm_forward(indptr, graph_indices, _f32(graph_values),
                                               sparse_data, sparse_selector, D, row_div=row_div,
                                               edge_sel_out=es)
        ctx.shape_v1 = (V, D)
        _save(ctx, (indptr, graph_indices, graph_values, sparse_selector,
                    bwd_div if bwd_div is not None else torch.empty(0),
                    es if es is not None else torch.empty(0)), sparse_data, row_div)
        ctx.has_div = bwd_div is not None
        ctx.has_es = es is not None
        ctx.mode = "v1"
        return out

    # ---- v4: precomputed top-k + degrees ---------------------------------------------
    @staticmethod
    def _forward_v4(ctx, graph_indices, graph_values, topk_values, topk_indices,
                    warp4_metadata=None, num_warps=0, graph_indptr=None, degrees=None,
                    dim_origin=None):
        vals = _f32_act(topk_values)
        sel = topk_indices if topk_indices.dtype == torch.uint8 else topk_indices.to(torch.uint8)
        sel = sel.contiguous()
        V, k = vals.shape
        D = int(dim_origin) if dim_origin is not None else FULL_DIM
        indptr = _indptr_for(graph_indptr, warp4_metadata, num_warps, V)
        row_div = _f32(degrees)
        es, ctx.es_mode = _edge_sel_for(indptr, graph_indices, k, V, D,
                                        _weight_grad_mode(ctx, graph_indices, k, V))
        out = maxk_cuda_kernels.spgemm_forward(indptr, graph_indices, _f32(graph_values), vals,
                                               sel, D, row_div=row_div, edge_sel_out=es)
        _save(ctx, (indptr, graph_indices, graph_values, sel,
                    row_div if row_div is not None else torch.empty(0),
                    es if es is not None else torch.empty(0)), vals, row_div)
        ctx.has_div = row_div is not None
        ctx.has_es = es is not None
        ctx.mode = "v4"
        return out

    @staticmethod
    def backward(ctx, grad_output):
        indptr, graph_indices, graph_values, sel, row_div, es = ctx.saved_tensors[:6]
        row_div = row_div if ctx.has_div else None
        g = grad_output.contiguous()
        if g.dtype != torch.float32:
            g = g.float()
        # with the forward's edge-selector stream the backward is the two-phase form (csc or
        # bsort) the forward resolved, reading it; with differentiable edge weights, the
        # graph-only mode the forward resolved
        grad_sparse = maxk_cuda_kernels.sspmm_backward(
            indptr, graph_indices, _f32(graph_values), g, sel, row_div=row_div,
            edge_sel=es if ctx.has_es else None,
            mode=ctx.es_mode if ctx.has_es else ctx.bwd_mode)
        grads = [None] * ctx.n_inputs
        if ctx.wgrad:
            cbsr_val, fwd_div = ctx.saved_tensors[6:8]
            grad_edge = maxk_cuda_kernels.edge_weight_grad(
                indptr, graph_indices, cbsr_val, sel, g,
                row_div=fwd_div if ctx.has_fwd_div else None)
            grads[1] = grad_edge.to(graph_values.dtype).reshape(graph_values.shape)
        if ctx.mode == "v1":
            V, D = ctx.shape_v1
            if ctx.needs_input_grad[2]:
                grads[2] = maxk_cuda_kernels.cbsr_scatter_dense(grad_sparse, sel, D)
        else:
            grads[2] = grad_sparse
        return tuple(grads)


def maxk_spgemm(graph_indices, graph_values, a3, a4, *rest, **kw):
    """Both shapes (see module doc):
    v1: maxk_spgemm(graph_indices, graph_values, input_features, k_value, warp4_metadata=None,
                    num_warps=0, graph_indptr=None, in_degrees=None, out_degrees=None,
                    graph_indices_T=None, graph_values_T=None, backward_divisor=None)
        backward_divisor: None / "adjoint" (G / in_degrees, the exact gradient) or
        "reference" (G / out_degrees, the reference's rule, maxk_spgemm_function.py:154-159)
    v4: maxk_spgemm(graph_indices, graph_values, topk_values, topk_indices, warp4_metadata,
                    num_warps, graph_indptr, degrees, dim_origin=None)"""
    _require_kernels()
    if isinstance(a4, torch.Tensor):
        names = ("warp4_metadata", "num_warps", "graph_indptr", "degrees", "dim_origin")
        defaults = (None, 0, None, None, None)
    else:
        names = ("warp4_metadata", "num_warps", "graph_indptr", "in_degrees", "out_degrees",
                 "graph_indices_T", "graph_values_T", "backward_divisor")
        defaults = (None, 0, None, None, None, None, None, None)
    args = list(rest) + [None] * (len(names) - len(rest))
    for i, n in enumerate(names):
        if n in kw:
            args[i] = kw.pop(n)
        elif i >= len(rest):
            args[i] = defaults[i]
    if kw:
        raise TypeError(f"unexpected keyword arguments: {sorted(kw)}")
    if args[-1] is None:  # dim_origin / backward_divisor left out: the reference's arity
        args = args[:-1]
    return MaxKSpGEMMFunction.apply(graph_indices, graph_values, a3, a4, *args)


class MaxKSpGEMMHeadsFunction(Function):
    """H aggregations over one graph and one CBSR that differ in their edge weights (attention
    heads): apply(graph_indptr, graph_indices, graph_values [H, E], topk_values [V, k],
    topk_indices [V, k], dim_origin, degrees) -> [H, V, dim_origin].

    The forward and the weight gradient are the multi-head kernels (one record gather per edge
    for all heads: maxk_cuda_kernels.spgemm_forward_heads / edge_weight_grad_heads); on a dense
    graph, where the multi-head forward measured no faster, the forward is H single-head calls
    into the slices of the output instead (maxk_cuda_kernels.heads_forward_route).  The
    feature gradient, the sum over the heads, is one sspmm_backward_heads call (the heads summed
    per edge before the contribution row is stored) where
    maxk_cuda_kernels.heads_backward_route says "heads": two or more heads, no forced backward
    mode; on route "calls" it is the sum, in head order, of sspmm_backward on (graph_values[h],
    grad_output[h]) in the graph-only mode the single-head function takes with differentiable
    weights."""

    @staticmethod
    def forward(ctx, graph_indptr, graph_indices, graph_values, topk_values, topk_indices,
                dim_origin, degrees):
        _require_kernels()
        indptr, indices = _i32(graph_indptr), _i32(graph_indices)
        vals = _f32_act(topk_values)
        sel = topk_indices if topk_indices.dtype == torch.uint8 else topk_indices.to(torch.uint8)
        sel = sel.contiguous()
        w = _f32_act(graph_values)  # attention weights change every step: never cached
        row_div = _f32(degrees)
        D = int(dim_origin)
        V, k = vals.shape
        num_rows = indptr.numel() - 1
        if maxk_cuda_kernels.heads_forward_route(num_rows, indices.numel()) == "heads":
            out = maxk_cuda_kernels.spgemm_forward_heads(indptr, indices, w, vals, sel, D,
                                                         row_div=row_div)
        else:  # a dense graph: the multi-head kernel measured no faster there
            if w.dim() != 2 or not 1 <= w.shape[0] <= maxk_cuda_kernels.MAX_HEADS:
                raise RuntimeError("graph_values must be [H, num_e] with 1 <= H <= "
                                   f"{maxk_cuda_kernels.MAX_HEADS}")
            out = torch.empty(w.shape[0], num_rows, D, dtype=torch.float32, device=vals.device)
            for h in range(w.shape[0]):
                maxk_cuda_kernels.spgemm_forward(indptr, indices, w[h], vals, sel, D,
                                                 row_div=row_div, out=out[h])
        ctx.bwd_mode = maxk_cuda_kernels.graph_only_mode(k, indices.numel(), V)
        ctx.has_div = row_div is not None
        ctx.save_for_backward(indptr, indices, w, vals, sel,
                              row_div if row_div is not None else torch.empty(0))
        ctx.w_dtype = graph_values.dtype
        return out

    @staticmethod
    def backward(ctx, grad_output):
        indptr, indices, w, vals, sel, row_div = ctx.saved_tensors
        row_div = row_div if ctx.has_div else None
        g = grad_output.contiguous()
        if g.dtype != torch.float32:
            g = g.float()
        grad_w = grad_tv = None
        if ctx.needs_input_grad[2]:
            grad_w = maxk_cuda_kernels.edge_weight_grad_heads(indptr, indices, vals, sel, g,
                                                              row_div=row_div).to(ctx.w_dtype)
        if ctx.needs_input_grad[3] and maxk_cuda_kernels.heads_backward_route(
                sel.shape[1], indices.numel(), sel.shape[0], indptr.numel() - 1,
                w.shape[0]) == "heads":
            grad_tv = maxk_cuda_kernels.sspmm_backward_heads(indptr, indices, w, g, sel,
                                                             row_div=row_div)
        elif ctx.needs_input_grad[3]:
            for h in range(w.shape[0]):  # accumulated in head order
                part = maxk_cuda_kernels.sspmm_backward(indptr, indices, w[h], g[h], sel,
                                                        row_div=row_div, mode=ctx.bwd_mode)
                grad_tv = part if grad_tv is None else grad_tv.add_(part)
        return None, None, grad_w, grad_tv, None, None, None


def maxk_spgemm_heads(graph_indptr, graph_indices, graph_values, topk_values, topk_indices,
                      dim_origin, degrees=None):
    """[H, V, dim_origin] = (A_h . scatter(topk)) / degrees for the H weight sets
    graph_values [H, E] of one CSR graph; gradients for graph_values and topk_values
    (MaxKSpGEMMHeadsFunction)."""
    _require_kernels()
    return MaxKSpGEMMHeadsFunction.apply(graph_indptr, graph_indices, graph_values, topk_values,
                                         topk_indices, dim_origin, degrees)


class MaxKGATAttentionHeadsFunction(Function):
    """The attention aggregation of H GAT heads with the softmax inside the walk:
    apply(graph_indptr, graph_indices, s_dst [H, V], s_src [H, V], topk_values [V, k],
    topk_indices [V, k], dim_origin, negative_slope) -> [H, V, dim_origin].

    The forward is one maxk_cuda_kernels.gat_attention_heads call.  It saves the graph, the
    scores, the CBSR and the two row statistics [H, V] -- no tensor of H * E elements.  The
    backward rebuilds the coefficients with gat_edge_alpha_heads as a transient, runs the
    stored path's backward on them (edge_weight_grad_heads, gat_edge_softmax_heads_backward,
    the feature gradient on the route heads_backward_route gives) and drops them.

    backward="fused" (a ninth argument; "rebuilt", the above, is the default) saves `out` as
    well and runs one maxk_cuda_kernels.gat_attention_heads_backward call instead: no tensor of
    H * E elements in the backward either.  It falls back to the rebuilt backward when not all
    three gradients are needed, when the table is too large for the entry
    (maxk_cuda_kernels.HEADS_MAX_COLS) and when MAXK_BWD_MODE forces a backward mode.

    dropout, seed (a tenth and eleventh argument, default 0.0 and 0): attention dropout under
    the mask of (seed, head, edge) that maxk_cuda_kernels.edge_dropout_heads documents.  Only
    the two numbers are kept: the forward walk evaluates the mask, the fused backward evaluates
    it again in its one call, and the rebuilt backward masks the rebuilt coefficients once for
    the feature gradient and the weight gradient before the softmax backward."""

    @staticmethod
    def forward(ctx, graph_indptr, graph_indices, s_dst, s_src, topk_values, topk_indices,
                dim_origin, negative_slope, backward="rebuilt", dropout=0.0, seed=0):
        _require_kernels()
        if backward not in ("rebuilt", "fused"):
            raise ValueError(f'backward must be "rebuilt" or "fused", got {backward!r}')
        indptr, indices = _i32(graph_indptr), _i32(graph_indices)
        vals = _f32_act(topk_values)
        sel = topk_indices if topk_indices.dtype == torch.uint8 else topk_indices.to(torch.uint8)
        sel = sel.contiguous()
        sd, ss = _f32_act(s_dst), _f32_act(s_src)
        out, row_max, row_sum = maxk_cuda_kernels.gat_attention_heads(
            indptr, indices, sd, ss, vals, sel, int(dim_origin), float(negative_slope),
            dropout=float(dropout), seed=int(seed))
        ctx.drop = (float(dropout), int(seed))
        V, k = vals.shape
        ctx.bwd_mode = maxk_cuda_kernels.graph_only_mode(k, indices.numel(), V)
        ctx.slope = float(negative_slope)
        ctx.dtypes = (s_dst.dtype, s_src.dtype)
        ctx.fused_bwd = (backward == "fused" and V < maxk_cuda_kernels.HEADS_MAX_COLS
                         and ctx.bwd_mode is not None)
        if ctx.fused_bwd:
            ctx.save_for_backward(indptr, indices, sd, ss, vals, sel, row_max, row_sum, out)
        else:
            ctx.save_for_backward(indptr, indices, sd, ss, vals, sel, row_max, row_sum)
        ctx.mark_non_differentiable(row_max, row_sum)
        return out, row_max, row_sum

    @staticmethod
    def backward(ctx, grad_output, _grad_max, _grad_sum):
        indptr, indices, sd, ss, vals, sel, row_max, row_sum = ctx.saved_tensors[:8]
        g = grad_output.contiguous()
        if g.dtype != torch.float32:
            g = g.float()
        H = sd.shape[0]
        need_s = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        grad_sd = grad_ss = grad_tv = None
        p, seed = ctx.drop
        if ctx.fused_bwd and all(ctx.needs_input_grad[2:5]):
            grad_sd, grad_ss, grad_tv = maxk_cuda_kernels.gat_attention_heads_backward(
                indptr, indices, sd, ss, vals, sel, ctx.saved_tensors[8], row_max, row_sum, g,
                ctx.slope, dropout=p, seed=seed)
            return (None, None, grad_sd.to(ctx.dtypes[0]), grad_ss.to(ctx.dtypes[1]), grad_tv,
                    None, None, None, None, None, None)
        alpha = maxk_cuda_kernels.gat_edge_alpha_heads(indptr, indices, sd, ss, row_max, row_sum,
                                                       ctx.slope)
        if need_s:
            grad_w = maxk_cuda_kernels.edge_weight_grad_heads(indptr, indices, vals, sel, g)
            if p > 0:  # the gradient of the dropped coefficients back through the mask
                maxk_cuda_kernels.edge_dropout_heads(grad_w, p, seed, out=grad_w)
            grad_sd, grad_ss = maxk_cuda_kernels.gat_edge_softmax_heads_backward(
                indptr, indices, sd, ss, alpha, grad_w, ctx.slope)
            del grad_w
            grad_sd, grad_ss = grad_sd.to(ctx.dtypes[0]), grad_ss.to(ctx.dtypes[1])
        if p > 0 and ctx.needs_input_grad[4]:  # the softmax backward above took the undropped
            maxk_cuda_kernels.edge_dropout_heads(alpha, p, seed, out=alpha)
        if ctx.needs_input_grad[4] and maxk_cuda_kernels.heads_backward_route(
                sel.shape[1], indices.numel(), sel.shape[0], indptr.numel() - 1, H) == "heads":
            grad_tv = maxk_cuda_kernels.sspmm_backward_heads(indptr, indices, alpha, g, sel)
        elif ctx.needs_input_grad[4]:
            for h in range(H):  # accumulated in head order
                part = maxk_cuda_kernels.sspmm_backward(indptr, indices, alpha[h], g[h], sel,
                                                        mode=ctx.bwd_mode)
                grad_tv = part if grad_tv is None else grad_tv.add_(part)
        del alpha
        return (None, None, grad_sd if ctx.needs_input_grad[2] else None,
                grad_ss if ctx.needs_input_grad[3] else None, grad_tv, None, None, None, None,
                None, None)


class MaxKEdgeDropoutHeadsFunction(Function):
    """Attention dropout of head-major edge weights: apply(w [H, E], p, seed) -> w * d, d the mask
    of maxk_cuda_kernels.edge_dropout_heads.  It saves (p, seed) and no tensor: the backward is
    the same call on the gradient, which recomputes the mask."""

    @staticmethod
    def forward(ctx, w, p, seed):
        _require_kernels()
        ctx.drop = (float(p), int(seed))
        ctx.w_dtype = w.dtype
        return maxk_cuda_kernels.edge_dropout_heads(_f32_act(w), *ctx.drop)

    @staticmethod
    def backward(ctx, grad_output):
        g = grad_output.contiguous()
        if g.dtype != torch.float32:
            g = g.float()
        return maxk_cuda_kernels.edge_dropout_heads(g, *ctx.drop).to(ctx.w_dtype), None, None


def maxk_edge_dropout_heads(w, p, seed):
    """w [H, E] * d under the attention-dropout mask of (seed, head, edge), rate p
    (MaxKEdgeDropoutHeadsFunction); p == 0 returns w itself."""
    if p == 0:
        return w
    return MaxKEdgeDropoutHeadsFunction.apply(w, p, seed)


def maxk_gat_attention_heads(graph_indptr, graph_indices, s_dst, s_src, topk_values,
                             topk_indices, dim_origin, negative_slope=0.2, backward="rebuilt",
                             dropout=0.0, seed=0):
    """[H, V, dim_origin] = sum over a row's edges of softmax(leaky_relu(s_dst[h, row] +
    s_src[h, col])) * scatter(topk)[col], for the H heads of one CSR graph, without the
    coefficients [H, E] being stored; gradients for s_dst, s_src and topk_values
    (MaxKGATAttentionHeadsFunction).  backward: "rebuilt" (the coefficients as a transient and
    the stored path's passes) or "fused" (one gat_attention_heads_backward call).  dropout,
    seed: attention dropout inside the walk, the mask recomputed by each backward."""
    _require_kernels()
    return MaxKGATAttentionHeadsFunction.apply(graph_indptr, graph_indices, s_dst, s_src,
                                               topk_values, topk_indices, dim_origin,
                                               negative_slope, backward, dropout, seed)[0]


def _dot_inputs(graph_indptr, graph_indices, q, topk_values, topk_indices):
    """The operands of the dot-product attention functions as the kernels take them."""
    sel = topk_indices if topk_indices.dtype == torch.uint8 else topk_indices.to(torch.uint8)
    return (_i32(graph_indptr), _i32(graph_indices), _f32_act(q), _f32_act(topk_values),
            sel.contiguous())


def _f32_grad(g):
    g = g.contiguous()
    return g if g.dtype == torch.float32 else g.float()


class MaxKDotScoresHeadsFunction(Function):
    """The scaled dot-product scores of H heads on CBSR keys, stored:
    apply(graph_indptr, graph_indices, q [H, V, D], topk_values [V, k], topk_indices [V, k],
    scale) -> logits [H, E], logits[h, e] = scale * q[h, row(e)] . scatter(topk)[col(e)].

    A composition of existing kernels, because the score of an edge is the aggregation's
    edge-weight gradient with the query in the place of grad_out: the forward is
    edge_weight_grad_heads(grad_output=q), the gradient of q is spgemm_forward_heads with the
    logits' gradient as the edge weights, and the gradient of topk_values is
    sspmm_backward_heads(values=grad, grad_output=q)."""

    @staticmethod
    def forward(ctx, graph_indptr, graph_indices, q, topk_values, topk_indices, scale):
        _require_kernels()
        indptr, indices, qf, vals, sel = _dot_inputs(graph_indptr, graph_indices, q, topk_values,
                                                     topk_indices)
        ctx.scale = float(scale)
        ctx.q_dtype = q.dtype
        logits = maxk_cuda_kernels.edge_weight_grad_heads(indptr, indices, vals, sel, qf)
        ctx.save_for_backward(indptr, indices, qf, vals, sel)
        return logits.mul_(ctx.scale)

    @staticmethod
    def backward(ctx, grad_output):
        indptr, indices, qf, vals, sel = ctx.saved_tensors
        g = _f32_grad(grad_output)
        grad_q = grad_tv = None
        if ctx.needs_input_grad[2]:
            grad_q = maxk_cuda_kernels.spgemm_forward_heads(indptr, indices, g, vals, sel,
                                                            qf.shape[2]).mul_(ctx.scale)
            grad_q = grad_q.to(ctx.q_dtype)
        if ctx.needs_input_grad[3]:
            grad_tv = maxk_cuda_kernels.sspmm_backward_heads(indptr, indices, g, qf,
                                                             sel).mul_(ctx.scale)
        return None, None, grad_q, grad_tv, None, None


def maxk_dot_scores_heads(graph_indptr, graph_indices, q, topk_values, topk_indices, scale):
    """logits [H, E] = scale * q[h, row] . scatter(topk)[col] for the H heads of one CSR graph;
    gradients for q and topk_values (MaxKDotScoresHeadsFunction)."""
    _require_kernels()
    return MaxKDotScoresHeadsFunction.apply(graph_indptr, graph_indices, q, topk_values,
                                            topk_indices, scale)


class MaxKDotAttentionHeadsFunction(Function):
    """Scaled dot-product attention of H heads on CBSR keys with the score and the softmax inside
    the aggregation walk: apply(graph_indptr, graph_indices, q [H, V, D], topk_values [V, k],
    topk_indices [V, k], dim_origin, scale) -> (out [H, V, dim_origin], row_max, row_sum).

    The forward is one maxk_cuda_kernels.dot_attention_heads call.  It saves the graph, q, the
    CBSR and the two row statistics [H, V] -- no tensor of H * E elements.  The backward rebuilds
    the coefficients with dot_edge_alpha_heads as a transient and runs the stored path's passes
    on them: edge_weight_grad_heads for the coefficients' gradient, edge_softmax_backward per head
    for the logits', spgemm_forward_heads on those for q, and for topk_values the sum of the
    aggregation's feature gradient (sspmm_backward_heads on the coefficients) and the scores'
    (sspmm_backward_heads on the logits' gradient against q).

    backward="fused" (an eighth argument; "rebuilt", the above, is the default) saves `out` as
    well and runs one maxk_cuda_kernels.dot_attention_heads_backward call instead: no tensor of
    H * E elements in the backward either.  It falls back to the rebuilt backward when not both
    gradients are needed, when the table is too large for the entry
    (maxk_cuda_kernels.HEADS_MAX_COLS) and when MAXK_BWD_MODE forces a backward mode.

    dropout, seed (a ninth and tenth argument, default 0.0 and 0): attention dropout under the
    mask of (seed, head, edge) that maxk_cuda_kernels.edge_dropout_heads documents.  Only the two
    numbers are kept: the forward walk evaluates the mask, the fused backward evaluates it again
    in its one call, and the rebuilt backward masks the coefficients' gradient before the softmax
    backward and the rebuilt coefficients after it, for the feature gradient."""

    @staticmethod
    def forward(ctx, graph_indptr, graph_indices, q, topk_values, topk_indices, dim_origin, scale,
                backward="rebuilt", dropout=0.0, seed=0):
        _require_kernels()
        if backward not in ("rebuilt", "fused"):
            raise ValueError(f'backward must be "rebuilt" or "fused", got {backward!r}')
        indptr, indices, qf, vals, sel = _dot_inputs(graph_indptr, graph_indices, q, topk_values,
                                                     topk_indices)
        ctx.scale = float(scale)
        ctx.q_dtype = q.dtype
        ctx.drop = (float(dropout), int(seed))
        out, row_max, row_sum = maxk_cuda_kernels.dot_attention_heads(
            indptr, indices, qf, vals, sel, int(dim_origin), ctx.scale, dropout=ctx.drop[0],
            seed=ctx.drop[1])
        V, k = vals.shape
        ctx.fused_bwd = (backward == "fused" and V < maxk_cuda_kernels.HEADS_MAX_COLS
                         and maxk_cuda_kernels.graph_only_mode(k, indices.numel(), V) is not None)
        if ctx.fused_bwd:
            ctx.save_for_backward(indptr, indices, qf, vals, sel, row_max, row_sum, out)
        else:
            ctx.save_for_backward(indptr, indices, qf, vals, sel, row_max, row_sum)
        ctx.mark_non_differentiable(row_max, row_sum)
        return out, row_max, row_sum

    @staticmethod
    def backward(ctx, grad_output, _grad_max, _grad_sum):
        indptr, indices, qf, vals, sel, row_max, row_sum = ctx.saved_tensors[:7]
        mk = maxk_cuda_kernels
        g = _f32_grad(grad_output)
        H, _, D = qf.shape
        p, seed = ctx.drop
        if ctx.fused_bwd and all(ctx.needs_input_grad[2:4]):
            grad_q, grad_tv = mk.dot_attention_heads_backward(
                indptr, indices, qf, vals, sel, ctx.saved_tensors[7], row_max, row_sum, g,
                ctx.scale, dropout=p, seed=seed)
            return (None, None, grad_q.to(ctx.q_dtype), grad_tv, None, None, None, None, None,
                    None)
        alpha = mk.dot_edge_alpha_heads(indptr, indices, qf, vals, sel, D, ctx.scale, row_max,
                                        row_sum)
        grad_a = mk.edge_weight_grad_heads(indptr, indices, vals, sel, g)
        if p > 0:  # the gradient of the dropped coefficients back through the mask
            mk.edge_dropout_heads(grad_a, p, seed, out=grad_a)
        grad_l = torch.empty_like(grad_a)
        for h in range(H):
            mk.edge_softmax_backward(indptr, alpha[h], grad_a[h], out=grad_l[h])
        del grad_a
        grad_q = grad_tv = None
        if ctx.needs_input_grad[2]:
            grad_q = mk.spgemm_forward_heads(indptr, indices, grad_l, vals, sel, D)
            grad_q = grad_q.mul_(ctx.scale).to(ctx.q_dtype)
        if ctx.needs_input_grad[3]:
            if p > 0:  # the softmax backward above took the undropped coefficients
                mk.edge_dropout_heads(alpha, p, seed, out=alpha)
            grad_tv = mk.sspmm_backward_heads(indptr, indices, alpha, g, sel)
            grad_tv.add_(mk.sspmm_backward_heads(indptr, indices, grad_l, qf, sel),
                         alpha=ctx.scale)
        del alpha, grad_l
        return None, None, grad_q, grad_tv, None, None, None, None, None, None


def maxk_dot_attention_heads(graph_indptr, graph_indices, q, topk_values, topk_indices,
                             dim_origin, scale, backward="rebuilt", dropout=0.0, seed=0):
    """[H, V, dim_origin] = sum over a row's edges of softmax(scale * q[h, row] .
    scatter(topk)[col]) * scatter(topk)[col], for the H heads of one CSR graph, without logits or
    coefficients [H, E] being stored; gradients for q and topk_values
    (MaxKDotAttentionHeadsFunction).  backward: "rebuilt" (the coefficients as a transient and
    the stored path's passes) or "fused" (one dot_attention_heads_backward call).  dropout,
    seed: attention dropout inside the walk, the mask recomputed by each backward."""
    _require_kernels()
    return MaxKDotAttentionHeadsFunction.apply(graph_indptr, graph_indices, q, topk_values,
                                               topk_indices, dim_origin, scale, backward, dropout,
                                               seed)[0]


class MaxKSpGEMMMaxFunction(Function):
    """The element-wise maximum over each row's neighbours of scatter(topk_values, topk_indices):
    apply(graph_indptr, graph_indices, topk_values [V, k], topk_indices [V, k], dim_origin)
    -> out [V, dim_origin] (maxk_cuda_kernels.spgemm_max_forward has the rules: the first
    largest candidate in edge order wins, a neighbour that does not keep a column competes with
    an implicit zero, a NaN beats everything).

    The forward saves the winners' edge indices arg [V, dim_origin] int32 and topk_indices, and
    nothing else of the activations (the graph's own tensors ride on the context); when
    topk_values needs no gradient -- it does not require one, or (a sixth argument, which
    maxk_spgemm_max passes: grad mode is always off inside a forward) grad mode is off -- the
    kernel stores no winners at all.  The backward is one maxk_cuda_kernels.spgemm_max_backward call: the gradient reaches
    topk_values only, each winner's slots receiving grad_output at their column."""

    @staticmethod
    def forward(ctx, graph_indptr, graph_indices, topk_values, topk_indices, dim_origin,
                grad_mode=True):
        _require_kernels()
        indptr, indices = _i32(graph_indptr), _i32(graph_indices)
        sel = topk_indices if topk_indices.dtype == torch.uint8 else topk_indices.to(torch.uint8)
        sel = sel.contiguous()
        want = bool(grad_mode and ctx.needs_input_grad[2])
        out, arg = maxk_cuda_kernels.spgemm_max_forward(indptr, indices, _f32_act(topk_values),
                                                        sel, int(dim_origin), want_arg=want)
        if want:
            ctx.graph = (indptr, indices)
            ctx.val_dtype = topk_values.dtype
            ctx.save_for_backward(arg, sel)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        arg, sel = ctx.saved_tensors
        indptr, indices = ctx.graph
        grad = maxk_cuda_kernels.spgemm_max_backward(indptr, indices, sel, arg,
                                                     _f32_grad(grad_output), sel.shape[1])
        return None, None, grad.to(ctx.val_dtype), None, None, None


def maxk_spgemm_max(graph_indptr, graph_indices, topk_values, topk_indices, dim_origin):
    """[V, dim_origin] = max over a row's neighbours of scatter(topk)[col], 0 for a row without
    edges; the gradient reaches topk_values (MaxKSpGEMMMaxFunction)."""
    _require_kernels()
    return MaxKSpGEMMMaxFunction.apply(graph_indptr, graph_indices, topk_values, topk_indices,
                                       dim_origin, torch.is_grad_enabled())


class MaxKSpmmWrapper:
    """Holds the warp4 metadata of one graph (maxk_spgemm_function.py:214-267)."""

    def __init__(self, graph_name: str = "", num_warps: int = 12, warp_max_nz: int = 64):
        self.graph_name = graph_name
        self.warp4_metadata = None
        self.num_warps = 0
        self.num_warps_config = num_warps
        self.warp_max_nz = warp_max_nz
        self._indptr_cache = None

    def load_metadata(self, graph_name: Optional[str] = None) -> bool:
        """Read kernels/w12_nz64_warp_4/<graph>.warp4 (CWD-relative); False on failure."""
        if graph_name is None:
            graph_name = self.graph_name
        if not MAXK_KERNELS_AVAILABLE:
            print("MaxK kernels not available")
            return False
        try:
            self.warp4_metadata = maxk_cuda_kernels.load_warp4_metadata(
                graph_name, self.num_warps_config, self.warp_max_nz)
        except Exception as e:  # noqa: BLE001 -- reference contract: report and return False
            print(f"Failed to load MaxK metadata: {e}")
            return False
        self.num_warps = self.warp4_metadata.size(0) // 4
        self._indptr_cache = None
        return True

    def build_metadata(self, graph_indptr: torch.Tensor) -> bool:
        """Build the warp4 schedule on the GPU from the CSR row pointer (no .warp4 file needed)."""
        _require_kernels()
        ip = graph_indptr if graph_indptr.dtype == torch.int32 else graph_indptr.int()
        self.warp4_metadata = maxk_cuda_kernels.build_warp4_metadata(ip.contiguous(),
                                                                     self.warp_max_nz)
        self.num_warps = self.warp4_metadata.size(0) // 4
        self._indptr_cache = ip.contiguous()
        return True

    def _indptr(self, graph_indptr, num_v):
        if graph_indptr is not None:
            return graph_indptr
        if self._indptr_cache is None or self._indptr_cache.numel() != num_v + 1:
            self._indptr_cache = _indptr_for(None, self.warp4_metadata, self.num_warps, num_v)
        return self._indptr_cache

    def spmm(self, graph_indices, graph_values, a3, a4, *rest, **kw):
        """v1: spmm(graph_indices, graph_values, input_features, k_value, graph_indptr=None,
                    in_degrees=None, out_degrees=None, graph_indices_T=None, graph_values_T=None)
        v4: spmm(graph_indices, graph_values, topk_values, topk_indices, graph_indptr, degrees)"""
        if isinstance(a4, torch.Tensor):
            names = ("graph_indptr", "degrees", "dim_origin")
        else:
            names = ("graph_indptr", "in_degrees", "out_degrees", "graph_indices_T",
                     "graph_values_T", "backward_divisor")
        vals = dict(zip(names, rest))
        vals.update(kw)
        ip = self._indptr(vals.get("graph_indptr"), a3.shape[0])
        if isinstance(a4, torch.Tensor):
            return maxk_spgemm(graph_indices, graph_values, a3, a4, self.warp4_metadata,
                               self.num_warps, ip, vals.get("degrees"),
                               dim_origin=vals.get("dim_origin"))
        return maxk_spgemm(graph_indices, graph_values, a3, a4, self.warp4_metadata,
                           self.num_warps, ip, vals.get("in_degrees"), vals.get("out_degrees"),
                           vals.get("graph_indices_T"), vals.get("graph_values_T"),
                           backward_divisor=vals.get("backward_divisor"))
