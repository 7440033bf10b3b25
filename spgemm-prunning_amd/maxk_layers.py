"""MaxK-GNN layers on the drop-in aggregation, without DGL.

The reference's integrated models (model_integrated_v3.py: OPTMaxK :28-43,
MaxKSAGEConv :62-192, MaxKGraphConv :194-398, MaxKGINConv :400-520, MaxKSAGE
:522-588) wrap DGL graphs; here a layer takes a `CSRGraph` (row r = destination,
its columns = source vertices) and every aggregation goes through
`maxk_spgemm_function.maxk_spgemm` (v4 shape) -> the HIP kernels.  The MaxK
nonlinearity runs on the HIP top-k.

Caller defects of the reference fixed here, each documented
where it applies:
  * OPTMaxK.backward drops the gradient of topk_values (:39-43) -> MaxK below
    returns grad = scatter(gather(g_dense) + g_topk);
  * GCN "both"/"left" normalisation scales feat_src, but the kernel is then fed
    the unnormalised topk_values AND divides by degree (:301-310, 341-345,
    380-389) -> here the symmetric normalisation is folded into the edge values
    once per graph and the kernel divides by nothing;
  * lin_before_mp paths apply the Linear to the [V, k] top-k values (:166, 330)
    -> here aggregation always runs on the CBSR and the Linear after it (equal by
    linearity, and the aggregation keeps its k-sparse input);
  * GIN "sum" passes the degrees, i.e. computes a mean (:493) -> here a sum;
  * the models' feat_drop masks x_sparse but the aggregation is fed the undropped
    topk_values (:153-181, :661-664, :743-746) -> here the aggregated values are the
    dropped ones.

`reference_compat=True` (on `maxk`, the convolutions and the models) reproduces every one of
these behaviours instead, so a model trained with the reference computes the same function
here (tests/test_layers_gpu.py checks each against a dense restatement of the reference's
lines).  The reference's lin_before_mp branches (in_feats > out_feats) multiply the [V, k]
top-k values by an [in_feats, out] matrix, which raises and sends the reference to its DGL
fallback, i.e. the normalised aggregation; compat mode computes that fallback there.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn as nn
from torch.autograd import Function

import maxk_cuda_kernels as mk
from maxk_spgemm_function import (maxk_dot_attention_heads, maxk_dot_scores_heads,
                                  maxk_edge_dropout_heads, maxk_gat_attention_heads, maxk_spgemm,
                                  maxk_spgemm_heads, maxk_spgemm_max)


def _clamped(graph, name: str) -> torch.Tensor:
    """graph.<name> clamped to >= 1: CSRGraph's cached tensor, or computed for a graph-like
    object without the cache."""
    f = getattr(graph, "clamped", None)
    return f(name) if f is not None else getattr(graph, name).clamp(min=1.0)


class CSRGraph:
    """Adjacency in CSR with rows = destinations: out[r] aggregates x[indices[e]], e in row r."""

    def __init__(self, indptr: torch.Tensor, indices: torch.Tensor,
                 values: Optional[torch.Tensor] = None):
        self.indptr = indptr.int().contiguous()
        self.indices = indices.int().contiguous()
        self.num_nodes = self.indptr.numel() - 1
        self.values = (torch.ones(self.indices.numel(), device=self.indices.device)
                       if values is None else values.float().contiguous())
        # in-degree of a destination row, out-degree of a source (column counts)
        self.in_degrees = torch.diff(self.indptr).float()
        self.out_degrees = torch.bincount(self.indices.long(),
                                          minlength=self.num_nodes).float()
        self._rows = None
        self._clamped = {}

    def clamped(self, name: str) -> torch.Tensor:
        """in_degrees / out_degrees clamped to >= 1, built once: the same divisor tensor
        every call, so per-(plan, divisor) work in the backward (maxk_cuda_kernels'
        pre-scaled pull entries) is done once per graph."""
        if name not in self._clamped:
            self._clamped[name] = getattr(self, name).clamp(min=1.0)
        return self._clamped[name]

    def edge_rows(self) -> torch.Tensor:
        if self._rows is None:
            self._rows = torch.repeat_interleave(
                torch.arange(self.num_nodes, device=self.indptr.device),
                torch.diff(self.indptr).long())
        return self._rows

    def aggregate(self, topk_values, topk_indices, dim: int, values=None, row_div=None):
        """(A . scatter(CBSR))[r] / row_div[r] through the drop-in v4 surface."""
        return maxk_spgemm(self.indices, self.values if values is None else values,
                           topk_values, topk_indices, None, 0, self.indptr, row_div,
                           dim_origin=dim)

    def aggregate_max(self, topk_values, topk_indices, dim: int):
        """[V, dim]: the element-wise maximum over each row's neighbours of scatter(CBSR)
        (maxk_spgemm_max): a neighbour that does not keep a column competes with 0 there, a row
        without edges is 0.  Unweighted: the graph's edge values are not used."""
        return maxk_spgemm_max(self.indptr, self.indices, topk_values, topk_indices, dim)

    def aggregate_heads(self, topk_values, topk_indices, dim: int, values, row_div=None):
        """[H, V, dim]: aggregate() for the H weight sets values [H, E] (attention heads), one
        record gather per edge serving all heads (maxk_spgemm_heads)."""
        return maxk_spgemm_heads(self.indptr, self.indices, values, topk_values, topk_indices,
                                 dim, row_div)

    def attend_heads(self, topk_values, topk_indices, dim: int, s_dst, s_src,
                     negative_slope: float = 0.2, backward: str = "rebuilt",
                     dropout: float = 0.0, seed: int = 0):
        """[H, V, dim]: the attention aggregation of H GAT heads from their scores s_dst [H, V]
        and s_src [H, V] with the softmax inside the walk (maxk_gat_attention_heads): what
        gat_edge_softmax_heads followed by aggregate_heads give, without alpha [H, E] stored.
        backward: "rebuilt" (alpha as a transient of the backward) or "fused" (one walk, no
        [H, E] tensor in the backward either); MAXK_HEADS_ATTN_BWD=fused|rebuilt overrides it.
        dropout, seed: attention dropout inside the walk under the mask of (seed, head, edge)
        (mk.edge_dropout_heads has the contract); only the two numbers are kept for the
        backward, which recomputes the mask."""
        if backward not in ("rebuilt", "fused"):
            raise ValueError(f'backward must be "rebuilt" or "fused", got {backward!r}')
        forced = os.environ.get("MAXK_HEADS_ATTN_BWD", "")
        if forced in ("fused", "rebuilt"):
            backward = forced
        return maxk_gat_attention_heads(self.indptr, self.indices, s_dst, s_src, topk_values,
                                        topk_indices, dim, negative_slope, backward, dropout,
                                        seed)

    def dot_attend_heads(self, topk_values, topk_indices, dim: int, q, scale: float,
                         backward: str = "rebuilt", dropout: float = 0.0, seed: int = 0):
        """[H, V, dim]: scaled dot-product attention of H heads on the CBSR keys, from the
        queries q [H, V, dim] mapped into the feature space, with the score and the softmax
        inside the aggregation walk (maxk_dot_attention_heads): what maxk_dot_scores_heads, the
        edge softmax per head and aggregate_heads give, without logits or alpha [H, E] stored.
        backward: "rebuilt" (alpha as a transient of the backward) or "fused" (one
        dot_attention_heads_backward call, no [H, E] tensor in the backward either);
        MAXK_DOT_ATTN_BWD=fused|rebuilt overrides it.
        dropout, seed: attention dropout inside the walk under the mask of (seed, head, edge)
        (mk.edge_dropout_heads has the contract); only the two numbers are kept for the
        backward, which recomputes the mask."""
        if backward not in ("rebuilt", "fused"):
            raise ValueError(f'backward must be "rebuilt" or "fused", got {backward!r}')
        forced = os.environ.get("MAXK_DOT_ATTN_BWD", "")
        if forced in ("fused", "rebuilt"):
            backward = forced
        return maxk_dot_attention_heads(self.indptr, self.indices, q, topk_values, topk_indices,
                                        dim, scale, backward, dropout, seed)


class MaxK(Function):
    """MaxK nonlinearity (model_integrated_v3.py:28-60): keeps the k largest entries of each
    row.  Returns (dense masked output, topk_values, topk_indices u8); gradients from the
    dense output and from topk_values both reach the input (the reference drops the latter).

    Both directions are single fused HIP passes: the forward writes the
    CBSR and the masked dense row from one top-k kernel (maxk_topk_cbsr_dense); the backward
    gathers the dense gradient at the selected columns, adds the topk_values gradient and
    writes the whole dense row in one kernel (maxk_topk_backward)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, k: int, drop_topk_grad: bool = False):
        dense, vals, idx = mk.topk_cbsr_dense(x.float(), int(k))
        ctx.save_for_backward(idx)
        ctx.D = x.shape[1]
        ctx.drop = bool(drop_topk_grad)
        ctx.mark_non_differentiable(idx)
        return dense, vals, idx

    @staticmethod
    def backward(ctx, g_dense, g_vals, g_idx):
        idx, = ctx.saved_tensors
        # drop_topk_grad: OPTMaxK.backward (model_integrated_v3.py:39-43) returns
        # grad_output * mask and ignores the topk_values gradient
        gv = None if g_vals is None or ctx.drop else g_vals.float().contiguous()
        gd = None if g_dense is None else g_dense.float().contiguous()
        if gv is None and gd is None:
            return None, None, None
        return mk.topk_backward(gv, gd, idx, ctx.D), None, None


def maxk(x: torch.Tensor, k: int, reference_compat: bool = False):
    """(masked dense x, topk_values, topk_indices u8).  reference_compat: the topk_values
    gradient is dropped, as the reference's OPTMaxK does."""
    return MaxK.apply(x, k, reference_compat)


def _dropped_values(x_sparse: torch.Tensor, topk_values: torch.Tensor,
                    topk_indices: torch.Tensor, drop: nn.Module) -> tuple:
    """(dropout(x_sparse), its values at the selected columns): the CBSR of the dropped
    features, so the aggregation sees what the layer's dense input sees.  Without an
    active dropout both are returned unchanged."""
    if not drop.training or getattr(drop, "p", 0.0) == 0.0:
        return x_sparse, topk_values
    xd = drop(x_sparse)
    return xd, xd.gather(1, topk_indices.long())


# ---- dense parts of a full-graph layer (N = all vertices) ---------------------------------
# rocBLAS / hipBLASLt pick a weight-gradient kernel for G^T X with K = N = 2.45M rows that
# runs at ~60 TFLOP/s (5.1 ms for 256x256 on ogbn-products); as a batched GEMM over 256
# row chunks plus a sum it takes 2.2 ms.  PyTorch's bias gradient g.sum(0) over [2.45M, 47]
# takes 19 ms; as a chunked sum 0.11 ms (tools/dense_probe.py).  Same sums, regrouped.

_CHUNKS = 256


def _wgrad(g: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """g^T @ x ([O, I]) for tall g [N, O], x [N, I]."""
    n = g.shape[0]
    if n < _CHUNKS * 1024:
        return g.t() @ x
    m = n // _CHUNKS * _CHUNKS
    out = torch.bmm(g[:m].view(_CHUNKS, m // _CHUNKS, g.shape[1]).transpose(1, 2),
                    x[:m].view(_CHUNKS, m // _CHUNKS, x.shape[1])).sum(0)
    if m < n:
        out.addmm_(g[m:].t(), x[m:])
    return out


def _bgrad(g: torch.Tensor) -> torch.Tensor:
    """g.sum(0) for tall g [N, O]."""
    n = g.shape[0]
    if n < _CHUNKS * 1024:
        return g.sum(0)
    m = n // _CHUNKS * _CHUNKS
    out = g[:m].view(_CHUNKS, m // _CHUNKS, g.shape[1]).sum(1).sum(0)
    return out + g[m:].sum(0) if m < n else out


class _Linear(Function):
    """out = x1 W1^T (+ x2 W2^T) (+ b): nn.Linear (or two summed, SAGE's fc_self + fc_neigh,
    accumulated by a second addmm in place) with the tall-matrix weight/bias gradients above."""

    @staticmethod
    def forward(ctx, x1, w1, b, x2, w2):
        out = torch.addmm(b, x1, w1.t()) if b is not None else x1 @ w1.t()
        if x2 is not None:
            out.addmm_(x2, w2.t())
        ctx.save_for_backward(x1, w1, x2, w2)
        ctx.has_b = b is not None
        return out

    @staticmethod
    def backward(ctx, g):
        x1, w1, x2, w2 = ctx.saved_tensors
        g = g.contiguous()
        n = ctx.needs_input_grad
        gx1 = g @ w1 if n[0] else None
        gw1 = _wgrad(g, x1) if n[1] else None
        gb = _bgrad(g) if ctx.has_b and n[2] else None
        gx2 = g @ w2 if x2 is not None and n[3] else None
        gw2 = _wgrad(g, x2) if x2 is not None and n[4] else None
        return gx1, gw1, gb, gx2, gw2


def linear(x: torch.Tensor, layer: nn.Linear, x2: Optional[torch.Tensor] = None,
           layer2: Optional[nn.Linear] = None) -> torch.Tensor:
    """layer(x) (+ layer2(x2)) through _Linear; layer2's bias (if any) is added separately."""
    out = _Linear.apply(x, layer.weight, layer.bias, x2,
                        None if layer2 is None else layer2.weight)
    if layer2 is not None and layer2.bias is not None:
        out = out + layer2.bias
    return out


def cross_entropy(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """F.cross_entropy(logits, target) (mean over rows) as log_softmax + gather + mean:
    PyTorch's nll_loss reduction kernel takes 5 ms forward + 4 ms backward on 2.45M rows,
    this form 1.3 ms for both (tools/dense_probe.py)."""
    return -torch.log_softmax(logits, 1).gather(1, target[:, None]).mean()


class MaxKSAGEConv(nn.Module):
    """GraphSAGE on MaxK features (model_integrated_v3.py:62-192).
    aggregator_type="mean": rst = fc_self(x_sparse) + fc_neigh(mean_{u in N(v)} x_sparse[u]).
    aggregator_type="pool" (DGL's SAGEConv pool aggregator, which the reference's layer surface
    names and hands to DGL): rst = fc_self(x_sparse) + fc_neigh(max_{u in N(v)} p[u]) with
    p = MaxK_pool_k(fc_pool(x_sparse)).  MaxK stands where DGL's ReLU stands: the pooled
    features are made k-sparse by the layer's own nonlinearity, which is what lets the maximum
    run on the CBSR (CSRGraph.aggregate_max; a neighbour that does not keep a column competes
    with 0 there, as its masked dense feature would).  pool_k: the k of that MaxK (default: the
    k of the topk_values passed in).  fc_pool is Xavier-initialised with the ReLU gain, as DGL
    does.  "mean" keeps its parameters, their initialisation and its state_dict keys."""

    def __init__(self, in_feats: int, out_feats: int, bias: bool = True, feat_drop: float = 0.,
                 activation=None, norm: Optional[nn.Module] = None,
                 reference_compat: bool = False, aggregator_type: str = "mean",
                 pool_k: Optional[int] = None):
        super().__init__()
        valid_aggre_types = {"mean", "pool"}
        if aggregator_type not in valid_aggre_types:
            raise ValueError(f"Invalid aggregator_type. Must be one of {valid_aggre_types}. "
                             f"But got {aggregator_type!r} instead.")
        self.aggregator_type, self.pool_k = aggregator_type, pool_k
        self.in_feats, self.out_feats = in_feats, out_feats
        self.reference_compat = reference_compat
        self.fc_neigh = nn.Linear(in_feats, out_feats, bias=False)
        self.fc_self = nn.Linear(in_feats, out_feats, bias=bias)
        self.feat_drop = nn.Dropout(feat_drop)
        self.activation, self.norm = activation, norm
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_uniform_(self.fc_self.weight, gain=gain)
        nn.init.xavier_uniform_(self.fc_neigh.weight, gain=gain)
        if aggregator_type == "pool":  # after the others: "mean" draws the same numbers as ever
            self.fc_pool = nn.Linear(in_feats, in_feats)
            nn.init.xavier_uniform_(self.fc_pool.weight, gain=gain)

    def forward(self, graph: CSRGraph, x_sparse, topk_values, topk_indices):
        deg = _clamped(graph, "in_degrees")
        if self.reference_compat:  # :153-181: only h_self sees the dropout
            h_self = self.feat_drop(x_sparse)
        else:
            h_self, topk_values = _dropped_values(x_sparse, topk_values, topk_indices,
                                                  self.feat_drop)
        if self.aggregator_type == "pool":
            _, pv, pi = maxk(self.fc_pool(h_self), self.pool_k or topk_values.shape[1])
            agg = graph.aggregate_max(pv, pi, self.in_feats)
        else:
            agg = graph.aggregate(topk_values, topk_indices, self.in_feats, row_div=deg)
        # fc_self(x) + fc_neigh(agg) as one accumulated pair of GEMMs
        rst = linear(h_self, self.fc_self, agg, self.fc_neigh)
        if self.activation is not None:
            rst = self.activation(rst)
        if self.norm is not None:
            rst = self.norm(rst)
        return rst


class MaxKGraphConv(nn.Module):
    """GCN on MaxK features (model_integrated_v3.py:194-398): rst = (N A N') x_sparse W + b,
    norm "both" = D_in^-1/2 A D_out^-1/2, "right" = D_in^-1 A, "left" = A D_out^-1."""

    def __init__(self, in_feats: int, out_feats: int, norm: str = "both", weight: bool = True,
                 bias: bool = True, activation=None, reference_compat: bool = False):
        super().__init__()
        if norm not in ("none", "both", "right", "left"):
            raise ValueError(f'Invalid norm value. Must be either "none", "both", "right" or '
                             f'"left". But got "{norm}".')
        self.in_feats, self.out_feats, self._norm = in_feats, out_feats, norm
        self.reference_compat = reference_compat
        self.weight = nn.Parameter(torch.empty(in_feats, out_feats)) if weight else None
        self.bias = nn.Parameter(torch.zeros(out_feats)) if bias else None
        self.activation = activation
        if self.weight is not None:
            nn.init.xavier_uniform_(self.weight)
        self._graph_key = None
        self._edge_values = None

    def _norm_values(self, graph: CSRGraph) -> torch.Tensor:
        if self._graph_key is not graph:  # once per graph, like the reference's set_graph_data
            v = graph.values
            if self._norm in ("left", "both"):
                src = _clamped(graph, "out_degrees")
                src = src.pow(-0.5) if self._norm == "both" else 1.0 / src
                v = v * src[graph.indices.long()]
            if self._norm in ("right", "both"):
                dst = _clamped(graph, "in_degrees")
                dst = dst.pow(-0.5) if self._norm == "both" else 1.0 / dst
                v = v * dst[graph.edge_rows()]
            self._edge_values, self._graph_key = v.contiguous(), graph
        return self._edge_values

    def forward(self, graph: CSRGraph, x_sparse, topk_values, topk_indices):
        if self.reference_compat and self.in_feats <= self.out_feats:
            # :302-310 normalise feat_src, which the kernel never reads; :341-345 feed it the
            # raw topk_values with the in-degrees as divisor; :381-389 then apply the right
            # normalisation on top
            deg = _clamped(graph, "in_degrees")
            rst = graph.aggregate(topk_values, topk_indices, self.in_feats, row_div=deg)
            if self.weight is not None:
                rst = rst @ self.weight
            if self._norm in ("right", "both"):
                rst = rst * (deg.pow(-0.5) if self._norm == "both" else 1.0 / deg)[:, None]
        else:
            rst = graph.aggregate(topk_values, topk_indices, self.in_feats,
                                  values=self._norm_values(graph))
            if self.weight is not None:
                rst = rst @ self.weight
        if self.bias is not None:
            rst = rst + self.bias
        if self.activation is not None:
            rst = self.activation(rst)
        return rst


class MaxKGINConv(nn.Module):
    """GIN on MaxK features (model_integrated_v3.py:400-520):
    rst = apply_func((1 + eps) x + sum_{u in N(v)} x_sparse[u]); aggregator_type="max" (DGL's
    GINConv max aggregator) takes the element-wise maximum of the neighbours' x_sparse instead
    of their sum (CSRGraph.aggregate_max on the layer's own CBSR inputs).  "max" has no
    reference behaviour to reproduce and is not combined with reference_compat."""

    def __init__(self, apply_func: Optional[nn.Module] = None, init_eps: float = 0.,
                 learn_eps: bool = False, activation=None, reference_compat: bool = False,
                 aggregator_type: str = "sum"):
        super().__init__()
        if aggregator_type not in ("sum", "max"):
            raise KeyError(f"Aggregator type {aggregator_type} not recognized.")
        if aggregator_type == "max" and reference_compat:
            raise ValueError('aggregator_type="max" is not combined with reference_compat')
        self.aggregator_type = aggregator_type
        self.apply_func, self.activation = apply_func, activation
        self.reference_compat = reference_compat
        if learn_eps:
            self.eps = nn.Parameter(torch.tensor([float(init_eps)]))
        else:
            self.register_buffer("eps", torch.tensor([float(init_eps)]))

    def forward(self, graph: CSRGraph, x, topk_values, topk_indices):
        # reference_compat: the "sum" kernel call passes the in-degrees (:491-495), a mean
        row_div = _clamped(graph, "in_degrees") if self.reference_compat else None
        if self.aggregator_type == "max":
            neigh = graph.aggregate_max(topk_values, topk_indices, x.shape[1])
        else:
            neigh = graph.aggregate(topk_values, topk_indices, x.shape[1], row_div=row_div)
        rst = (1 + self.eps) * x + neigh
        if self.apply_func is not None:
            rst = self.apply_func(rst)
        if self.activation is not None:
            rst = self.activation(rst)
        return rst


class EdgeSoftmax(Function):
    """w = softmax of per-edge logits over every destination's incoming edges (the CSR row),
    both directions in HIP (maxk_edge_softmax / _backward): no E-sized intermediates, no
    atomics, bitwise repeatable."""

    @staticmethod
    def forward(ctx, indptr, logits):
        w = mk.edge_softmax(indptr, logits.float().contiguous())
        ctx.save_for_backward(indptr, w)
        ctx.dtype = logits.dtype
        return w.to(logits.dtype)

    @staticmethod
    def backward(ctx, grad_w):
        indptr, w = ctx.saved_tensors
        g = mk.edge_softmax_backward(indptr, w, grad_w.float().contiguous())
        return None, g.to(ctx.dtype)


class GATEdgeSoftmax(Function):
    """alpha = softmax over the row of leaky_relu(s_dst[row] + s_src[col]): a GAT head's
    attention coefficients from its two score vectors (maxk_gat_edge_softmax / _backward).
    Saves alpha and the scores; the backward recomputes the sign of the pre-activation."""

    @staticmethod
    def forward(ctx, indptr, indices, s_dst, s_src, negative_slope):
        sd, ss = s_dst.float().contiguous(), s_src.float().contiguous()
        w = mk.gat_edge_softmax(indptr, indices, sd, ss, negative_slope)
        ctx.save_for_backward(indptr, indices, sd, ss, w)
        ctx.slope = float(negative_slope)
        ctx.dtypes = (s_dst.dtype, s_src.dtype)
        return w

    @staticmethod
    def backward(ctx, grad_w):
        indptr, indices, sd, ss, w = ctx.saved_tensors
        g_dst, g_src = mk.gat_edge_softmax_backward(indptr, indices, sd, ss, w,
                                                    grad_w.float().contiguous(), ctx.slope)
        return None, None, g_dst.to(ctx.dtypes[0]), g_src.to(ctx.dtypes[1]), None


class GATEdgeSoftmaxHeads(Function):
    """alpha [H, E] of H GAT heads from s_dst [H, V] and s_src [H, V] in one pass each way
    (maxk_gat_edge_softmax_heads / _backward): the column index and a column's H scores are read
    once per edge.  Saves alpha and the scores, as GATEdgeSoftmax does."""

    @staticmethod
    def forward(ctx, indptr, indices, s_dst, s_src, negative_slope):
        sd, ss = s_dst.float().contiguous(), s_src.float().contiguous()
        w = mk.gat_edge_softmax_heads(indptr, indices, sd, ss, negative_slope)
        ctx.save_for_backward(indptr, indices, sd, ss, w)
        ctx.slope = float(negative_slope)
        ctx.dtypes = (s_dst.dtype, s_src.dtype)
        return w

    @staticmethod
    def backward(ctx, grad_w):
        indptr, indices, sd, ss, w = ctx.saved_tensors
        g_dst, g_src = mk.gat_edge_softmax_heads_backward(indptr, indices, sd, ss, w,
                                                          grad_w.float().contiguous(), ctx.slope)
        return None, None, g_dst.to(ctx.dtypes[0]), g_src.to(ctx.dtypes[1]), None


def edge_softmax(graph: CSRGraph, logits: torch.Tensor) -> torch.Tensor:
    """Softmax of logits [E] (CSR order) over each destination's incoming edges."""
    return EdgeSoftmax.apply(graph.indptr, logits)


def gat_edge_softmax(graph: CSRGraph, s_dst: torch.Tensor, s_src: torch.Tensor,
                     negative_slope: float = 0.2) -> torch.Tensor:
    """alpha [E] float32 of a single GAT head: s_dst [V] scores the destinations, s_src [V] the
    sources."""
    return GATEdgeSoftmax.apply(graph.indptr, graph.indices, s_dst, s_src, negative_slope)


def _check_attn_drop(p) -> float:
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"attn_drop must be in [0, 1), got {p}")
    return p


def attn_seed_of(attn_seed: Optional[int]) -> int:
    """The seed of one forward's attention-dropout mask: attn_seed as given, or a fresh 63-bit
    draw from torch's default CPU generator (reproducible under torch.manual_seed, and no device
    synchronisation).  The seed reaches the kernels by value: a forward captured into a graph
    replays the mask it was captured with."""
    if attn_seed is not None:
        return int(attn_seed)
    return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())


def gat_edge_softmax_heads(graph: CSRGraph, s_dst: torch.Tensor, s_src: torch.Tensor,
                           negative_slope: float = 0.2) -> torch.Tensor:
    """alpha [H, E] float32 of H GAT heads from their scores s_dst [H, V], s_src [H, V]: one
    multi-head pass (GATEdgeSoftmaxHeads) or the single-head pass on each head's contiguous
    slice, stacked, as mk.heads_softmax_route says.  The two give the same alpha, byte for byte,
    and gradients within the kernels' bounds of each other."""
    s_dst, s_src = s_dst.contiguous(), s_src.contiguous()
    if mk.heads_softmax_route(s_dst.shape[0], graph.indptr.numel() - 1,
                              graph.indices.numel()) == "heads":
        return GATEdgeSoftmaxHeads.apply(graph.indptr, graph.indices, s_dst, s_src,
                                         negative_slope)
    return torch.stack([GATEdgeSoftmax.apply(graph.indptr, graph.indices, s_dst[h], s_src[h],
                                             negative_slope) for h in range(s_dst.shape[0])])


class MaxKGATConv(nn.Module):
    """Single-head GAT on MaxK features:
    rst[v] = sum_{u in N(v)} alpha_vu fc(x_sparse[u]) + b,
    alpha_v. = softmax_u leaky_relu(attn_dst . fc(x_sparse[v]) + attn_src . fc(x_sparse[u])).
    As everywhere here the aggregation runs on the CBSR and the Linear after it (equal by
    linearity); the scores are x_sparse @ (fc.weight^T attn), two [V] vectors, and the
    coefficients come from them in one HIP pass (gat_edge_softmax).  Gradients reach fc.weight
    and both attention vectors, x_sparse through the scores and topk_values through the
    aggregation (its feature backward, edge_weight_grad and the softmax backward).  The
    reference has no GAT: there is no reference_compat.

    attn_drop: the GAT's dropout of alpha between the softmax and the aggregation, in training
    mode, through mk.edge_dropout_heads at one head (see MaxKMultiHeadGATConv);
    forward(..., attn_seed=) fixes the mask's seed."""

    def __init__(self, in_feats: int, out_feats: int, negative_slope: float = 0.2,
                 bias: bool = True, activation=None, attn_drop: float = 0.0):
        super().__init__()
        self.attn_drop = _check_attn_drop(attn_drop)
        self.in_feats, self.out_feats = in_feats, out_feats
        self.negative_slope = float(negative_slope)
        self.fc = nn.Linear(in_feats, out_feats, bias=False)
        self.attn_src = nn.Parameter(torch.empty(out_feats))
        self.attn_dst = nn.Parameter(torch.empty(out_feats))
        self.bias = nn.Parameter(torch.zeros(out_feats)) if bias else None
        self.activation = activation
        gain = nn.init.calculate_gain("relu")  # as the usual GATConv: Xavier-normal, ReLU gain
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        with torch.no_grad():
            nn.init.xavier_normal_(self.attn_src.view(1, -1), gain=gain)
            nn.init.xavier_normal_(self.attn_dst.view(1, -1), gain=gain)

    def forward(self, graph: CSRGraph, x_sparse, topk_values, topk_indices,
                attn_seed: Optional[int] = None):
        # attn . fc(x) = x . (fc.weight^T attn): both scores from one [V, in] x [in, 2] product
        v = self.fc.weight.t() @ torch.stack((self.attn_dst, self.attn_src), 1)
        s = x_sparse @ v
        alpha = gat_edge_softmax(graph, s[:, 0], s[:, 1], self.negative_slope)
        if self.training and self.attn_drop > 0:
            alpha = maxk_edge_dropout_heads(alpha.view(1, -1), self.attn_drop,
                                            attn_seed_of(attn_seed)).view(-1)
        agg = graph.aggregate(topk_values, topk_indices, self.in_feats, values=alpha,
                              row_div=None)
        rst = linear(agg, self.fc)
        if self.bias is not None:
            rst = rst + self.bias
        if self.activation is not None:
            rst = self.activation(rst)
        return rst


class MaxKMultiHeadGATConv(nn.Module):
    """GAT with num_heads heads on MaxK features; returns [V, num_heads, out_feats], as the
    usual multi-head GATConv does:
    rst[v, h] = sum_{u in N(v)} alpha_hvu W_h x_sparse[u] + b_h,
    alpha_hv. = softmax_u leaky_relu(attn_dst[h] . W_h x_sparse[v]
                                     + attn_src[h] . W_h x_sparse[u]),
    W_h = fc.weight[h * out_feats:(h + 1) * out_feats].  The scores of all heads come from one
    [V, in] x [in, 2H] product, alpha [H, E] from the HIP softmax per head, and the aggregation
    of all heads from one multi-head call on the CBSR (CSRGraph.aggregate_heads: one record
    gather per edge whatever H), agg [H, V, in]; the Linear follows it as one bmm.  Gradients
    reach fc.weight, both attention matrices, x_sparse through the scores and topk_values
    through the aggregation.

    attention="stored" (the default) keeps alpha [H, E] between forward and backward;
    attention="fused" computes the softmax inside the aggregation walk
    (CSRGraph.attend_heads), keeps the row statistics [H, V] instead and rebuilds alpha as a
    transient in the backward.  MAXK_HEADS_ATTN=fused|stored overrides the argument.
    attention_backward="fused" (with the fused attention only; the default is "rebuilt") runs
    that backward as one walk without alpha (CSRGraph.attend_heads(backward="fused"));
    MAXK_HEADS_ATTN_BWD=fused|rebuilt overrides the argument.

    attn_drop: the GAT's attention dropout, in training mode: every alpha_hvu is zeroed with
    probability attn_drop and the kept ones scaled by 1 / (1 - attn_drop), after the softmax's
    normalisation.  The mask is a pure function of (seed, head, edge) that every kernel
    recomputes (mk.edge_dropout_heads has the contract) and nothing stores, so it works with all
    three combinations of attention / attention_backward and adds no [H, E] tensor to the fused
    ones.  The stored path keeps two [H, E] tensors for its backward, alpha for the softmax
    backward and the dropped alpha for the aggregation: a known limit.  forward(...,
    attn_seed=None) draws a fresh seed per call (attn_seed_of); an int is used as given.  In
    eval() or with attn_drop == 0 the layer computes bitwise what it computes without the
    argument."""

    def __init__(self, in_feats: int, out_feats: int, num_heads: int,
                 negative_slope: float = 0.2, bias: bool = True, activation=None,
                 attention: str = "stored", attention_backward: str = "rebuilt",
                 attn_drop: float = 0.0):
        super().__init__()
        self.attn_drop = _check_attn_drop(attn_drop)
        if attention not in ("stored", "fused"):
            raise ValueError(f'attention must be "stored" or "fused", got {attention!r}')
        if attention_backward not in ("rebuilt", "fused"):
            raise ValueError('attention_backward must be "rebuilt" or "fused", got '
                             f'{attention_backward!r}')
        self.attention = attention
        self.attention_backward = attention_backward
        if not 1 <= int(num_heads) <= mk.MAX_HEADS:
            raise ValueError(f"num_heads must be in [1, {mk.MAX_HEADS}], got {num_heads}")
        self.in_feats, self.out_feats, self.num_heads = in_feats, out_feats, int(num_heads)
        self.negative_slope = float(negative_slope)
        self.fc = nn.Linear(in_feats, self.num_heads * out_feats, bias=False)
        self.attn_src = nn.Parameter(torch.empty(self.num_heads, out_feats))
        self.attn_dst = nn.Parameter(torch.empty(self.num_heads, out_feats))
        self.bias = nn.Parameter(torch.zeros(self.num_heads, out_feats)) if bias else None
        self.activation = activation
        gain = nn.init.calculate_gain("relu")  # as the usual GATConv: Xavier-normal, ReLU gain
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_src, gain=gain)
        nn.init.xavier_normal_(self.attn_dst, gain=gain)

    def attention_mode(self) -> str:
        """"fused" or "stored": MAXK_HEADS_ATTN when it names one, else the `attention`
        argument."""
        forced = os.environ.get("MAXK_HEADS_ATTN", "")
        return forced if forced in ("fused", "stored") else self.attention

    def attention_backward_mode(self) -> str:
        """"fused" or "rebuilt", the backward of the fused attention: MAXK_HEADS_ATTN_BWD when
        it names one, else the `attention_backward` argument.  Without effect where
        attention_mode() is "stored"."""
        forced = os.environ.get("MAXK_HEADS_ATTN_BWD", "")
        return forced if forced in ("fused", "rebuilt") else self.attention_backward

    def forward(self, graph: CSRGraph, x_sparse, topk_values, topk_indices,
                attn_seed: Optional[int] = None):
        H, O = self.num_heads, self.out_feats
        p = self.attn_drop if self.training else 0.0
        seed = attn_seed_of(attn_seed) if p > 0 else 0
        W = self.fc.weight.view(H, O, self.in_feats)
        # attn[h] . W_h x = x . (W_h^T attn[h]): every head's two scores from one product
        v = torch.cat((torch.einsum("hoi,ho->ih", W, self.attn_dst),
                       torch.einsum("hoi,ho->ih", W, self.attn_src)), 1)  # [in, 2H]
        s = (x_sparse @ v).t().contiguous()                               # [2H, V]
        if self.attention_mode() == "fused":
            agg = graph.attend_heads(topk_values, topk_indices, self.in_feats, s[:H], s[H:],
                                     self.negative_slope, self.attention_backward_mode(), p,
                                     seed)
        else:
            alpha = gat_edge_softmax_heads(graph, s[:H], s[H:], self.negative_slope)
            alpha = maxk_edge_dropout_heads(alpha, p, seed)
            agg = graph.aggregate_heads(topk_values, topk_indices, self.in_feats, alpha)
        rst = torch.bmm(agg, W.transpose(1, 2)).transpose(0, 1)          # [V, H, out]
        if self.bias is not None:
            rst = rst + self.bias
        if self.activation is not None:
            rst = self.activation(rst)
        return rst


class MaxKTransformerConv(nn.Module):
    """Scaled dot-product (graph transformer) attention with num_heads heads on MaxK features;
    returns [V, num_heads, out_feats]:
    rst[v, h] = sum_{u in N(v)} alpha_hvu W_v,h x_sparse[u] + b_h,
    alpha_hv. = softmax_u((W_q,h x_sparse[v]) . (W_k,h x_sparse[u]) / sqrt(out_feats)),
    W_*,h = fc_*.weight[h * out_feats:(h + 1) * out_feats].  The MaxK trick serves the keys as
    well as the values: (W_q x_v) . (W_k x_u) = q[h, v] . x_u with q[h] = (x_sparse W_q,h^T) W_k,h
    in the feature space [H, V, in], and x_u is the CBSR row -- so the score of an edge is a dot
    product of q with the packed record the aggregation gathers anyway.  As in
    MaxKMultiHeadGATConv the aggregation runs on the CBSR, agg [H, V, in], and W_v follows it as
    one bmm.  Gradients reach fc_q and fc_k through q (torch ops), fc_v, x_sparse through q and
    topk_values through the scores and the aggregation.

    attention="stored" (the default) computes the logits [H, E] (maxk_dot_scores_heads), their
    softmax per head and the aggregation over the stored coefficients; attention="fused" runs
    CSRGraph.dot_attend_heads, which keeps the row statistics [H, V] instead and rebuilds alpha
    as a transient in the backward.  MAXK_DOT_ATTN=fused|stored overrides the argument.

    attention_backward="fused" (with the fused attention only; the default is "rebuilt") runs
    that backward as one mk.dot_attention_heads_backward call, with no [H, E] tensor in the
    backward either; it keeps `agg` [H, V, in] alive until then.
    MAXK_DOT_ATTN_BWD=fused|rebuilt overrides the argument; mk.dot_attention_backward_route has
    the measurements.

    attn_drop: dropout of alpha after the softmax's normalisation, in training mode, under the
    mask of (seed, head, edge) (mk.edge_dropout_heads); forward(..., attn_seed=) fixes the seed.
    By default the stored path only: the fused walk then raises a ValueError in training mode.

    fused_attn_drop=True opts into the dropout inside the fused walk: in training mode with
    attn_drop > 0 and the fused attention the layer calls CSRGraph.dot_attend_heads(...,
    dropout=attn_drop, seed=...) in either backward mode -- the same mask as the stored path's
    for the same seed, only the two numbers kept for the backward and no [H, E] tensor anywhere
    with the fused backward.  In eval() or with attn_drop == 0 the keyword changes nothing.
    Flipping its default, which would retire the ValueError, is left to a later change."""

    def __init__(self, in_feats: int, out_feats: int, num_heads: int, bias: bool = True,
                 activation=None, attention: str = "stored", attn_drop: float = 0.0,
                 attention_backward: str = "rebuilt", fused_attn_drop: bool = False):
        super().__init__()
        self.attn_drop = _check_attn_drop(attn_drop)
        self.fused_attn_drop = bool(fused_attn_drop)
        if attention not in ("stored", "fused"):
            raise ValueError(f'attention must be "stored" or "fused", got {attention!r}')
        if attention_backward not in ("rebuilt", "fused"):
            raise ValueError('attention_backward must be "rebuilt" or "fused", got '
                             f'{attention_backward!r}')
        self.attention = attention
        self.attention_backward = attention_backward
        if not 1 <= int(num_heads) <= mk.MAX_HEADS:
            raise ValueError(f"num_heads must be in [1, {mk.MAX_HEADS}], got {num_heads}")
        self.in_feats, self.out_feats, self.num_heads = in_feats, out_feats, int(num_heads)
        self.scale = float(out_feats) ** -0.5
        self.fc_q = nn.Linear(in_feats, self.num_heads * out_feats, bias=False)
        self.fc_k = nn.Linear(in_feats, self.num_heads * out_feats, bias=False)
        self.fc_v = nn.Linear(in_feats, self.num_heads * out_feats, bias=False)
        self.bias = nn.Parameter(torch.zeros(self.num_heads, out_feats)) if bias else None
        self.activation = activation
        gain = nn.init.calculate_gain("relu")  # as the GAT layers: Xavier-normal, ReLU gain
        for fc in (self.fc_q, self.fc_k, self.fc_v):
            nn.init.xavier_normal_(fc.weight, gain=gain)

    def attention_mode(self) -> str:
        """"fused" or "stored": MAXK_DOT_ATTN when it names one, else the `attention`
        argument."""
        forced = os.environ.get("MAXK_DOT_ATTN", "")
        return forced if forced in ("fused", "stored") else self.attention

    def attention_backward_mode(self) -> str:
        """"fused" or "rebuilt", the backward of the fused attention: MAXK_DOT_ATTN_BWD when it
        names one, else the `attention_backward` argument.  Without effect where attention_mode()
        is "stored"."""
        forced = os.environ.get("MAXK_DOT_ATTN_BWD", "")
        return forced if forced in ("fused", "rebuilt") else self.attention_backward

    def forward(self, graph: CSRGraph, x_sparse, topk_values, topk_indices,
                attn_seed: Optional[int] = None):
        H, O, I = self.num_heads, self.out_feats, self.in_feats
        p = self.attn_drop if self.training else 0.0
        fused = self.attention_mode() == "fused"
        if fused and p > 0 and not self.fused_attn_drop:
            raise ValueError("MaxKTransformerConv: the fused walk has no dropout yet; use "
                             'attention="stored" with attn_drop > 0, or opt into the masked '
                             "fused walk with fused_attn_drop=True")
        Wq, Wk, Wv = (fc.weight.view(H, O, I) for fc in (self.fc_q, self.fc_k, self.fc_v))
        # (W_q x_v) . (W_k x_u) = ((x_v W_q^T) W_k) . x_u: the query in the feature space
        q = torch.matmul(torch.matmul(x_sparse, Wq.transpose(1, 2)), Wk)  # [H, V, in]
        if fused and p > 0:
            agg = graph.dot_attend_heads(topk_values, topk_indices, I, q, self.scale,
                                         self.attention_backward_mode(), dropout=p,
                                         seed=attn_seed_of(attn_seed))
        elif fused:
            agg = graph.dot_attend_heads(topk_values, topk_indices, I, q, self.scale,
                                         self.attention_backward_mode())
        else:
            logits = maxk_dot_scores_heads(graph.indptr, graph.indices, q, topk_values,
                                           topk_indices, self.scale)
            alpha = torch.stack([edge_softmax(graph, logits[h]) for h in range(H)])
            if p > 0:
                alpha = maxk_edge_dropout_heads(alpha, p, attn_seed_of(attn_seed))
            agg = graph.aggregate_heads(topk_values, topk_indices, I, alpha)
        rst = torch.bmm(agg, Wv.transpose(1, 2)).transpose(0, 1)          # [V, H, out]
        if self.bias is not None:
            rst = rst + self.bias
        if self.activation is not None:
            rst = self.activation(rst)
        return rst


class MaxKSAGE(nn.Module):
    """lin_in -> [MaxK -> MaxKSAGEConv] x L -> lin_out (model_integrated_v3.py:522-588; same
    constructor arguments; graph_name is accepted and unused: no schedule files are needed)."""

    def __init__(self, in_size: int, hid_size: int, num_hid_layers: int, out_size: int,
                 maxk: int = 32, feat_drop: float = 0.5, norm: bool = False,
                 nonlinear: str = "maxk", graph_name: str = "", reference_compat: bool = False):
        super().__init__()
        if nonlinear != "maxk":
            raise ValueError(f"Only 'maxk' supported, got {nonlinear}")
        self.k, self.num_layers, self.graph_name = maxk, num_hid_layers, graph_name
        self.reference_compat = reference_compat
        self.lin_in = nn.Linear(in_size, hid_size)
        self.layers = nn.ModuleList([
            MaxKSAGEConv(hid_size, hid_size, feat_drop=feat_drop,
                         norm=nn.LayerNorm(hid_size) if norm else None,
                         reference_compat=reference_compat)
            for _ in range(num_hid_layers)])
        self.lin_out = nn.Linear(hid_size, out_size)
        nn.init.xavier_uniform_(self.lin_in.weight)
        nn.init.xavier_uniform_(self.lin_out.weight)

    def forward(self, graph: CSRGraph, x):
        x = linear(x, self.lin_in)
        for layer in self.layers:
            x_sparse, vals, idx = maxk(x, self.k, self.reference_compat)
            x = layer(graph, x_sparse, vals, idx)
        return linear(x, self.lin_out)


class _MaxKStack(nn.Module):
    """Shared body of MaxKGCN / MaxKGIN (model_integrated_v3.py:590-752): lin_in + relu, then
    per layer Linear -> MaxK -> dropout -> conv (-> LayerNorm), then lin_out."""

    def __init__(self, in_size, hid_size, num_hid_layers, out_size, maxk, feat_drop, norm,
                 nonlinear, graph_name, reference_compat, make_conv):
        super().__init__()
        if nonlinear != "maxk":
            raise ValueError(f"Only 'maxk' supported, got {nonlinear}")
        self.k, self.num_layers, self.graph_name = maxk, num_hid_layers, graph_name
        self.reference_compat = reference_compat
        self.dropoutlayers = nn.ModuleList([nn.Dropout(feat_drop) for _ in range(num_hid_layers)])
        self.convs = nn.ModuleList([make_conv() for _ in range(num_hid_layers)])
        self.normlayers = nn.ModuleList([nn.LayerNorm(hid_size) for _ in range(num_hid_layers)]
                                        if norm else [])
        self.linlayers = nn.ModuleList([nn.Linear(hid_size, hid_size)
                                        for _ in range(num_hid_layers)])
        for lin in self.linlayers:
            nn.init.xavier_uniform_(lin.weight)
        self.lin_in = nn.Linear(in_size, hid_size)
        self.lin_out = nn.Linear(hid_size, out_size)
        nn.init.xavier_uniform_(self.lin_in.weight)
        nn.init.xavier_uniform_(self.lin_out.weight)

    def forward(self, graph: CSRGraph, x):
        x = linear(x, self.lin_in).relu()
        for i in range(self.num_layers):
            x = linear(x, self.linlayers[i])
            x_sparse, vals, idx = maxk(x, self.k, self.reference_compat)
            if self.reference_compat:  # :661, :743: the kernel gets the undropped values
                x_sparse = self.dropoutlayers[i](x_sparse)
            else:
                x_sparse, vals = _dropped_values(x_sparse, vals, idx, self.dropoutlayers[i])
            x = self.convs[i](graph, x_sparse, vals, idx)
            if self.normlayers:
                x = self.normlayers[i](x)
        return linear(x, self.lin_out)


class MaxKGCN(_MaxKStack):
    """GCN model (model_integrated_v3.py:590-670): MaxKGraphConv(norm="both", no weight, no
    bias) after a per-layer Linear."""

    def __init__(self, in_size: int, hid_size: int, num_hid_layers: int, out_size: int,
                 maxk: int = 32, feat_drop: float = 0.5, norm: bool = False,
                 nonlinear: str = "maxk", graph_name: str = "", reference_compat: bool = False):
        super().__init__(in_size, hid_size, num_hid_layers, out_size, maxk, feat_drop, norm,
                         nonlinear, graph_name, reference_compat,
                         lambda: MaxKGraphConv(hid_size, hid_size, norm="both", weight=False,
                                               bias=False, reference_compat=reference_compat))

    @property
    def gcnlayers(self):
        return self.convs


class MaxKGIN(_MaxKStack):
    """GIN model (model_integrated_v3.py:672-752): MaxKGINConv(sum, learnable eps from 0)
    after a per-layer Linear."""

    def __init__(self, in_size: int, hid_size: int, num_hid_layers: int, out_size: int,
                 maxk: int = 32, feat_drop: float = 0.5, norm: bool = False,
                 nonlinear: str = "maxk", graph_name: str = "", reference_compat: bool = False):
        super().__init__(in_size, hid_size, num_hid_layers, out_size, maxk, feat_drop, norm,
                         nonlinear, graph_name, reference_compat,
                         lambda: MaxKGINConv(None, init_eps=0.0, learn_eps=True,
                                             reference_compat=reference_compat))

    @property
    def ginlayers(self):
        return self.convs
