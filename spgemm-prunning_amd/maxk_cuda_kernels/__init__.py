"""maxk_cuda_kernels -- MI355X-native drop-in for the reference extension of the same name.

Same function names, argument names, defaults and return shapes as the
reference's pybind11 module (cuda_kernel_bindings.cpp:429-490, plus the v2
additions load_warp4_metadata_csc / validate_spmm_maxk_backward,
binding_v2.py:320-351,464-486).  Every compute call goes to hand-written HIP
kernels for gfx950 in libmaxk_hip.so through its C ABI (include/maxk_hip.h);
there is no CPU or PyTorch fallback.

Differences from the reference, all deliberate (DESIGN.md "Boundary"):
  * launches go on torch's *current* HIP stream, not the legacy default stream;
  * `dim_origin` (the dense width D) is a keyword argument defaulting to the
    reference's hard-coded 256 (cuda_kernel_bindings.cpp:70) instead of a constant;
  * the kernels consume the CSR row_ptr; `spmm_maxk_forward/backward` accept the
    reference's warp4 metadata and derive row_ptr from it on the GPU (or take
    `indptr=` directly);
  * results are exact for every k in [1, D] (the reference drops rows / reads
    stale shared memory for k < 32);
  * cuda_topk_maxk_float is an exact top-k (the reference quantises to uint8).
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import warnings
from typing import List, NamedTuple, Optional, Tuple

import torch

from . import _capi
from ._cache import TensorCache

_L = _capi.load()  # ImportError here <=> extension missing (callers test this, like the reference)

__all__ = [
    "spmm_maxk_forward", "spmm_maxk_backward", "cuda_topk_maxk", "cuda_topk_maxk_float",
    "topk_u8_reference",
    "records_ok",
    "cbsr_records",
    "spgemm_forward_records",
    "prepare_cbsr_format_maxk", "cusparse_spmm", "load_warp4_metadata",
    "load_warp4_metadata_csc", "generate_sparse_selector", "benchmark_spmm_maxk",
    "validate_spmm_maxk", "validate_spmm_maxk_backward", "CudaTimer",
    # MI355X additions
    "topk_cbsr", "cbsr_scatter_dense", "topk_cbsr_dense", "topk_backward", "topk_error_rows",
    "build_warp4_metadata", "warp4_to_indptr",
    "spgemm_forward", "sspmm_backward", "edge_weight_grad", "graph_only_mode", "DenseSpMMPlan",
    "edge_softmax", "edge_softmax_backward", "gat_edge_softmax", "gat_edge_softmax_backward",
    "spgemm_forward_heads", "edge_weight_grad_heads", "MAX_HEADS", "heads_forward_route",
    "sspmm_backward_heads", "heads_backward_route",
    "gat_edge_softmax_heads", "gat_edge_softmax_heads_backward", "heads_softmax_route",
    "gat_attention_heads", "gat_edge_alpha_heads", "heads_attention_route",
    "gat_attention_heads_backward", "heads_attention_backward_route", "edge_dropout_heads",
    "dot_attention_heads", "dot_edge_alpha_heads", "dot_attention_heads_backward",
    "dot_attention_backward_route",
    "spgemm_max_forward", "spgemm_max_backward",
    "version", "device_count",
    "transpose_plan", "bsort_plan", "pull_plan", "edge_selector_mode", "backward_plan", "BWD_MODES",
    "dense_plan", "hybrid_plan", "pull_locality", "edge_selectors_wanted",
    "pull_stream_plan", "pull_stream_buckets", "PullStreamPlan",
]

FULL_DIM = 256  # the reference binding's fixed output width (cuda_kernel_bindings.cpp:70)


def _lib():
    return _L


def version() -> int:
    return _lib().maxk_version()


def device_count() -> int:
    return _lib().maxk_device_count()


def _validate_mode() -> str:
    """MAXK_VALIDATE: unset -> check each graph once (cached per tensor, like the transpose
    plan); "1" -> check every call (graph and selectors); "0" -> never check."""
    v = os.environ.get("MAXK_VALIDATE", "")
    return "once" if v == "" else ("never" if v == "0" else "always")


def _validate_default() -> bool:
    return _validate_mode() == "always"


_CHECKED = TensorCache()


def _check_graph_once(row_ptr, col_idx, num_cols):
    """Out-of-range row_ptr / col_idx are the only inputs that can make a kernel read out of
    bounds, so each graph is validated the first time it is used; the check is cached on the
    tensors' identity and versions.  Selectors change every call and are not checked here:
    a selector >= D contributes nothing in every kernel (the forward sends it to a trash
    column, the two-phase and atomic backwards read a zeroed LDS slot, the pull backward
    gathers 0 for it), so it cannot read outside G or another row of it."""
    def build():
        _validate_graph(row_ptr, col_idx, num_cols, col_idx.numel())
        return True  # the entry says: checked
    _CHECKED.get((row_ptr, col_idx), (int(num_cols),), build)


def _validate_call(validate, row_ptr, col_idx, num_cols, sel, D):
    if validate is False:
        return  # no check asked for: no need to ask whether one could run
    if torch.cuda.is_current_stream_capturing():
        return  # a range check synchronises the host: impossible inside a hipGraph capture
    if validate if validate is not None else _validate_default():
        _validate_graph(row_ptr, col_idx, num_cols, col_idx.numel())
        _validate_selector(sel, D)
    elif validate is None and _validate_mode() == "once":
        _check_graph_once(row_ptr, col_idx, num_cols)


def _ptr(t: Optional[torch.Tensor]):
    # a plain int: ctypes converts it for the c_void_p argument (no c_void_p object per call)
    return t.data_ptr() if t is not None and t.numel() > 0 else None


def _need(t, name, dtype=None):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be CUDA tensor")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"{name} must be {str(dtype).replace('torch.', '')}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _stream(dev):
    """torch's current HIP stream on `dev` as a raw pointer (int).  The raw accessor skips the
    torch.cuda.Stream object torch.cuda.current_stream() builds per call (~3 us of the ~20 us
    a small graph's call spent on the host, tools/host_profile.py)."""
    return torch._C._cuda_getCurrentRawStream(
        dev.index if dev.index is not None else torch.cuda.current_device())


_NO_SWITCH = contextlib.nullcontext()


def _on(dev):
    """torch.cuda.device(dev), or nothing when dev is already the current device (the
    context manager costs ~2.6 us per call).  `dev` holds a tensor, so HIP is initialised and
    the raw accessor serves, as in _stream."""
    cur = torch._C._cuda_getDevice()
    return _NO_SWITCH if dev.index is None or dev.index == cur else torch.cuda.device(dev)


def _launch(dev, name, *args):
    """The C-ABI call `name`(*args) with `dev` current; raises on a non-zero status."""
    with _on(dev):
        _capi.check(getattr(_L, name)(*args), name)


def _sized(dev, name, *args) -> int:
    """A size the library derives from the *current* device (its CU count): asked with `dev`
    current, like the launch it sizes."""
    with _on(dev):
        return int(getattr(_L, name)(*args))


def _workspace(dev, size_name, *size_args) -> torch.Tensor:
    """uint8 scratch on `dev` of `size_name`(*size_args) bytes (never empty)."""
    return torch.empty(max(_sized(dev, size_name, *size_args), 1), dtype=torch.uint8, device=dev)


def _launch_ws(dev, name, size_name, size_args, args, tail=()):
    """_workspace and _launch under one device switch, for a call that runs straight after its
    size query: `name`(*args, workspace, its bytes, torch's current stream on dev, *tail)."""
    with _on(dev):
        n = max(getattr(_L, size_name)(*size_args), 1)
        ws = torch.empty(n, dtype=torch.uint8, device=dev)
        _capi.check(getattr(_L, name)(*args, ws.data_ptr(), n, _stream(dev), *tail), name)


def _validate_graph(row_ptr, col_idx, num_cols, num_e):
    if row_ptr.numel() == 0:
        raise RuntimeError("row_ptr must have num_rows+1 entries")
    if int(row_ptr[0]) != 0 or int(row_ptr[-1]) != num_e:
        raise RuntimeError(f"row_ptr must start at 0 and end at num_e={num_e}")
    if row_ptr.numel() > 1 and bool((row_ptr[1:] < row_ptr[:-1]).any()):
        raise RuntimeError("row_ptr must be non-decreasing")
    if num_e and (int(col_idx.min()) < 0 or int(col_idx.max()) >= num_cols):
        raise RuntimeError(f"col_idx out of range [0, {num_cols})")


def _validate_selector(sel, D):
    if sel.numel() and int(sel.max()) >= D:
        raise RuntimeError(f"sparse_selector entries must be < dim_origin={D}")


# --------------------------------------------------------------------------- schedule
def warp4_to_indptr(warp4_metadata: torch.Tensor, num_v: int,
                    num_warps: Optional[int] = None) -> torch.Tensor:
    """CSR row_ptr [num_v+1] described by a warp4 array (first `num_warps` entries)."""
    _need(warp4_metadata, "warp4_metadata", torch.int32)
    W = warp4_metadata.numel() // 4 if num_warps is None else min(int(num_warps),
                                                                   warp4_metadata.numel() // 4)
    row_ptr = torch.empty(num_v + 1, dtype=torch.int32, device=warp4_metadata.device)
    _launch(warp4_metadata.device, "maxk_warp4_to_row_ptr", _ptr(warp4_metadata), W, num_v,
            _ptr(row_ptr), _stream(warp4_metadata.device))
    return row_ptr


def build_warp4_metadata(indptr: torch.Tensor, warp_max_nz: int = 64) -> torch.Tensor:
    """warp4 schedule built on the GPU (kernels/generate_meta.py:30-48 semantics).
    Returns flat int32 [4W] on the device of `indptr` -- the layout of a .warp4 file."""
    _need(indptr, "indptr", torch.int32)
    dev = indptr.device
    V = indptr.numel() - 1
    n = ctypes.c_int64(0)
    _launch(dev, "maxk_warp4_count", _ptr(indptr), V, warp_max_nz, ctypes.byref(n), _stream(dev))
    out = torch.empty(4 * n.value, dtype=torch.int32, device=dev)
    _launch_ws(dev, "maxk_warp4_build", "maxk_warp4_build_workspace_size", (V,),
               (_ptr(indptr), V, warp_max_nz, _ptr(out), n.value))
    return out


def _read_warp4_file(path: str, device="cuda") -> torch.Tensor:
    if not os.path.exists(path):
        raise RuntimeError(f"Cannot open warp4 file: {path}")
    import numpy as np
    data = np.fromfile(path, dtype=np.int32)
    return torch.from_numpy(data).to(device)


def load_warp4_metadata(graph_name: str, num_warps: int = 12, warp_max_nz: int = 64) -> torch.Tensor:
    """Read kernels/w{num_warps}_nz{warp_max_nz}_warp_4/<graph>.warp4 (CWD-relative) into
    an int32 CUDA tensor -- cuda_kernel_bindings.cpp:287-317."""
    path = f"kernels/w{num_warps}_nz{warp_max_nz}_warp_4/{graph_name}.warp4"
    return _read_warp4_file(path)


def load_warp4_metadata_csc(graph_name: str, num_warps: int = 12,
                            warp_max_nz: int = 64) -> torch.Tensor:
    """CSC twin, binding_v2.py:320-351 (kernels/w12_nz64_warp_4_csc/<graph>.warp4_csc)."""
    path = f"kernels/w{num_warps}_nz{warp_max_nz}_warp_4_csc/{graph_name}.warp4_csc"
    return _read_warp4_file(path)


# --------------------------------------------------------------------------- hot path
def _forward_common(indptr, indices, values, num_cols, k, sel, D, row_div, chunk, out, accumulate,
                    validate, dev):
    """What spgemm_forward and spgemm_forward_records share once their own operands passed: the
    other input checks and `out`.  Returns (out, (num_rows, num_cols, E, D, k, chunk)), the
    shape arguments of both the kernel and its workspace size."""
    if values.numel() != indices.numel():
        raise RuntimeError("values and indices must have the same length")
    num_rows = indptr.numel() - 1
    if row_div is not None:
        _need(row_div, "row_div", torch.float32)
        if row_div.numel() != num_rows:
            raise RuntimeError("row_div must have num_rows entries")
    _validate_call(validate, indptr, indices, num_cols, sel, D)
    if out is None:
        if accumulate:
            raise RuntimeError("accumulate=True needs out=")
        out = torch.empty(num_rows, D, dtype=torch.float32, device=dev)
    else:
        _need(out, "out", torch.float32)
        if tuple(out.shape) != (num_rows, D):
            raise RuntimeError("out must be [num_rows, dim_origin]")
    return out, (num_rows, num_cols, indices.numel(), D, k, chunk)


def spgemm_forward(indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor,
                   cbsr_val: torch.Tensor, cbsr_idx: torch.Tensor, dim_origin: int,
                   row_div: Optional[torch.Tensor] = None, chunk: int = 0,
                   out: Optional[torch.Tensor] = None, validate: Optional[bool] = None,
                   accumulate: bool = False, edge_sel_out: Optional[torch.Tensor] = None
                   ) -> torch.Tensor:
    """out[num_rows, D] = diag(1/row_div) . A . scatter(cbsr)  (CSR A: indptr/indices/values).
    accumulate: out += the product instead (out= required; maxk_spgemm_forward_accumulate).
    edge_sel_out (uint8 [E, k]): also store each edge's selectors, cbsr_idx[indices[e]], for
    sspmm_backward(..., edge_sel=) (maxk_spgemm_forward_sel; with accumulate,
    maxk_spgemm_forward_accumulate_sel)."""
    for t, n, dt in ((indptr, "indptr", torch.int32), (indices, "indices", torch.int32),
                     (values, "values", torch.float32), (cbsr_val, "input_data", torch.float32),
                     (cbsr_idx, "sparse_selector", torch.uint8)):
        _need(t, n, dt)
    num_cols, k = (cbsr_val.shape[0], cbsr_val.shape[1]) if cbsr_val.dim() == 2 else (0, 0)
    if cbsr_idx.shape != cbsr_val.shape:
        raise RuntimeError("input_data and sparse_selector must have the same [V, k] shape")
    out, shape = _forward_common(indptr, indices, values, num_cols, k, cbsr_idx, int(dim_origin),
                                 row_div, chunk, out, accumulate, validate, cbsr_val.device)
    tail = ()
    if edge_sel_out is not None:
        _need(edge_sel_out, "edge_sel_out", torch.uint8)
        if tuple(edge_sel_out.shape) != (shape[2], k):
            raise RuntimeError("edge_sel_out must be [num_e, k]")
        tail = (_ptr(edge_sel_out),)
    _launch_ws(cbsr_val.device, "maxk_spgemm_forward" + ("_accumulate" if accumulate else "")
               + ("_sel" if tail else ""), "maxk_spgemm_forward_workspace_size", shape,
               (_ptr(indptr), _ptr(indices), _ptr(values), _ptr(cbsr_val), _ptr(cbsr_idx),
                _ptr(row_div), _ptr(out), *shape), tail)
    return out


def edge_weight_grad(indptr: torch.Tensor, indices: torch.Tensor, cbsr_val: torch.Tensor,
                     cbsr_idx: torch.Tensor, grad_output: torch.Tensor,
                     row_div: Optional[torch.Tensor] = None, chunk: int = 0,
                     out: Optional[torch.Tensor] = None,
                     validate: Optional[bool] = None) -> torch.Tensor:
    """grad_edge[E] float32: the forward's gradient with respect to the edge weights,
    grad_edge[e] = sum_l cbsr_val[c, l] * grad_output[r, cbsr_idx[c, l]] / row_div[r] for edge
    e of row r into column c = indices[e] (maxk_edge_weight_grad): the adjoint of
    spgemm_forward in `values`, which it does not read.  Any k <= D <= 256; bitwise
    repeatable.  The same operand checks as spgemm_forward / sspmm_backward."""
    for t, n, dt in ((indptr, "indptr", torch.int32), (indices, "indices", torch.int32),
                     (cbsr_val, "input_data", torch.float32),
                     (cbsr_idx, "sparse_selector", torch.uint8),
                     (grad_output, "grad_output", torch.float32)):
        _need(t, n, dt)
    if cbsr_val.dim() != 2 or cbsr_idx.shape != cbsr_val.shape:
        raise RuntimeError("input_data and sparse_selector must have the same [V, k] shape")
    num_cols, k = cbsr_val.shape
    num_rows = indptr.numel() - 1
    if grad_output.dim() != 2 or grad_output.shape[0] != num_rows:
        raise RuntimeError("grad_output must be [num_rows, dim_origin]")
    D = grad_output.shape[1]
    if row_div is not None:
        _need(row_div, "row_div", torch.float32)
        if row_div.numel() != num_rows:
            raise RuntimeError("row_div must have num_rows entries")
    _validate_call(validate, indptr, indices, num_cols, cbsr_idx, D)
    E = indices.numel()
    dev = grad_output.device
    if out is None:
        out = torch.empty(E, dtype=torch.float32, device=dev)
    else:
        _need(out, "out", torch.float32)
        if tuple(out.shape) != (E,):
            raise RuntimeError("out must be [num_e]")
    shape = (num_rows, num_cols, E, D, k, chunk)
    _launch_ws(dev, "maxk_edge_weight_grad", "maxk_edge_weight_grad_workspace_size", shape,
               (_ptr(indptr), _ptr(indices), _ptr(cbsr_val), _ptr(cbsr_idx), _ptr(grad_output),
                _ptr(row_div), _ptr(out), *shape))
    return out


MAX_HEADS = 8  # MAXK_MAX_HEADS (maxk_hip.h)


def _heads_operands(indptr, indices, cbsr_val, cbsr_idx, row_div, validate, D):
    """The operand checks the two multi-head calls share; returns (num_rows, num_cols, k)."""
    for t, n, dt in ((indptr, "indptr", torch.int32), (indices, "indices", torch.int32),
                     (cbsr_val, "input_data", torch.float32),
                     (cbsr_idx, "sparse_selector", torch.uint8)):
        _need(t, n, dt)
    if cbsr_val.dim() != 2 or cbsr_idx.shape != cbsr_val.shape:
        raise RuntimeError("input_data and sparse_selector must have the same [V, k] shape")
    num_cols, k = cbsr_val.shape
    num_rows = indptr.numel() - 1
    if row_div is not None:
        _need(row_div, "row_div", torch.float32)
        if row_div.numel() != num_rows:
            raise RuntimeError("row_div must have num_rows entries")
    _validate_call(validate, indptr, indices, num_cols, cbsr_idx, D)
    return num_rows, num_cols, k


def _heads_out(out, shape, dev, what):
    if out is None:
        return torch.empty(*shape, dtype=torch.float32, device=dev)
    _need(out, "out", torch.float32)
    if tuple(out.shape) != tuple(shape):
        raise RuntimeError(f"out must be {what}")
    return out


def spgemm_forward_heads(indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor,
                         cbsr_val: torch.Tensor, cbsr_idx: torch.Tensor, dim_origin: int,
                         row_div: Optional[torch.Tensor] = None, chunk: int = 0,
                         out: Optional[torch.Tensor] = None,
                         validate: Optional[bool] = None) -> torch.Tensor:
    """out[H, num_rows, D]: spgemm_forward for H sets of edge weights, values [H, E], over one
    graph and one CBSR, with one record gather per edge serving all heads
    (maxk_spgemm_forward_heads).  1 <= H <= MAX_HEADS; row_div is shared by the heads.  Head
    h's slice equals, within the forward's bound, spgemm_forward(..., values[h], ...); bitwise
    repeatable.  The same operand checks as spgemm_forward."""
    D = int(dim_origin)
    _need(values, "values", torch.float32)
    num_rows, num_cols, k = _heads_operands(indptr, indices, cbsr_val, cbsr_idx, row_div,
                                            validate, D)
    E = indices.numel()
    if values.dim() != 2 or values.shape[1] != E or not 1 <= values.shape[0] <= MAX_HEADS:
        raise RuntimeError(f"values must be [H, num_e] with 1 <= H <= {MAX_HEADS}")
    H = values.shape[0]
    dev = cbsr_val.device
    out = _heads_out(out, (H, num_rows, D), dev, "[H, num_rows, dim_origin]")
    shape = (num_rows, num_cols, E, D, k, H, chunk)
    _launch_ws(dev, "maxk_spgemm_forward_heads", "maxk_spgemm_forward_heads_workspace_size", shape,
               (_ptr(indptr), _ptr(indices), _ptr(values), _ptr(cbsr_val), _ptr(cbsr_idx),
                _ptr(row_div), _ptr(out), *shape))
    return out


HEADS_SPARSE_DEGREE = 128  # kFwdSparseDegree (cbsr_pack.h): below it a graph is "sparse"


def heads_forward_route(num_rows: int, num_e: int) -> str:
    """How a multi-head aggregation's forward runs (CSRGraph.aggregate_heads, maxk_spgemm_heads):
    "heads", one spgemm_forward_heads call, on a sparse graph (average degree below
    HEADS_SPARSE_DEGREE), where the record gathers are random memory lines and sharing them
    pays -- ogbn-products-sized, k = 32: 0.84 (H = 4) and 0.81 (H = 8) of the H single-head
    calls; "calls", H spgemm_forward calls into the slices of one output, on a dense one, whose
    records stay in the caches -- Reddit-sized, k = 16: 1.00 and 0.99, inside the run-to-run
    spread (profiles/r12/heads/).  The weight gradient takes
    edge_weight_grad_heads everywhere (0.52 to 0.62).  MAXK_HEADS_FWD=heads|calls forces one."""
    forced = os.environ.get("MAXK_HEADS_FWD", "")
    if forced in ("heads", "calls"):
        return forced
    return "heads" if num_e < HEADS_SPARSE_DEGREE * num_rows else "calls"


def edge_weight_grad_heads(indptr: torch.Tensor, indices: torch.Tensor, cbsr_val: torch.Tensor,
                           cbsr_idx: torch.Tensor, grad_output: torch.Tensor,
                           row_div: Optional[torch.Tensor] = None, chunk: int = 0,
                           out: Optional[torch.Tensor] = None,
                           validate: Optional[bool] = None) -> torch.Tensor:
    """grad_edge[H, E]: edge_weight_grad for H gradients grad_output [H, num_rows, D] of
    spgemm_forward_heads, with one record gather per edge serving all heads
    (maxk_edge_weight_grad_heads).  Head h's slice is bitwise edge_weight_grad(...,
    grad_output[h], ...)."""
    _need(grad_output, "grad_output", torch.float32)
    if grad_output.dim() != 3 or not 1 <= grad_output.shape[0] <= MAX_HEADS:
        raise RuntimeError(f"grad_output must be [H, num_rows, dim_origin] with 1 <= H <= "
                           f"{MAX_HEADS}")
    H, _, D = grad_output.shape
    num_rows, num_cols, k = _heads_operands(indptr, indices, cbsr_val, cbsr_idx, row_div,
                                            validate, D)
    if grad_output.shape[1] != num_rows:
        raise RuntimeError("grad_output must be [H, num_rows, dim_origin]")
    E = indices.numel()
    dev = grad_output.device
    out = _heads_out(out, (H, E), dev, "[H, num_e]")
    shape = (num_rows, num_cols, E, D, k, H, chunk)
    _launch_ws(dev, "maxk_edge_weight_grad_heads", "maxk_edge_weight_grad_heads_workspace_size",
               shape, (_ptr(indptr), _ptr(indices), _ptr(cbsr_val), _ptr(cbsr_idx),
                       _ptr(grad_output), _ptr(row_div), _ptr(out), *shape))
    return out


def _validate_rows(validate, indptr, indices, num_cols, num_e):
    """The edge softmax's graph check, under the rules of _validate_call: the CSR's ranges once
    per graph by default (indices None: the plain form, which reads no column -- row_ptr alone,
    every call it is asked for), never inside a capture."""
    if validate is False or torch.cuda.is_current_stream_capturing():
        return
    always = validate if validate is not None else _validate_default()
    if indices is None:
        if always or _validate_mode() == "once":
            def build():
                if indptr.numel() == 0 or int(indptr[0]) != 0 or int(indptr[-1]) != num_e:
                    raise RuntimeError(f"row_ptr must start at 0 and end at num_e={num_e}")
                if bool((indptr[1:] < indptr[:-1]).any()):
                    raise RuntimeError("row_ptr must be non-decreasing")
                return True
            if always:
                build()
            else:
                _CHECKED.get((indptr,), (int(num_e),), build)
    elif always:
        _validate_graph(indptr, indices, num_cols, num_e)
    elif _validate_mode() == "once":
        _check_graph_once(indptr, indices, num_cols)


def _edge_vector(out, E, dev, name="out"):
    if out is None:
        return torch.empty(E, dtype=torch.float32, device=dev)
    _need(out, name, torch.float32)
    if tuple(out.shape) != (E,):
        raise RuntimeError(f"{name} must be [num_e]")
    return out


def edge_softmax(indptr: torch.Tensor, logits: torch.Tensor, chunk: int = 0,
                 out: Optional[torch.Tensor] = None,
                 validate: Optional[bool] = None) -> torch.Tensor:
    """w[E] float32: the softmax of `logits` over every CSR row (a destination's incoming edges),
    maxk_edge_softmax.  Rows without edges write nothing; bitwise repeatable."""
    _need(indptr, "indptr", torch.int32)
    _need(logits, "logits", torch.float32)
    E = logits.numel()
    if logits.dim() != 1:
        raise RuntimeError("logits must be [num_e]")
    _validate_rows(validate, indptr, None, 0, E)
    dev = logits.device
    out = _edge_vector(out, E, dev)
    shape = (indptr.numel() - 1, 0, E, chunk)
    _launch_ws(dev, "maxk_edge_softmax", "maxk_edge_softmax_workspace_size", shape,
               (_ptr(indptr), _ptr(logits), _ptr(out), *shape))
    return out


def edge_softmax_backward(indptr: torch.Tensor, w: torch.Tensor, grad_w: torch.Tensor,
                          chunk: int = 0, out: Optional[torch.Tensor] = None,
                          validate: Optional[bool] = None) -> torch.Tensor:
    """grad_logits[E] = w * (grad_w - sum over the row of w * grad_w), from the forward's w
    (maxk_edge_softmax_backward); no atomics, bitwise repeatable."""
    _need(indptr, "indptr", torch.int32)
    _need(w, "w", torch.float32)
    _need(grad_w, "grad_w", torch.float32)
    E = w.numel()
    if w.dim() != 1 or grad_w.shape != w.shape:
        raise RuntimeError("w and grad_w must be [num_e]")
    _validate_rows(validate, indptr, None, 0, E)
    dev = w.device
    out = _edge_vector(out, E, dev)
    shape = (indptr.numel() - 1, 0, E, chunk)
    _launch_ws(dev, "maxk_edge_softmax_backward", "maxk_edge_softmax_backward_workspace_size",
               shape, (_ptr(indptr), _ptr(w), _ptr(grad_w), _ptr(out), *shape))
    return out


def _gat_operands(indptr, indices, s_dst, s_src):
    for t, n, dt in ((indptr, "indptr", torch.int32), (indices, "indices", torch.int32),
                     (s_dst, "s_dst", torch.float32), (s_src, "s_src", torch.float32)):
        _need(t, n, dt)
    num_rows = indptr.numel() - 1
    if s_dst.dim() != 1 or s_dst.numel() != num_rows:
        raise RuntimeError("s_dst must be [num_rows]")
    if s_src.dim() != 1:
        raise RuntimeError("s_src must be [num_cols]")
    return num_rows, s_src.numel(), indices.numel()


def gat_edge_softmax(indptr: torch.Tensor, indices: torch.Tensor, s_dst: torch.Tensor,
                     s_src: torch.Tensor, negative_slope: float = 0.2, chunk: int = 0,
                     out: Optional[torch.Tensor] = None,
                     validate: Optional[bool] = None) -> torch.Tensor:
    """w[E] float32: the softmax over every CSR row of leaky_relu(s_dst[row] + s_src[indices[e]])
    (maxk_gat_edge_softmax): the attention coefficients of a single GAT head, from the two score
    vectors, without an E-sized intermediate.  Bitwise repeatable."""
    num_rows, num_cols, E = _gat_operands(indptr, indices, s_dst, s_src)
    _validate_rows(validate, indptr, indices, num_cols, E)
    dev = s_src.device
    out = _edge_vector(out, E, dev)
    shape = (num_rows, num_cols, E, chunk)
    _launch_ws(dev, "maxk_gat_edge_softmax", "maxk_gat_edge_softmax_workspace_size", shape,
               (_ptr(indptr), _ptr(indices), _ptr(s_dst), _ptr(s_src), float(negative_slope),
                _ptr(out), *shape))
    return out


def gat_edge_softmax_backward(indptr: torch.Tensor, indices: torch.Tensor, s_dst: torch.Tensor,
                              s_src: torch.Tensor, w: torch.Tensor, grad_w: torch.Tensor,
                              negative_slope: float = 0.2, chunk: int = 0,
                              out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                              validate: Optional[bool] = None):
    """(grad_s_dst [num_rows], grad_s_src [num_cols]) of gat_edge_softmax from its w and the
    gradient of w (maxk_gat_edge_softmax_backward).  The column sums go through the graph's
    transpose plan (transpose_plan, cached per `indices`) in CSC slot order: no atomics, bitwise
    repeatable; every element is written, 0 for a row without edges and a column no edge
    reads."""
    num_rows, num_cols, E = _gat_operands(indptr, indices, s_dst, s_src)
    _need(w, "w", torch.float32)
    _need(grad_w, "grad_w", torch.float32)
    if tuple(w.shape) != (E,) or tuple(grad_w.shape) != (E,):
        raise RuntimeError("w and grad_w must be [num_e]")
    _validate_rows(validate, indptr, indices, num_cols, E)
    dev = s_src.device
    col_ptr, csc_eid = transpose_plan(indices, num_cols)
    if out is None:
        g_dst = torch.empty(num_rows, dtype=torch.float32, device=dev)
        g_src = torch.empty(num_cols, dtype=torch.float32, device=dev)
    else:
        g_dst, g_src = out
        _need(g_dst, "out[0]", torch.float32)
        _need(g_src, "out[1]", torch.float32)
        if tuple(g_dst.shape) != (num_rows,) or tuple(g_src.shape) != (num_cols,):
            raise RuntimeError("out must be ([num_rows], [num_cols])")
    shape = (num_rows, num_cols, E, chunk)
    _launch_ws(dev, "maxk_gat_edge_softmax_backward",
               "maxk_gat_edge_softmax_backward_workspace_size", shape,
               (_ptr(indptr), _ptr(indices), _ptr(col_ptr), _ptr(csc_eid), _ptr(s_dst),
                _ptr(s_src), float(negative_slope), _ptr(w), _ptr(grad_w), _ptr(g_dst),
                _ptr(g_src), *shape))
    return g_dst, g_src


def _gat_heads_operands(indptr, indices, s_dst, s_src):
    for t, n, dt in ((indptr, "indptr", torch.int32), (indices, "indices", torch.int32),
                     (s_dst, "s_dst", torch.float32), (s_src, "s_src", torch.float32)):
        _need(t, n, dt)
    num_rows = indptr.numel() - 1
    if s_dst.dim() != 2 or not 1 <= s_dst.shape[0] <= MAX_HEADS or s_dst.shape[1] != num_rows:
        raise RuntimeError(f"s_dst must be [H, num_rows] with 1 <= H <= {MAX_HEADS}")
    if s_src.dim() != 2 or s_src.shape[0] != s_dst.shape[0]:
        raise RuntimeError("s_src must be [H, num_cols]")
    return s_dst.shape[0], num_rows, s_src.shape[1], indices.numel()


def gat_edge_softmax_heads(indptr: torch.Tensor, indices: torch.Tensor, s_dst: torch.Tensor,
                           s_src: torch.Tensor, negative_slope: float = 0.2, chunk: int = 0,
                           out: Optional[torch.Tensor] = None,
                           validate: Optional[bool] = None) -> torch.Tensor:
    """w[H, E] float32: gat_edge_softmax for H heads, s_dst [H, num_rows] and s_src
    [H, num_cols], over one walk of the graph: indices and a column's H scores are read once per
    edge (maxk_gat_edge_softmax_heads).  1 <= H <= MAX_HEADS.  Head h's slice is bitwise
    gat_edge_softmax(..., s_dst[h], s_src[h], ...) at the same chunk."""
    H, num_rows, num_cols, E = _gat_heads_operands(indptr, indices, s_dst, s_src)
    _validate_rows(validate, indptr, indices, num_cols, E)
    dev = s_src.device
    out = _heads_out(out, (H, E), dev, "[H, num_e]")
    shape = (num_rows, num_cols, E, chunk)
    _launch_ws(dev, "maxk_gat_edge_softmax_heads", "maxk_gat_edge_softmax_heads_workspace_size",
               (H,) + shape, (_ptr(indptr), _ptr(indices), _ptr(s_dst), _ptr(s_src),
                              float(negative_slope), _ptr(out), H, *shape))
    return out


def gat_edge_softmax_heads_backward(indptr: torch.Tensor, indices: torch.Tensor,
                                    s_dst: torch.Tensor, s_src: torch.Tensor, w: torch.Tensor,
                                    grad_w: torch.Tensor, negative_slope: float = 0.2,
                                    chunk: int = 0,
                                    out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                                    validate: Optional[bool] = None):
    """(grad_s_dst [H, num_rows], grad_s_src [H, num_cols]) of gat_edge_softmax_heads from its
    w [H, E] and the gradient of w (maxk_gat_edge_softmax_heads_backward): one read of indices,
    of a column's H scores and of a CSC slot's H values per edge.  The workspace holds an
    [E, HP] float buffer (HP = H rounded up to 2, 4 or 8), H times the single-head call's.
    Head h's slices equal gat_edge_softmax_backward on head h's slices within its bound, and
    bitwise at H = 1 (one head is the single-head call)."""
    H, num_rows, num_cols, E = _gat_heads_operands(indptr, indices, s_dst, s_src)
    _need(w, "w", torch.float32)
    _need(grad_w, "grad_w", torch.float32)
    if tuple(w.shape) != (H, E) or tuple(grad_w.shape) != (H, E):
        raise RuntimeError("w and grad_w must be [H, num_e]")
    _validate_rows(validate, indptr, indices, num_cols, E)
    dev = s_src.device
    col_ptr, csc_eid = transpose_plan(indices, num_cols)
    if out is None:
        g_dst = torch.empty(H, num_rows, dtype=torch.float32, device=dev)
        g_src = torch.empty(H, num_cols, dtype=torch.float32, device=dev)
    else:
        g_dst, g_src = out
        _need(g_dst, "out[0]", torch.float32)
        _need(g_src, "out[1]", torch.float32)
        if tuple(g_dst.shape) != (H, num_rows) or tuple(g_src.shape) != (H, num_cols):
            raise RuntimeError("out must be ([H, num_rows], [H, num_cols])")
    shape = (num_rows, num_cols, E, chunk)
    _launch_ws(dev, "maxk_gat_edge_softmax_heads_backward",
               "maxk_gat_edge_softmax_heads_backward_workspace_size", (H,) + shape,
               (_ptr(indptr), _ptr(indices), _ptr(col_ptr), _ptr(csc_eid), _ptr(s_dst),
                _ptr(s_src), float(negative_slope), _ptr(w), _ptr(grad_w), _ptr(g_dst),
                _ptr(g_src), H, *shape))
    return g_dst, g_src


def heads_softmax_route(num_heads: int, num_rows: int, num_e: int) -> str:
    """How the attention coefficients of a multi-head GAT layer are computed
    (maxk_layers.gat_edge_softmax_heads): "heads", one gat_edge_softmax_heads call and one
    backward, or "calls", the single-head pass per head.  "heads" from two heads on, on every
    graph: measured against the H calls in the same run, Reddit-sized and products-sized, at
    H = 2, 4 and 8, each direction gains 26 to 68 % against spreads of at most 3.4 %
    (profiles/r14/heads_softmax/), so the rule has no threshold and num_rows and
    num_e do not enter it.  One head takes "calls": there is nothing to share.
    MAXK_HEADS_SOFTMAX=heads|calls forces one."""
    forced = os.environ.get("MAXK_HEADS_SOFTMAX", "")
    if forced in ("heads", "calls"):
        return forced
    return "heads" if num_heads >= 2 else "calls"


def gat_attention_heads(indptr: torch.Tensor, indices: torch.Tensor, s_dst: torch.Tensor,
                        s_src: torch.Tensor, cbsr_val: torch.Tensor, cbsr_idx: torch.Tensor,
                        dim_origin: int, negative_slope: float = 0.2, chunk: int = 0,
                        out: Optional[torch.Tensor] = None, validate: Optional[bool] = None,
                        dropout: float = 0.0, seed: int = 0):
    """(out [H, num_rows, D], row_max [H, num_rows], row_sum [H, num_rows]): the attention
    aggregation of H GAT heads in one walk of the graph (maxk_gat_attention_heads) -- what
    gat_edge_softmax_heads followed by spgemm_forward_heads compute, without the coefficients
    [H, E] ever being stored.  row_max and row_sum are the softmax statistics of every row and
    head (the largest logit and the sum of exp(logit - max)); gat_edge_alpha_heads rebuilds the
    coefficients from them.  1 <= H <= MAX_HEADS; bitwise repeatable.
    dropout > 0: attention dropout at that rate under the mask of (seed, head, edge)
    (maxk_gat_attention_heads_dropout; edge_dropout_heads has the contract): out sums
    alpha * d * value, the statistics stay those of the undropped softmax."""
    D = int(dim_origin)
    H, num_rows, num_cols, E = _gat_heads_operands(indptr, indices, s_dst, s_src)
    _, cols2, k = _heads_operands(indptr, indices, cbsr_val, cbsr_idx, None, validate, D)
    if cols2 != num_cols:
        raise RuntimeError("s_src must be [H, num_cols] with num_cols = input_data.shape[0]")
    dev = cbsr_val.device
    out = _heads_out(out, (H, num_rows, D), dev, "[H, num_rows, dim_origin]")
    row_max = torch.empty(H, num_rows, dtype=torch.float32, device=dev)
    row_sum = torch.empty(H, num_rows, dtype=torch.float32, device=dev)
    shape = (num_rows, num_cols, E, D, k, H, chunk)
    args = (_ptr(indptr), _ptr(indices), _ptr(s_dst), _ptr(s_src), float(negative_slope),
            _ptr(cbsr_val), _ptr(cbsr_idx), _ptr(out), _ptr(row_max), _ptr(row_sum), *shape)
    if dropout > 0:
        _launch_ws(dev, "maxk_gat_attention_heads_dropout",
                   "maxk_gat_attention_heads_dropout_workspace_size", shape,
                   args + _dropout_args(dropout, seed))
    else:
        _dropout_args(dropout, seed)
        _launch_ws(dev, "maxk_gat_attention_heads", "maxk_gat_attention_heads_workspace_size",
                   shape, args)
    return out, row_max, row_sum


def _dropout_args(p, seed) -> Tuple[float, int]:
    """(p, seed) as the C ABI takes them: 0 <= p < 1, seed an unsigned 64-bit integer."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise RuntimeError(f"dropout must be in [0, 1), got {p}")
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise RuntimeError("seed must be in [0, 2^64)")
    return p, seed


def edge_dropout_heads(w: torch.Tensor, p: float, seed: int,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[H, E] = w[H, E] * d: attention dropout of head-major edge weights
    (maxk_edge_dropout_heads).  d[h, e] is 0 where word h & 3 of Philox4x32-10(counter
    (e, 0, h >> 2, 0), key seed) is below floor(p * 2^32), else float32(1 / (1 - p)): a pure
    function of (seed, h, e) that no kernel stores, so the same call on the gradient is this
    one's backward and the fused attention (gat_attention_heads(dropout=, seed=)) applies the
    same mask.  out may be w.  0 <= p < 1."""
    _need(w, "w", torch.float32)
    if w.dim() != 2 or not 1 <= w.shape[0] <= MAX_HEADS:
        raise RuntimeError(f"w must be [H, num_e] with 1 <= H <= {MAX_HEADS}")
    p, seed = _dropout_args(p, seed)
    dev = w.device
    out = _heads_out(out, tuple(w.shape), dev, "[H, num_e]")
    _launch(dev, "maxk_edge_dropout_heads", _ptr(w), _ptr(out), w.shape[0], w.shape[1], p, seed,
            _stream(dev))
    return out


def gat_edge_alpha_heads(indptr: torch.Tensor, indices: torch.Tensor, s_dst: torch.Tensor,
                         s_src: torch.Tensor, row_max: torch.Tensor, row_sum: torch.Tensor,
                         negative_slope: float = 0.2, out: Optional[torch.Tensor] = None,
                         validate: Optional[bool] = None) -> torch.Tensor:
    """w[H, E] float32: the attention coefficients from the scores and the row statistics of
    gat_attention_heads, exp(logit - row_max) / row_sum per edge (maxk_gat_edge_alpha_heads):
    one read of indices and one gather of a column's H scores per edge, no reductions.  Within
    gat_edge_softmax_heads's bound of its w."""
    H, num_rows, num_cols, E = _gat_heads_operands(indptr, indices, s_dst, s_src)
    _need(row_max, "row_max", torch.float32)
    _need(row_sum, "row_sum", torch.float32)
    if tuple(row_max.shape) != (H, num_rows) or tuple(row_sum.shape) != (H, num_rows):
        raise RuntimeError("row_max and row_sum must be [H, num_rows]")
    _validate_rows(validate, indptr, indices, num_cols, E)
    dev = s_src.device
    out = _heads_out(out, (H, E), dev, "[H, num_e]")
    shape = (H, num_rows, num_cols, E)
    _launch_ws(dev, "maxk_gat_edge_alpha_heads", "maxk_gat_edge_alpha_heads_workspace_size", shape,
               (_ptr(indptr), _ptr(indices), _ptr(s_dst), _ptr(s_src), float(negative_slope),
                _ptr(row_max), _ptr(row_sum), _ptr(out), *shape))
    return out


def _dot_operands(indptr, indices, q, cbsr_val, cbsr_idx, D, scale, validate):
    """The operand checks of the two dot-product attention calls; returns (H, num_rows, num_cols,
    k, scale as a float)."""
    _need(q, "q", torch.float32)
    if q.dim() != 3 or not 1 <= q.shape[0] <= MAX_HEADS or q.shape[2] != D:
        raise RuntimeError(f"q must be [H, num_rows, dim_origin] with 1 <= H <= {MAX_HEADS}")
    num_rows, num_cols, k = _heads_operands(indptr, indices, cbsr_val, cbsr_idx, None, validate, D)
    if q.shape[1] != num_rows:
        raise RuntimeError("q must be [H, num_rows, dim_origin]")
    scale = float(scale)
    if not (0.0 < scale < float("inf")):
        raise RuntimeError(f"scale must be finite and > 0, got {scale}")
    return q.shape[0], num_rows, num_cols, k, scale


def dot_attention_heads(indptr: torch.Tensor, indices: torch.Tensor, q: torch.Tensor,
                        cbsr_val: torch.Tensor, cbsr_idx: torch.Tensor, dim_origin: int,
                        scale: float, chunk: int = 0, validate: Optional[bool] = None,
                        out: Optional[torch.Tensor] = None, dropout: float = 0.0, seed: int = 0):
    """(out [H, num_rows, D], row_max [H, num_rows], row_sum [H, num_rows]): scaled dot-product
    attention of H heads on CBSR keys in one walk of the graph (maxk_dot_attention_heads).  The
    logit of edge (r <- c) is scale * sum_l cbsr_val[c, l] * q[h, r, cbsr_idx[c, l]], q
    [H, num_rows, D] the query of every destination mapped into the feature space; its softmax
    over the row weighs the CBSR rows summed into out -- what edge_weight_grad_heads(grad_output=q),
    the scale, H edge_softmax calls and spgemm_forward_heads compute, without logits or
    coefficients [H, E] ever being stored.  row_max and row_sum are the softmax statistics of
    every row and head; dot_edge_alpha_heads rebuilds the coefficients from them.
    1 <= H <= MAX_HEADS; scale finite and > 0; bitwise repeatable.
    dropout > 0: attention dropout at that rate under the mask of (seed, head, edge)
    (maxk_dot_attention_heads_dropout; edge_dropout_heads has the contract): out sums
    alpha * d * value, the statistics stay those of the undropped softmax."""
    D = int(dim_origin)
    H, num_rows, num_cols, k, scale = _dot_operands(indptr, indices, q, cbsr_val, cbsr_idx, D,
                                                    scale, validate)
    dev = cbsr_val.device
    out = _heads_out(out, (H, num_rows, D), dev, "[H, num_rows, dim_origin]")
    row_max = torch.empty(H, num_rows, dtype=torch.float32, device=dev)
    row_sum = torch.empty(H, num_rows, dtype=torch.float32, device=dev)
    shape = (num_rows, num_cols, indices.numel(), D, k, H, chunk)
    args = (_ptr(indptr), _ptr(indices), _ptr(q), scale, _ptr(cbsr_val), _ptr(cbsr_idx),
            _ptr(out), _ptr(row_max), _ptr(row_sum), *shape)
    if dropout > 0:
        _launch_ws(dev, "maxk_dot_attention_heads_dropout",
                   "maxk_dot_attention_heads_dropout_workspace_size", shape,
                   args + _dropout_args(dropout, seed))
    else:
        _dropout_args(dropout, seed)
        _launch_ws(dev, "maxk_dot_attention_heads", "maxk_dot_attention_heads_workspace_size",
                   shape, args)
    return out, row_max, row_sum


def dot_edge_alpha_heads(indptr: torch.Tensor, indices: torch.Tensor, q: torch.Tensor,
                         cbsr_val: torch.Tensor, cbsr_idx: torch.Tensor, dim_origin: int,
                         scale: float, row_max: torch.Tensor, row_sum: torch.Tensor,
                         chunk: int = 0, out: Optional[torch.Tensor] = None,
                         validate: Optional[bool] = None) -> torch.Tensor:
    """w[H, E] float32: the attention coefficients from the query, the CBSR and the row statistics
    of dot_attention_heads, exp(logit - row_max) / row_sum per edge (maxk_dot_edge_alpha_heads):
    one record gather per edge for all heads, no reductions over edges."""
    D = int(dim_origin)
    H, num_rows, num_cols, k, scale = _dot_operands(indptr, indices, q, cbsr_val, cbsr_idx, D,
                                                    scale, validate)
    _need(row_max, "row_max", torch.float32)
    _need(row_sum, "row_sum", torch.float32)
    if tuple(row_max.shape) != (H, num_rows) or tuple(row_sum.shape) != (H, num_rows):
        raise RuntimeError("row_max and row_sum must be [H, num_rows]")
    dev = cbsr_val.device
    E = indices.numel()
    out = _heads_out(out, (H, E), dev, "[H, num_e]")
    shape = (num_rows, num_cols, E, D, k, H, chunk)
    _launch_ws(dev, "maxk_dot_edge_alpha_heads", "maxk_dot_edge_alpha_heads_workspace_size", shape,
               (_ptr(indptr), _ptr(indices), _ptr(q), scale, _ptr(cbsr_val), _ptr(cbsr_idx),
                _ptr(row_max), _ptr(row_sum), _ptr(out), *shape))
    return out


def dot_attention_heads_backward(indptr: torch.Tensor, indices: torch.Tensor, q: torch.Tensor,
                                 cbsr_val: torch.Tensor, cbsr_idx: torch.Tensor,
                                 out: torch.Tensor, row_max: torch.Tensor, row_sum: torch.Tensor,
                                 grad_output: torch.Tensor, scale: float, chunk: int = 0,
                                 validate: Optional[bool] = None, plan=None,
                                 dropout: float = 0.0, seed: int = 0):
    """(grad_q [H, num_rows, D], grad_cbsr [num_cols, k]) of dot_attention_heads from its three
    results and the gradient of `out`, in one call (maxk_dot_attention_heads_backward): what
    dot_edge_alpha_heads, edge_weight_grad_heads, H edge_softmax_backward calls,
    spgemm_forward_heads and two sspmm_backward_heads calls compute, with no [H, E] tensor
    allocated.  The row sum of the softmax backward is taken as the dot product of out[h, r] and
    grad_output[h, r], so `out` must be the forward's.  Uses the graph's transpose plan (cached
    per `indices`, or `plan=` from transpose_plan()).  Bitwise repeatable; the same operand
    checks as dot_attention_heads.  dropout, seed: those of the forward that produced `out`
    (maxk_dot_attention_heads_dropout_backward); the row sum is still that dot product."""
    _need(grad_output, "grad_output", torch.float32)
    _need(out, "out", torch.float32)
    _need(q, "q", torch.float32)
    if q.dim() != 3:
        raise RuntimeError(f"q must be [H, num_rows, dim_origin] with 1 <= H <= {MAX_HEADS}")
    D = q.shape[2]
    H, num_rows, num_cols, k, scale = _dot_operands(indptr, indices, q, cbsr_val, cbsr_idx, D,
                                                    scale, validate)
    if tuple(grad_output.shape) != (H, num_rows, D) or tuple(out.shape) != (H, num_rows, D):
        raise RuntimeError("out and grad_output must be [H, num_rows, dim_origin]")
    _need(row_max, "row_max", torch.float32)
    _need(row_sum, "row_sum", torch.float32)
    if tuple(row_max.shape) != (H, num_rows) or tuple(row_sum.shape) != (H, num_rows):
        raise RuntimeError("row_max and row_sum must be [H, num_rows]")
    dev = cbsr_val.device
    col_ptr, csc_eid = plan if plan is not None else transpose_plan(indices, num_cols)
    grad_q = torch.empty(H, num_rows, D, dtype=torch.float32, device=dev)
    grad_cbsr = torch.empty(num_cols, k, dtype=torch.float32, device=dev)
    shape = (num_rows, num_cols, indices.numel(), D, k, H, chunk)
    args = (_ptr(indptr), _ptr(indices), _ptr(col_ptr), _ptr(csc_eid), _ptr(q), scale,
            _ptr(cbsr_val), _ptr(cbsr_idx), _ptr(out), _ptr(row_max), _ptr(row_sum),
            _ptr(grad_output), _ptr(grad_q), _ptr(grad_cbsr), *shape)
    if dropout > 0:
        _launch_ws(dev, "maxk_dot_attention_heads_dropout_backward",
                   "maxk_dot_attention_heads_dropout_backward_workspace_size", shape,
                   args + _dropout_args(dropout, seed))
    else:
        _dropout_args(dropout, seed)
        _launch_ws(dev, "maxk_dot_attention_heads_backward",
                   "maxk_dot_attention_heads_backward_workspace_size", shape, args)
    return grad_q, grad_cbsr


def spgemm_max_forward(indptr: torch.Tensor, indices: torch.Tensor, vals: torch.Tensor,
                       idx: torch.Tensor, dim: int, chunk: int = 0, want_arg: bool = True,
                       validate: Optional[bool] = None):
    """(out [num_rows, dim] float32, arg [num_rows, dim] int32 or None): the element-wise maximum
    over each row's neighbours of scatter(vals, idx) (maxk_spgemm_max_forward), and the CSR edge
    index of every winner, -1 where the implicit zero of a neighbour that does not keep the
    column wins or the row has no edges.  The first largest candidate in edge order wins, a NaN
    beats everything (torch's amax); include/maxk_hip.h has the rules.  out and arg are bitwise
    independent of `chunk`.  want_arg=False stores no winners (inference)."""
    D = int(dim)
    num_rows, num_cols, k = _heads_operands(indptr, indices, vals, idx, None, validate, D)
    dev = vals.device
    out = torch.empty(num_rows, D, dtype=torch.float32, device=dev)
    arg = torch.empty(num_rows, D, dtype=torch.int32, device=dev) if want_arg else None
    shape = (num_rows, num_cols, indices.numel(), D, k, int(chunk))
    _launch_ws(dev, "maxk_spgemm_max_forward", "maxk_spgemm_max_forward_workspace_size", shape,
               (_ptr(indptr), _ptr(indices), _ptr(vals), _ptr(idx), _ptr(out), _ptr(arg), *shape))
    return out, arg


def spgemm_max_backward(indptr: torch.Tensor, indices: torch.Tensor, idx: torch.Tensor,
                        arg: torch.Tensor, grad_out: torch.Tensor, k: int,
                        plan=None) -> torch.Tensor:
    """grad_vals [num_cols, k] of spgemm_max_forward from its `arg` and the gradient of `out`
    (maxk_spgemm_max_backward): slot (c, l) receives grad_out[r, idx[c, l]] of every edge
    (r <- c) that won its column, summed in CSC slot order; bitwise repeatable.  Uses the graph's
    transpose plan (cached per `indices`, or `plan=` from transpose_plan())."""
    for t, n, dt in ((indptr, "indptr", torch.int32), (indices, "indices", torch.int32),
                     (idx, "sparse_selector", torch.uint8), (arg, "arg", torch.int32),
                     (grad_out, "grad_out", torch.float32)):
        _need(t, n, dt)
    k = int(k)
    if idx.dim() != 2 or idx.shape[1] != k:
        raise RuntimeError("sparse_selector must be [num_cols, k]")
    num_cols = idx.shape[0]
    num_rows = indptr.numel() - 1
    if grad_out.dim() != 2 or grad_out.shape[0] != num_rows or arg.shape != grad_out.shape:
        raise RuntimeError("arg and grad_out must be [num_rows, dim_origin]")
    D = grad_out.shape[1]
    dev = grad_out.device
    col_ptr, csc_eid = plan if plan is not None else transpose_plan(indices, num_cols)
    grad_vals = torch.empty(num_cols, k, dtype=torch.float32, device=dev)
    shape = (num_rows, num_cols, indices.numel(), D, k)
    _launch_ws(dev, "maxk_spgemm_max_backward", "maxk_spgemm_max_backward_workspace_size", shape,
               (_ptr(indptr), _ptr(indices), _ptr(col_ptr), _ptr(csc_eid), _ptr(idx), _ptr(arg),
                _ptr(grad_out), _ptr(grad_vals), *shape))
    return grad_vals


def dot_attention_backward_route(num_heads: int, num_rows: int, num_e: int, k: int) -> str:
    """How the backward of the fused dot-product attention should run: "fused", one
    dot_attention_heads_backward call, or "rebuilt", dot_edge_alpha_heads and the stored path's
    passes (edge_weight_grad_heads, H edge_softmax_backward, spgemm_forward_heads, two
    sspmm_backward_heads).  Measured against exactly that sequence on the same inputs in the same
    run (profiles/r20/dot_attention_bwd/), fused / rebuilt at H = 1, 2, 4, 8:
    Reddit-sized k = 16 0.55, 0.56, 0.59, 0.80 and k = 32 0.58, 0.61, 0.66, 0.89; products-sized
    k = 16 0.59, 0.58, 0.58, 0.78 and k = 32 0.62, 0.63, 0.64, 0.86, against spreads of the
    rebuilt backward of 0.2 to 1.8 % -- a win past the spread at every point, smallest at eight
    heads, where the staged rows leave two waves per SIMD -- and MaxKTransformerConv's training
    step 0.71 to 0.94 of the step with the rebuilt backward.  So the rule has no threshold and
    num_rows, num_e and k do not enter it: "fused" for every head count.  What it costs is
    memory on a sparse graph: `out` [H, V, D] stays alive until this backward has run, and where
    D exceeds the average degree it is larger than the [H, E] transients it replaces -- the
    products-sized step peaks 2.7 to 17.0 GB above the step with the rebuilt backward (its
    `out`: 2.5 GB per head) and 4.9 to 31.2 GB above the stored path, while the Reddit-sized
    step peaks 0.3 to 1.2 GB below the rebuilt one from two heads on and below the stored path
    too: "rebuilt" remains the memory-saving option on sparse graphs.
    MAXK_DOT_ATTN_BWD=fused|rebuilt forces one.  Not wired into a default: MaxKTransformerConv's
    `attention_backward` defaults to "rebuilt"."""
    forced = os.environ.get("MAXK_DOT_ATTN_BWD", "")
    if forced in ("fused", "rebuilt"):
        return forced
    return "fused"


def heads_attention_route(num_heads: int, num_rows: int, num_e: int) -> Tuple[str, str]:
    """(forward under no_grad, training step): how a multi-head GAT layer's attention should run,
    "fused" (gat_attention_heads: no [H, E] tensor; the row statistics are saved and the
    coefficients rebuilt in the backward) or "stored" (gat_edge_softmax_heads, then the
    aggregation over the stored coefficients).  Measured against exactly what each replaces, in
    the same run (profiles/r15/gat_attention/), fused / stored at H = 1, 2, 4, 8:
    the forward on the Reddit-sized graph, k = 16 (dense: the stored forward is H single-head
    calls) 1.07, 0.90, 0.85, 0.98 against spreads below 1 %; on the products-sized graph,
    k = 32 (sparse: its records are random memory lines, and the fused walk keeps fewer waves
    resident) 1.16, 1.06, 1.13, 1.31; the layer's forward plus backward 1.02 to 1.13 on both,
    because the backward pays gat_edge_alpha_heads on top of the stored path's.  So: the
    forward is "fused" on a dense graph (average degree of at least HEADS_SPARSE_DEGREE, the
    regime of heads_forward_route) from two heads on, "stored" otherwise, and the training step
    is "stored" everywhere.  "fused" remains the memory-saving option: it never holds the
    4 * H * E bytes of the coefficients between forward and backward (3.6 GB of an 18.4 GB
    step at 8 heads, Reddit-sized).  MAXK_HEADS_ATTN=fused|stored forces both.
    MaxKMultiHeadGATConv's default does not follow this function: its `attention` argument
    defaults to "stored"."""
    forced = os.environ.get("MAXK_HEADS_ATTN", "")
    if forced in ("fused", "stored"):
        return forced, forced
    dense = num_e >= HEADS_SPARSE_DEGREE * num_rows
    return ("fused" if dense and num_heads >= 2 else "stored"), "stored"


def gat_attention_heads_backward(indptr: torch.Tensor, indices: torch.Tensor,
                                 s_dst: torch.Tensor, s_src: torch.Tensor,
                                 cbsr_val: torch.Tensor, cbsr_idx: torch.Tensor,
                                 out: torch.Tensor, row_max: torch.Tensor, row_sum: torch.Tensor,
                                 grad_output: torch.Tensor, negative_slope: float = 0.2,
                                 chunk: int = 0, validate: Optional[bool] = None, plan=None,
                                 dropout: float = 0.0, seed: int = 0):
    """(grad_s_dst [H, num_rows], grad_s_src [H, num_cols], grad_cbsr [num_cols, k]) of
    gat_attention_heads from its three results and the gradient of `out`, in one walk of the
    graph (maxk_gat_attention_heads_backward): what gat_edge_alpha_heads, edge_weight_grad_heads,
    gat_edge_softmax_heads_backward and sspmm_backward_heads compute in four, with no [H, E]
    tensor allocated.  The row sum of the softmax backward is taken as the dot product of
    out[h, r] and grad_output[h, r], so `out` must be the forward's.  Uses the graph's transpose
    plan (cached per `indices`, or `plan=` from transpose_plan()).  Bitwise repeatable; the same
    operand checks as gat_attention_heads.  dropout, seed: those of the forward that produced
    `out` (maxk_gat_attention_heads_dropout_backward); the row sum is still that dot product."""
    _need(grad_output, "grad_output", torch.float32)
    _need(out, "out", torch.float32)
    if grad_output.dim() != 3 or not 1 <= grad_output.shape[0] <= MAX_HEADS:
        raise RuntimeError(f"grad_output must be [H, num_rows, dim_origin] with 1 <= H <= "
                           f"{MAX_HEADS}")
    D = grad_output.shape[2]
    H, num_rows, num_cols, E = _gat_heads_operands(indptr, indices, s_dst, s_src)
    _, cols2, k = _heads_operands(indptr, indices, cbsr_val, cbsr_idx, None, validate, D)
    if cols2 != num_cols:
        raise RuntimeError("s_src must be [H, num_cols] with num_cols = input_data.shape[0]")
    if tuple(grad_output.shape) != (H, num_rows, D) or tuple(out.shape) != (H, num_rows, D):
        raise RuntimeError("out and grad_output must be [H, num_rows, dim_origin]")
    _need(row_max, "row_max", torch.float32)
    _need(row_sum, "row_sum", torch.float32)
    if tuple(row_max.shape) != (H, num_rows) or tuple(row_sum.shape) != (H, num_rows):
        raise RuntimeError("row_max and row_sum must be [H, num_rows]")
    dev = cbsr_val.device
    col_ptr, csc_eid = plan if plan is not None else transpose_plan(indices, num_cols)
    g_dst = torch.empty(H, num_rows, dtype=torch.float32, device=dev)
    g_src = torch.empty(H, num_cols, dtype=torch.float32, device=dev)
    g_cbsr = torch.empty(num_cols, k, dtype=torch.float32, device=dev)
    shape = (num_rows, num_cols, E, D, k, H, chunk)
    args = (_ptr(indptr), _ptr(indices), _ptr(col_ptr), _ptr(csc_eid), _ptr(s_dst), _ptr(s_src),
            float(negative_slope), _ptr(cbsr_val), _ptr(cbsr_idx), _ptr(out), _ptr(row_max),
            _ptr(row_sum), _ptr(grad_output), _ptr(g_dst), _ptr(g_src), _ptr(g_cbsr), *shape)
    if dropout > 0:
        _launch_ws(dev, "maxk_gat_attention_heads_dropout_backward",
                   "maxk_gat_attention_heads_dropout_backward_workspace_size", shape,
                   args + _dropout_args(dropout, seed))
    else:
        _dropout_args(dropout, seed)
        _launch_ws(dev, "maxk_gat_attention_heads_backward",
                   "maxk_gat_attention_heads_backward_workspace_size", shape, args)
    return g_dst, g_src, g_cbsr


def heads_attention_backward_route(num_heads: int, num_rows: int, num_e: int) -> str:
    """How the backward of a fused multi-head attention should run: "fused", one
    gat_attention_heads_backward call, or "rebuilt", gat_edge_alpha_heads and the stored path's
    three passes.  Measured against exactly those four calls in the same run
    (profiles/r16/gat_attention_bwd/), fused / rebuilt at H = 1, 2, 4, 8:
    Reddit-sized k = 16 0.88, 0.76, 0.66, 0.55; products-sized k = 32 0.96, 0.90, 0.80, 0.66,
    against spreads of the rebuilt backward of 0.8 to 3.1 % -- a win past the spread at every
    point, the one-head products-sized one by less than a point -- and the layer's training step
    0.78 to 0.99 of the step with the rebuilt backward.  So the rule has no threshold and
    num_rows and num_e do not enter it: "fused" for every head count.  What it costs is memory:
    `out` [H, V, D] stays alive until this backward has run and T [E, k] and gz [E, HP] are live
    together, so the step peaks above the rebuilt backward's (16.8 against 14.9 GB Reddit-sized
    and 67.4 against 48.7 GB products-sized at 8 heads; the stored path: 18.5 and 52.5 GB):
    "rebuilt" remains the memory-saving option.  MAXK_HEADS_ATTN_BWD=fused|rebuilt forces one.
    Not wired into a default: MaxKMultiHeadGATConv's `attention_backward` defaults to
    "rebuilt"."""
    forced = os.environ.get("MAXK_HEADS_ATTN_BWD", "")
    if forced in ("fused", "rebuilt"):
        return forced
    return "fused"


def records_ok(num_rows: int, num_cols: int, num_e: int, dim_origin: int, k: int) -> bool:
    """Whether the forward over transport records applies (maxk_records_ok)."""
    return bool(_lib().maxk_records_ok(int(num_rows), int(num_cols), int(num_e), int(dim_origin),
                                       int(k)))


def cbsr_records(cbsr_val: torch.Tensor, cbsr_idx: torch.Tensor, dim_origin: int,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Transport records [V, 5k] uint8 of a CBSR ([k f32 | k u8] per vertex; maxk_cbsr_records):
    what a shard owner all-gathers so the receivers' forward needs no record pack."""
    _need(cbsr_val, "cbsr_val", torch.float32)
    _need(cbsr_idx, "cbsr_idx", torch.uint8)
    if cbsr_val.dim() != 2 or cbsr_idx.shape != cbsr_val.shape:
        raise RuntimeError("cbsr_val / cbsr_idx must be the same [V, k] shape")
    V, k = cbsr_val.shape
    if out is None:
        out = torch.empty(V, 5 * k, dtype=torch.uint8, device=cbsr_val.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (V, 5 * k) or not out.is_contiguous():
        raise RuntimeError("out must be a contiguous uint8 [V, 5k] tensor")
    _launch(cbsr_val.device, "maxk_cbsr_records", _ptr(cbsr_val), _ptr(cbsr_idx), _ptr(out), V,
            int(dim_origin), k, _stream(cbsr_val.device))
    return out


def spgemm_forward_records(indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor,
                           rec: torch.Tensor, k: int, dim_origin: int,
                           row_div: Optional[torch.Tensor] = None, chunk: int = 0,
                           out: Optional[torch.Tensor] = None,
                           accumulate: bool = False,
                           validate: Optional[bool] = None) -> torch.Tensor:
    """spgemm_forward over transport records (cbsr_records of every column, e.g. all-gathered
    by a sharded forward): the same sums, no record pack.  The same input checks as
    spgemm_forward: dtypes, contiguity, shapes of out / row_div / values, and the
    graph's range check (once per graph by default, every call with validate=True)."""
    _need(indptr, "indptr", torch.int32)
    _need(indices, "indices", torch.int32)
    _need(values, "values", torch.float32)
    _need(rec, "rec", torch.uint8)
    k = int(k)
    if k <= 0 or rec.dim() != 2 or rec.shape[1] != 5 * k:
        raise RuntimeError("rec must be [num_cols, 5k]")
    # the selectors are the records' last k bytes: a strided view, read only by the selector
    # range check (validate=True); the graph check is what bounds the kernel's record reads
    out, shape = _forward_common(indptr, indices, values, rec.shape[0], k, rec[:, 4 * k:],
                                 int(dim_origin), row_div, chunk, out, accumulate, validate,
                                 rec.device)
    _launch_ws(rec.device, "maxk_spgemm_forward_records", "maxk_spgemm_forward_workspace_size",
               shape, (_ptr(indptr), _ptr(indices), _ptr(values), _ptr(rec), _ptr(row_div),
                       _ptr(out), *shape), (1 if accumulate else 0,))
    return out


_PLAN_CACHE = TensorCache()


def transpose_plan(indices: torch.Tensor, num_cols: int, cache: bool = True):
    """(col_ptr int32 [num_cols+1], csc_eid int32 [E]) of the CSR column indices: the CSC
    pointer and, per CSC slot, the CSR edge id it holds.  Built once per graph on the GPU
    (stable radix sort); cached per `indices` tensor object (and its version counter)."""
    _need(indices, "indices", torch.int32)

    def build():
        dev = indices.device
        E = indices.numel()
        col_ptr = torch.empty(num_cols + 1, dtype=torch.int32, device=dev)
        csc_eid = torch.empty(max(E, 1), dtype=torch.int32, device=dev)[:E]
        _launch_ws(dev, "maxk_transpose_plan", "maxk_transpose_plan_workspace_size",
                   (num_cols, E), (_ptr(indices), num_cols, E, _ptr(col_ptr), _ptr(csc_eid)))
        return col_ptr, csc_eid
    return _PLAN_CACHE.get((indices,), (int(num_cols),), build, cache)


_DENSE_CACHE = TensorCache()


def dense_plan(indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor, num_cols: int,
               cache: bool = True):
    """(col_ptr int32 [num_cols+1], t_src int32 [E], t_w float [E]) of the dense backward: the
    graph's transpose (transpose_plan) with, per CSC slot, the CSR row of its edge and its
    weight (maxk_dense_plan).  Cached per (indptr, indices, values) tensor objects and their
    version counters."""
    for t, n, dt in ((indptr, "indptr", torch.int32), (indices, "indices", torch.int32),
                     (values, "values", torch.float32)):
        _need(t, n, dt)

    def build():
        col_ptr, csc_eid = transpose_plan(indices, num_cols, cache=False)
        dev = indices.device
        E = indices.numel()
        t_src = torch.empty(max(E, 1), dtype=torch.int32, device=dev)[:E]
        t_w = torch.empty(max(E, 1), dtype=torch.float32, device=dev)[:E]
        _launch(dev, "maxk_dense_plan", _ptr(indptr), _ptr(values), _ptr(csc_eid),
                indptr.numel() - 1, E, _ptr(t_src), _ptr(t_w), _stream(dev))
        return col_ptr, t_src, t_w
    return _DENSE_CACHE.get((indptr, indices, values), (int(num_cols),), build, cache)


_BSORT_CACHE = TensorCache()


def bsort_plan(indptr: torch.Tensor, indices: torch.Tensor, num_cols: int, k: int,
               cache: bool = True):
    """(bucket_ptr int32 [nb+1], bucket_pos int32 [E], bucket_dst uint16 [E], win_src uint16
    [E], edge_row int32 [E], shift) of a CSR graph for the window-sorted backward at width k
    (maxk_bsort_plan): the bucket plan of maxk_bucket_shift(k) with each entry's T row in
    place of its edge id, per T row the edge (within its window of maxk_bsort_window(k) CSR
    edges) phase 1 stores there, and the source row of every edge.  Built once per graph and k on the GPU; cached per
    (indptr, indices) tensor objects (and their version counters)."""
    _need(indptr, "indptr", torch.int32)
    _need(indices, "indices", torch.int32)
    L = _lib()
    if int(L.maxk_bsort_window(int(k))) <= 0:
        raise RuntimeError(f"bsort_plan: k must be a multiple of 4 in [4, 256], got {k}")
    shift = int(L.maxk_bucket_shift(int(k)))

    def build():
        dev = indices.device
        E = indices.numel()
        nb = int(L.maxk_bucket_count(num_cols, shift))
        bptr = torch.empty(nb + 1, dtype=torch.int32, device=dev)
        bpos = torch.empty(max(E, 1), dtype=torch.int32, device=dev)[:E]
        bdst = torch.empty(max(E, 1), dtype=torch.uint16, device=dev)[:E]
        wsrc = torch.empty(max(E, 1), dtype=torch.uint16, device=dev)[:E]
        wrow = torch.empty(max(E, 1), dtype=torch.int32, device=dev)[:E]
        _launch_ws(dev, "maxk_bsort_plan", "maxk_bsort_plan_workspace_size", (num_cols, E),
                   (_ptr(indptr), _ptr(indices), indptr.numel() - 1, num_cols, E, int(k), shift,
                    _ptr(bptr), _ptr(bpos), _ptr(bdst), _ptr(wsrc), _ptr(wrow)))
        return bptr, bpos, bdst, wsrc, wrow, shift
    return _BSORT_CACHE.get((indptr, indices), (int(k), int(num_cols)), build, cache)


_PULL_CACHE = TensorCache()


def pull_plan(indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor, num_cols: int,
              k: int, dim: int = 256, slices: Optional[int] = None, cache: bool = True,
              shift: Optional[int] = None):
    """(tile_ptr int32 [S*nb+1], ent int32 [E, 2], shift, S) of a CSR graph and its edge
    values for the pull backward at width k: rows cut into S slices (default
    maxk_pull_slices: ~3.5 MiB of G rows per slice and rank part, at most 3 parts), columns into
    buckets of 2^shift; per tile
    (slice, bucket) the edges in CSR order, each {row in its slice | column in its bucket
    << 16, weight bits}.  Built on the GPU (one stable radix sort); cached per
    (indptr, indices, values) tensor objects and their version counters -- indptr assigns
    the edges to rows and slices, and the weights are copied into the plan, so a plan serves
    the graph and values it was built from.  `shift` overrides the bucket shift
    (maxk_pull_shift(k) by default; any shift the C ABI accepts for k)."""
    for t, n, dt in ((indptr, "indptr", torch.int32), (indices, "indices", torch.int32),
                     (values, "values", torch.float32)):
        _need(t, n, dt)
    L = _lib()
    num_rows = indptr.numel() - 1
    shift = int(L.maxk_pull_shift(int(k))) if shift is None else int(shift)
    if shift < 0:
        raise RuntimeError(f"pull_plan: invalid k {k}")
    # by default sized by the CU count of the device that holds the graph
    S = int(slices) if slices else _sized(indices.device, "maxk_pull_slices", num_rows,
                                          int(num_cols), int(dim), int(k))

    def build():
        dev = indices.device
        E = indices.numel()
        nb = int(L.maxk_bucket_count(num_cols, shift))
        tptr = torch.empty(S * nb + 1, dtype=torch.int32, device=dev)
        ent = torch.empty(max(E, 1), 2, dtype=torch.int32, device=dev)[:E]
        _launch_ws(dev, "maxk_pull_plan", "maxk_pull_plan_workspace_size",
                   (num_rows, num_cols, E, shift, S),
                   (_ptr(indptr), _ptr(indices), _ptr(values), num_rows, num_cols, E, shift, S,
                    _ptr(tptr), _ptr(ent)))
        return tptr, ent, shift, S
    return _PULL_CACHE.get((indptr, indices, values), (shift, S, int(num_cols)), build, cache)


_STREAM_CACHE = TensorCache()


class PullStreamPlan(NamedTuple):
    """Plan of the stream pull backward (pull_stream_plan); opaque to callers, who pass it back
    as `plan=`."""
    bucket_col: torch.Tensor  # int32 [n_buckets + 1]
    grp_ptr: torch.Tensor     # int32 [n_buckets + 1]
    ent: torch.Tensor         # int32 [E, 2]
    shift: int                # column bits of an entry: maxk_pull_shift(k)
    n_buckets: int
    slices: int


def _stream_on() -> bool:
    """MAXK_PULL_STREAM=0 keeps the tiled pull everywhere (the same build, both ways)."""
    return os.environ.get("MAXK_PULL_STREAM", "1") != "0"


def pull_stream_buckets(dev, num_rows: int, num_cols: int, num_e: int, dim: int, k: int) -> int:
    """Buckets of the stream pull backward for this shape on `dev` (maxk_pull_stream_buckets
    with that device's CU count), or 0 where the tiled pull stays: see include/maxk_hip.h."""
    if not _stream_on():
        return 0
    return _sized(dev, "maxk_pull_stream_buckets", int(num_rows), int(num_cols), int(num_e),
                  int(dim), int(k), 0)


def pull_stream_plan(indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor,
                     num_cols: int, k: int, dim: int = 256, groups: Optional[int] = None,
                     slices: Optional[int] = None, cache: bool = True) -> PullStreamPlan:
    """The stream pull backward's plan of a CSR graph and its edge values at width k
    (maxk_pull_stream_plan): `groups` buckets of at most 2^maxk_pull_shift(k) columns holding
    about equal edge counts (default pull_stream_buckets: whole rounds of one workgroup per CU
    and part; an error where that rule refuses the shape), each bucket's edges ordered by
    (one of `slices` row slices, CSR order) as {row << shift | column in the bucket, weight
    bits}.  `slices` (default maxk_pull_stream_slices: 1) only widens the sort key: a bucket's
    entries are in CSR order whatever it is.  Built on the GPU, cached like pull_plan."""
    for t, n, dt in ((indptr, "indptr", torch.int32), (indices, "indices", torch.int32),
                     (values, "values", torch.float32)):
        _need(t, n, dt)
    L = _lib()
    dev = indices.device
    num_rows, E = indptr.numel() - 1, indices.numel()
    shift = int(L.maxk_pull_shift(int(k)))
    if k % 4 or shift < 4:
        raise RuntimeError(f"pull_stream_plan needs k % 4 == 0, got k={k}")
    nb = int(groups) if groups else pull_stream_buckets(dev, num_rows, num_cols, E, dim, k)
    if nb <= 0:
        raise RuntimeError(f"pull_stream_plan: the stream path does not apply to {num_rows} x "
                           f"{num_cols}, dim={dim}, k={k}; pass groups= or use pull_plan")
    S = int(slices) if slices else int(L.maxk_pull_stream_slices(num_rows, int(num_cols),
                                                                 int(dim), int(k)))

    def build():
        bcol = torch.empty(nb + 1, dtype=torch.int32, device=dev)
        gptr = torch.empty(nb + 1, dtype=torch.int32, device=dev)
        ent = torch.empty(max(E, 1), 2, dtype=torch.int32, device=dev)[:E]
        _launch_ws(dev, "maxk_pull_stream_plan", "maxk_pull_stream_plan_workspace_size",
                   (max(int(num_cols), 1), max(E, 1), nb, S),
                   (_ptr(indptr), _ptr(indices), _ptr(values), num_rows, int(num_cols), E, int(k),
                    nb, S, _ptr(bcol), _ptr(gptr), _ptr(ent)))
        return PullStreamPlan(bcol, gptr, ent, shift, nb, S)
    return _STREAM_CACHE.get((indptr, indices, values), (int(k), nb, S, int(num_cols)), build,
                             cache)


def _scaled_stream_entries(plan: PullStreamPlan, num_rows: int, k: int,
                           row_div: torch.Tensor) -> Optional[torch.Tensor]:
    """_scaled_entries for a stream plan (maxk_pull_stream_entries_scale): the row is in the
    entry, so one pass over the entries."""
    ent = plan.ent
    sc = _SCALED.lookup((ent, row_div), ())
    if sc is not None:
        return sc
    if ent.is_cuda and torch.cuda.is_current_stream_capturing():
        return None  # as _scaled_entries: nothing is built inside a capture

    def build():
        sc = torch.empty_like(ent)
        _launch(ent.device, "maxk_pull_stream_entries_scale", _ptr(ent), ent.shape[0], num_rows,
                int(k), _ptr(row_div), _ptr(sc), _stream(ent.device))
        return sc
    return _SCALED.get((ent, row_div), (), build)


_HYBRID_CACHE = TensorCache()
MAXK_PULL_NO_REDUCE, MAXK_PULL_REDUCE_ONLY = 2, 4  # include/maxk_hip.h
MAXK_HYBRID_PRESCALED = 1
# maxk_backward_mode_auto's codes (include/maxk_hip.h MAXK_BWD_*)
_MODE_OF_CODE = {0: "pull", 1: "csc", 3: "hybrid", 4: "atomic", 5: "bsort", 6: "dense"}
_SIDE: dict = {}


def _side_stream(dev: torch.device) -> "torch.cuda.Stream":
    """One extra HIP stream per device (the hybrid backward's tile kernels)."""
    i = dev.index if dev.index is not None else torch.cuda.current_device()
    if i not in _SIDE:
        _SIDE[i] = torch.cuda.Stream(device=i)
    return _SIDE[i]
# a tile pulls when it holds at least this many entries per row of its slice
HYBRID_DENSITY = 0.5  # MAXK_HYBRID_DENSITY in include/maxk_hip.h
# mode "auto" picks "hybrid" on a sparse graph whose pull_locality reaches this (products-
# sized, k=32: 1.02 (random labels) csc 8.2 vs hybrid 8.4 ms; 1.9: 8.1 vs 6.4; 6.9: 7.4 vs 4.7)
HYBRID_LOCALITY = 1.5  # MAXK_HYBRID_LOCALITY


def hybrid_plan(indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor,
                num_cols: int, k: int, dim: int = 256, density: Optional[float] = None,
                cache: bool = True):
    """Plan of the "hybrid" backward (maxk_hybrid_plan, C ABI): the pull over the dense tiles
    of the graph's pull plan (at least `density` entries per row of the tile's slice), the
    two-phase csc over the other edges.  A community-ordered graph keeps most edges in the
    tiles near the diagonal, which pull well, while a pull over every tile would write one
    [num_cols, k] partial per row slice.  Returns (tile_list, tile_ent, bucket_ptr,
    bucket_tiles, ent, shift, S, (off_indptr, off_indices, off_values, off_transpose_plan));
    cached like pull_plan.  k % 4 == 0.  `density` defaults to MAXK_HYBRID_DENSITY or
    HYBRID_DENSITY."""
    if density is None:
        density = float(os.environ.get("MAXK_HYBRID_DENSITY", HYBRID_DENSITY))
    if k % 4:
        raise RuntimeError(f"hybrid backward needs k % 4 == 0, got k={k}")

    def build():
        tptr, ent, shift, S = pull_plan(indptr, indices, values, num_cols, k, dim, cache=False)
        dev = indices.device
        num_rows = indptr.numel() - 1
        E = indices.numel()
        nb = int(_lib().maxk_bucket_count(num_cols, shift))
        nt = S * nb
        i32 = dict(dtype=torch.int32, device=dev)
        tile_list = torch.empty(max(nt, 1), **i32)
        tile_ent = torch.empty(nt + 1, **i32)
        bucket_ptr = torch.empty(nb + 1, **i32)
        bucket_tiles = torch.empty(max(nt, 1), **i32)
        ent_d = torch.empty(max(E, 1), 2, **i32)
        off_ip = torch.empty(num_rows + 1, **i32)
        off_ix = torch.empty(max(E, 1), **i32)
        off_val = torch.empty(max(E, 1), dtype=torch.float32, device=dev)
        counts = (ctypes.c_int64 * 3)()
        _launch_ws(dev, "maxk_hybrid_plan", "maxk_hybrid_plan_workspace_size",
                   (num_rows, num_cols, E, shift, S),
                   (_ptr(indptr), _ptr(indices), _ptr(values), _ptr(tptr), _ptr(ent), num_rows,
                    num_cols, E, shift, S, float(density), _ptr(tile_list), _ptr(tile_ent),
                    _ptr(bucket_ptr), _ptr(bucket_tiles), _ptr(ent_d), _ptr(off_ip), _ptr(off_ix),
                    _ptr(off_val), counts))
        n_t, n_p, n_o = (int(c) for c in counts)
        del tptr, ent
        # the slices are views of their worst-case buffers; copies keep the plan compact
        tile_list, bucket_tiles = tile_list[:n_t].clone(), bucket_tiles[:n_t].clone()
        tile_ent = tile_ent[:n_t + 1].clone()
        ent_d = ent_d[:n_p].clone()
        off_ix, off_val = off_ix[:n_o].clone(), off_val[:n_o].clone()
        off = (off_ip, off_ix, off_val, transpose_plan(off_ix, num_cols, cache=False))
        return tile_list, tile_ent, bucket_ptr, bucket_tiles, ent_d, shift, S, off
    return _HYBRID_CACHE.get((indptr, indices, values),
                             (int(k), int(dim), float(density), int(num_cols)), build, cache)


BWD_MODES = ("auto", "pull", "csc", "atomic", "hybrid", "bsort", "dense")
BSORT_KMAX = 8  # MAXK_BSORT_KMAX: the auto rule's bsort limit
_BSORT_WARNED: set = set()  # (id(indptr), k) already warned about


_LOCALITY = TensorCache()
_SCALED = TensorCache()


def _scaled_entries(ent: torch.Tensor, tiles: Optional[torch.Tensor], tile_ent: torch.Tensor,
                    num_rows: int, num_cols: int, shift: int, S: int,
                    row_div: torch.Tensor) -> Optional[torch.Tensor]:
    """The pull entries with each weight divided by its source row's row_div
    (maxk_pull_entries_scale), so the tile kernels gather G itself instead of a G / row_div
    copy (gprime_kernel: a read and a write of all of G per call; ogbn-products 2 x 2.5 GB).
    `tiles[i]` (None: i) is the tile of the entries' i-th run [tile_ent[i], tile_ent[i+1]).
    Cached per entry tensor for one (row_div object, version): the degrees a layer divides by
    are the same tensor every call (maxk_layers.CSRGraph).  None when it would have to be built
    inside a stream capture."""
    sc = _SCALED.lookup((ent, row_div), ())
    if sc is not None:
        return sc
    if ent.is_cuda and torch.cuda.is_current_stream_capturing():
        # a hipGraph capture records kernels without running them: a copy built here would
        # be cached before it holds anything, so the caller keeps the G / row_div route
        return None

    def build():
        sc = torch.empty_like(ent)
        _launch(ent.device, "maxk_pull_entries_scale", _ptr(ent), _ptr(tiles), _ptr(tile_ent),
                tile_ent.numel() - 1, num_rows, num_cols, shift, S, _ptr(row_div), _ptr(sc),
                _stream(ent.device))
        return sc
    return _SCALED.get((ent, row_div), (), build)


def _prescale() -> bool:
    """MAXK_PULL_PRESCALE=0 keeps the per-call G / row_div copy instead of scaled entries."""
    return os.environ.get("MAXK_PULL_PRESCALE", "1") != "0"


def pull_locality(indptr: torch.Tensor, indices: torch.Tensor, shift: int) -> float:
    """Edges per occupied (source row, bucket of 2^shift columns) pair (maxk_pull_locality):
    how many entries of a pull tile share a source row's G lines.  A randomly labelled graph
    with `a` edges per (row, bucket) on average has a / (1 - e^-a) (ogbn-products-sized:
    ~1.0); a graph whose vertex order groups its communities (maxk_graph.locality_order) has
    many more, whatever the average.  One pass over the edges (columns sorted within rows,
    else an under-estimate), cached per (indptr, indices, shift) and their versions.  Reported
    by bench.py (extra.pull_locality); on sparse graphs it steers mode "auto" to "hybrid"."""
    def build():
        _need(indptr, "indptr", torch.int32)
        _need(indices, "indices", torch.int32)
        dev = indices.device
        out = ctypes.c_double(0.0)
        ws = torch.empty(8, dtype=torch.uint8, device=dev)
        _launch(dev, "maxk_pull_locality", _ptr(indptr), _ptr(indices), indptr.numel() - 1,
                indices.numel(), int(shift), ctypes.byref(out), _ptr(ws), ws.numel(),
                _stream(dev))
        return float(out.value)
    return _LOCALITY.get((indptr, indices), (int(shift),), build)


def _bwd_mode(mode: Optional[str], k: int = 4, num_e: int = 0, num_cols: int = 0,
              num_rows: Optional[int] = None, dim: Optional[int] = None,
              graph: Optional[tuple] = None) -> str:
    """Resolve the backward mode.  "auto" (default; MAXK_BWD_MODE overrides) is the C ABI's
    rule, maxk_backward_mode_auto: "dense" at k >= dim / 2 (dim % 4 == 0, dim <= 128, k % 4 ==
    0: Flickr-shaped D = 64 at k = 32 / 64, where a CBSR row is as wide as the dense row);
    else "pull" where it measured faster than "csc" -- k % 4 == 0
    or k <= 64, dim % 4 == 0 when dim is given, and at least ~1/2 edge per (source row,
    bucket of 2^maxk_bucket_shift(k) columns) on average (Reddit k=16: 2.2, k=64: 0.54;
    ogbn-proteins k=64: 1.2; ogbn-products: 0.02), or a gradient G of at most 64 MiB (Flickr:
    23 MB, 0.05 vs 0.13 ms), which stays cache-resident however sparse the graph (at most
    256 x 65536 rows; past that the rules below apply).  On a sparse graph the whole pull loses
    even with locality (its per-slice partials, [num_cols, k] per row slice: a community-
    ordered ogbn-products-sized graph 46 ms against 8 ms csc), but where
    `graph` = (indptr, indices) is given and its pull_locality reaches HYBRID_LOCALITY (k % 4
    == 0, dim % 4 == 0) "hybrid" pulls the dense tiles and runs csc over the rest (that graph:
    4.7 against 7.4 ms); otherwise "bsort" at k % 4 == 0, k <= 8 when a window of
    maxk_bsort_window(k) edges holds >= 2 rows per destination bucket on average (ogbn-
    products k = 8: 2.9 against 3.9 ms for csc, both with the selector stream), else "csc".
    "pull", "bsort" and "hybrid" sum in fp64 LDS accumulators: two runs
    agree except in rare fp32 rounding ties; MAXK_BWD_MODE=csc forces the bitwise-
    deterministic form everywhere."""
    mode = mode or os.environ.get("MAXK_BWD_MODE", "auto")
    if mode not in BWD_MODES:
        raise RuntimeError(f"backward mode must be one of {BWD_MODES}, got {mode!r}")
    if mode == "auto":
        L = _lib()
        rows = num_rows if num_rows else num_cols
        D = -1 if dim is None else int(dim)
        code = int(L.maxk_backward_mode_auto(rows, num_cols, num_e, D, int(k), -1.0))
        if (code in (1, 5) and graph is not None and k % 4 == 0 and num_e > 0
                and rows <= 256 * 65536):  # csc / bsort unless the locality asks for hybrid
            loc = pull_locality(graph[0], graph[1], int(L.maxk_pull_shift(int(k))))
            code = int(L.maxk_backward_mode_auto(rows, num_cols, num_e, D, int(k), loc))
        mode = _MODE_OF_CODE[code]
    for ok, message in _MODE_NEEDS.get(mode, ()):
        if not ok(k, dim):
            raise RuntimeError(message.format(k=k, dim=dim))
    return mode


def _k4_dim4(k, dim):
    return k % 4 == 0 and (dim is None or dim % 4 == 0)


# mode -> ((what (k, dim) must satisfy, the error otherwise), ...); dim None: not known here
_MODE_NEEDS = {
    "bsort": ((lambda k, dim: k % 4 == 0, "backward mode 'bsort' needs k % 4 == 0, got k={k}"),),
    "pull": ((lambda k, dim: k % 4 == 0 or k <= 64,
              "backward mode 'pull' needs k % 4 == 0 or k <= 64, got k={k}"),
             (lambda k, dim: dim is None or dim % 4 == 0,
              "backward mode 'pull' needs dim_origin % 4 == 0, got {dim}")),
    "dense": ((_k4_dim4, "backward mode 'dense' needs k % 4 == 0 and dim_origin % 4 == 0, "
                         "got k={k}, dim={dim}"),),
    "hybrid": ((_k4_dim4, "backward mode 'hybrid' needs k % 4 == 0 and dim_origin % 4 == 0, "
                          "got k={k}, dim={dim}"),),
}


def graph_only_mode(k: int, num_e: int, num_cols: int) -> Optional[str]:
    """The feature backward's mode for differentiable edge weights, or None when a mode is
    forced (MAXK_BWD_MODE set to anything but "auto").  The pull, dense and hybrid plans embed
    the edge weights (pull_plan, dense_plan and hybrid_plan are keyed on `values`), so a weight
    tensor that changes every step -- a Parameter updated in place, or attention coefficients,
    a fresh tensor per call -- would rebuild such a plan on every call (Reddit-sized: the plan
    build costs several forwards, profiles/r07/edge_grad/).  The choice is therefore among the
    modes whose plans depend on the graph alone: "bsort" where maxk_backward_mode_auto's rule
    for it holds (k % 4 == 0, k <= BSORT_KMAX, a window of maxk_bsort_window(k) edges holding
    >= 2 rows per destination bucket), else "csc"."""
    if os.environ.get("MAXK_BWD_MODE", "auto") != "auto":
        return None
    L = _lib()
    k = int(k)
    if (k > 0 and k % 4 == 0 and k <= BSORT_KMAX and num_e > 0 and
            int(L.maxk_bsort_window(k)) * (1 << int(L.maxk_bucket_shift(k))) >= 2 * num_cols):
        return "bsort"
    return "csc"


def backward_plan(indices: torch.Tensor, num_cols: int, k: int, mode: Optional[str] = None,
                  num_rows: Optional[int] = None, indptr: Optional[torch.Tensor] = None,
                  values: Optional[torch.Tensor] = None, dim: Optional[int] = None):
    """The per-graph plan sspmm_backward needs for `mode` at width k (None for "atomic");
    num_rows (default num_cols) and dim only steer mode "auto".  Mode "pull" also needs
    the graph's indptr and edge values."""
    mode = _bwd_mode(mode, k, indices.numel(), num_cols, num_rows, dim,
                     None if indptr is None else (indptr, indices))
    if mode in ("pull", "hybrid"):
        if indptr is None or values is None:
            raise RuntimeError(f"backward_plan: mode '{mode}' needs indptr= and values=")
        if mode == "hybrid":
            return hybrid_plan(indptr, indices, values, num_cols, k, dim or 256)
        return _pull_plan_for(indptr, indices, values, num_cols, k, dim or 256)
    if mode == "dense":
        if indptr is None or values is None:
            raise RuntimeError("backward_plan: mode 'dense' needs indptr= and values=")
        return dense_plan(indptr, indices, values, num_cols)
    if mode == "bsort":
        if indptr is None:
            raise RuntimeError("backward_plan: mode 'bsort' needs indptr=")
        return bsort_plan(indptr, indices, num_cols, k)
    if mode == "csc":
        return transpose_plan(indices, num_cols)
    return None


def sspmm_backward(indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor,
                   grad_output: torch.Tensor, cbsr_idx: torch.Tensor,
                   row_div: Optional[torch.Tensor] = None, chunk: int = 0,
                   out: Optional[torch.Tensor] = None, validate: Optional[bool] = None,
                   mode: Optional[str] = None, plan=None,
                   edge_sel: Optional[torch.Tensor] = None) -> torch.Tensor:
    """grad_cbsr[num_cols, k] = (A^T diag(1/row_div) G)[c, cbsr_idx[c, l]].

    edge_sel (uint8 [E, k], k % 4 == 0; modes "csc" and "bsort", ignored by the others): the
    selectors per edge (edge_selectors(), or the forward's by-product), read in CSR order
    instead of gathered.

    mode "auto" (default; MAXK_BWD_MODE overrides): "dense", "pull", "hybrid", "bsort" or
    "csc", see _bwd_mode.  The autograd surface (maxk_spgemm_function) does not leave the choice
    to "auto" when the edge weights require grad: it passes graph_only_mode()'s "bsort" or
    "csc", whose plans depend on the graph alone, since the pull, dense and hybrid plans embed
    the weights and would be rebuilt whenever they change.
    mode "pull": per tile (row slice, destination bucket), the k values of every edge
    gathered from G and summed in fp64 LDS accumulators, no contribution rows (with a
    row_div the plan's weights are pre-divided, once per divisor: _scaled_entries);
    uses the graph's pull plan (built once per (indptr, indices, values) and cached, or
    `plan=` from pull_plan()); fp64 tile sums, so two runs agree except in rare rounding
    ties (use "csc" for bitwise repeatability).  Where pull_stream_buckets accepts the shape
    (k % 4 == 0, buckets that fill whole rounds of one workgroup per CU without narrowing
    them by more than 12.5 %; MAXK_PULL_STREAM=0 turns it off) the stream path runs instead:
    one workgroup per (bucket, part) walks all of the bucket's entries and stores its rows
    itself, no tile partials and no reduce (pull_stream_plan(), or that plan as `plan=`).
    mode "csc": two-phase, atomic-free and bitwise deterministic, using the graph's
    transpose plan (built once and cached, or `plan=` from transpose_plan()).
    mode "bsort" (k % 4 == 0): two-phase, phase 1 writing each window of maxk_bsort_window(k)
    CSR edges' rows ordered by destination bucket (staged in LDS), phase 2 summing each
    bucket's rows of a window as one run in fp64 LDS accumulators -- for large sparse graphs
    at small k, where a csc phase 2 pays a whole random line per 32-B row (bsort_plan()).
    mode "atomic": one global fp32 atomic per (edge, l); no preprocessing.
    mode "dense" (k % 4 == 0, dim % 4 == 0; "auto" picks it at k >= dim / 2, dim <= 128,
    maxk_dense_route): Y = A^T diag(1/row_div) G over dense G rows along the graph's transpose
    with source rows (dense_plan), then the k selected columns of each row of Y; bitwise
    repeatable.
    mode "hybrid" (k % 4 == 0; "auto" picks it on sparse graphs with locality): the pull
    over the dense tiles of the pull plan, on a second stream, beside csc over the other
    edges (hybrid_plan), for large graphs whose vertex order groups their communities."""
    for t, n, dt in ((indptr, "indptr", torch.int32), (indices, "indices", torch.int32),
                     (values, "values", torch.float32), (grad_output, "grad_output", torch.float32),
                     (cbsr_idx, "sparse_selector", torch.uint8)):
        _need(t, n, dt)
    num_rows = indptr.numel() - 1
    if grad_output.dim() != 2 or grad_output.shape[0] != num_rows:
        raise RuntimeError("grad_output must be [num_rows, dim_origin]")
    D = grad_output.shape[1]
    num_cols, k = cbsr_idx.shape
    if row_div is not None:
        _need(row_div, "row_div", torch.float32)
        if row_div.numel() != num_rows:
            raise RuntimeError("row_div must have num_rows entries")
    _validate_call(validate, indptr, indices, num_cols, cbsr_idx, D)
    dev = grad_output.device
    if out is None:
        out = torch.empty(num_cols, k, dtype=torch.float32, device=dev)
    else:
        _need(out, "out", torch.float32)
        if tuple(out.shape) != (num_cols, k):
            raise RuntimeError("out must be [num_cols, k]")
    E = indices.numel()
    asked = mode or os.environ.get("MAXK_BWD_MODE", "auto")
    mode = _bwd_mode(mode, k, E, num_cols, num_rows, D, (indptr, indices))
    if mode == "dense" and asked == "auto" and not (
            grad_output.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
            and cbsr_idx.data_ptr() % 4 == 0):
        mode, plan = "pull", None  # the dense kernels' vector loads need aligned rows
    if edge_sel is not None and mode in ("csc", "bsort"):
        _need(edge_sel, "edge_sel", torch.uint8)
        if tuple(edge_sel.shape) != (E, k):
            raise RuntimeError("edge_sel must be [num_e, k]")
    _BWD[mode](indptr, indices, values, grad_output, row_div, cbsr_idx, edge_sel, out,
               (num_rows, num_cols, E, D, k), chunk, plan)
    return out


# One function per backward mode, all called as _BWD[mode](indptr, indices, values, G, row_div,
# sel, edge_sel, out, shape, chunk, plan) with shape = (num_rows, num_cols, E, D, k) and every
# operand checked by sspmm_backward; `plan` None: the graph's cached plan.
def _bwd_dense(indptr, indices, values, G, row_div, sel, edge_sel, out, shape, chunk, plan):
    col_ptr, t_src, t_w = (plan if plan is not None
                           else dense_plan(indptr, indices, values, shape[1]))
    _launch_ws(G.device, "maxk_sspmm_backward_dense", "maxk_sspmm_backward_dense_workspace_size",
               (*shape, chunk),
               (_ptr(col_ptr), _ptr(t_src), _ptr(t_w), _ptr(G), _ptr(row_div), _ptr(sel),
                _ptr(out), *shape, chunk))


def _bwd_hybrid(indptr, indices, values, G, row_div, sel, edge_sel, out, shape, chunk, plan):
    num_rows, num_cols, _, D, k = shape
    tl, te, bp, bt, ent, shift, S, off = (plan if plan is not None else
                                         hybrid_plan(indptr, indices, values, num_cols, k, D))
    oip, oix, oval, (ocp, oeid) = off
    n_t, n_off = tl.numel(), oix.numel()
    flags = 0
    if row_div is not None and n_t > 0 and _prescale():
        sc = _scaled_entries(ent, tl, te, num_rows, num_cols, shift, S, row_div)
        if sc is not None:
            ent, flags = sc, MAXK_HYBRID_PRESCALED
    dev = G.device
    size = "maxk_sspmm_backward_hybrid_workspace_size", (num_rows, num_cols, n_off, D, k, n_t)
    if not (n_off > 0 and n_t > 0 and os.environ.get("MAXK_HYBRID_STREAMS", "1") != "0"):
        # everything on the caller's stream, in one C-ABI call
        _launch_ws(dev, "maxk_sspmm_backward_hybrid", *size,
                   (_ptr(G), _ptr(row_div), _ptr(sel), _ptr(tl), _ptr(te), n_t, _ptr(bp), _ptr(bt),
                    _ptr(ent), ent.shape[0], shift, S, _ptr(oip), _ptr(oix), _ptr(oval), n_off,
                    _ptr(ocp), _ptr(oeid), flags, _ptr(out), num_rows, num_cols, D, k),
                   (None, None, None))
        return
    # the same sequence with the tile kernels on a side stream beside the csc, forked
    # and joined by torch (fresh events each call: one pair re-recorded by eager calls
    # broke the join of a graph captured with it, test_hipgraph_capture_*[hybrid])
    with _on(dev):
        ws = _workspace(dev, size[0], *size[1])
        a = _sized(dev, "maxk_sspmm_backward_csc_workspace_size", num_rows, num_cols, n_off, D,
                   k, 0)
        a = (a + 255) // 256 * 256
        ws_csc, ws_pull = ws[:a], ws[a:]
        tile_div = None if flags & MAXK_HYBRID_PRESCALED else row_div

        def tiles(acc, stream):
            _launch(dev, "maxk_sspmm_backward_pull_tiles", _ptr(G), _ptr(tile_div), _ptr(sel),
                    _ptr(tl), _ptr(te), n_t, _ptr(bp), _ptr(bt), _ptr(ent), shift, S, acc,
                    _ptr(out), num_rows, num_cols, ent.shape[0], D, k, _ptr(ws_pull),
                    ws_pull.numel(), stream)
        main = torch.cuda.current_stream(dev)
        side = _side_stream(dev)
        side.wait_stream(main)
        tiles(MAXK_PULL_NO_REDUCE, ctypes.c_void_p(side.cuda_stream))
        _launch(dev, "maxk_sspmm_backward_csc", _ptr(oip), _ptr(oix), _ptr(oval), _ptr(G),
                _ptr(row_div), _ptr(sel), _ptr(ocp), _ptr(oeid), _ptr(out), num_rows, num_cols,
                n_off, D, k, 0, _ptr(ws_csc), ws_csc.numel(), _stream(dev))
        main.wait_stream(side)
        tiles(MAXK_PULL_REDUCE_ONLY | 1, _stream(dev))
    # the side stream is joined to the caller's stream before the call returns, so what
    # it read (ws included) is free for reuse in that stream's order


def _pull_plan_for(indptr, indices, values, num_cols, k, dim):
    """The plan mode "pull" uses for a graph: the stream plan where pull_stream_buckets accepts
    the shape on the graph's device, else the tiled pull_plan."""
    num_rows, E = indptr.numel() - 1, indices.numel()
    if k % 4 == 0 and pull_stream_buckets(indices.device, num_rows, num_cols, E, dim, k) > 0:
        return pull_stream_plan(indptr, indices, values, num_cols, k, dim)
    return pull_plan(indptr, indices, values, num_cols, k, dim)


def _bwd_pull(indptr, indices, values, G, row_div, sel, edge_sel, out, shape, chunk, plan):
    num_rows, num_cols, E, D, k = shape
    if plan is None:
        plan = _pull_plan_for(indptr, indices, values, num_cols, k, D)
    if isinstance(plan, PullStreamPlan):
        ent = plan.ent
        if plan.shift != int(_lib().maxk_pull_shift(int(k))) or ent.shape[0] != E:
            raise RuntimeError(f"the stream plan was not built for this graph at k={k}")
        if row_div is not None and E > 0 and _prescale():
            sc = _scaled_stream_entries(plan, num_rows, k, row_div)
            if sc is not None:
                ent, row_div = sc, None
        _launch_ws(G.device, "maxk_sspmm_backward_pull_stream",
                   "maxk_sspmm_backward_pull_stream_workspace_size", (num_rows, num_cols, D, k),
                   (_ptr(G), _ptr(row_div), _ptr(sel), _ptr(plan.bucket_col), _ptr(plan.grp_ptr),
                    _ptr(ent), plan.n_buckets, _ptr(out), *shape))
        return
    tptr, ent, shift, S = plan
    if row_div is not None and E > 0 and _prescale():
        sc = _scaled_entries(ent, None, tptr, num_rows, num_cols, shift, S, row_div)
        if sc is not None:
            ent, row_div = sc, None
    _launch_ws(G.device, "maxk_sspmm_backward_pull", "maxk_sspmm_backward_pull_workspace_size",
               (num_rows, num_cols, D, k, S),
               (_ptr(G), _ptr(row_div), _ptr(sel), _ptr(tptr), _ptr(ent), shift, S, _ptr(out),
                *shape))


def _bwd_bsort(indptr, indices, values, G, row_div, sel, edge_sel, out, shape, chunk, plan):
    k = shape[4]
    if k > BSORT_KMAX and (id(indptr), k) not in _BSORT_WARNED:
        _BSORT_WARNED.add((id(indptr), k))
        warnings.warn(f"backward mode 'bsort' at k={k} > {BSORT_KMAX} (MAXK_BSORT_KMAX): a "
                      f"window of {int(_lib().maxk_bsort_window(k))} edges holds few rows per "
                      "destination bucket; correct, but csc is faster", stacklevel=3)
    bptr, bpos, bdst, wsrc, wrow, shift = (plan if plan is not None
                                           else bsort_plan(indptr, indices, shape[1], k))
    _launch_ws(G.device, "maxk_sspmm_backward_bsort", "maxk_sspmm_backward_bsort_workspace_size",
               shape,
               (_ptr(indptr), _ptr(indices), _ptr(values), _ptr(G), _ptr(row_div), _ptr(sel),
                _ptr(edge_sel), _ptr(bptr), _ptr(bpos), _ptr(bdst), _ptr(wsrc), _ptr(wrow), shift,
                _ptr(out), *shape))


def _bwd_atomic(indptr, indices, values, G, row_div, sel, edge_sel, out, shape, chunk, plan):
    _launch_ws(G.device, "maxk_sspmm_backward", "maxk_sspmm_backward_workspace_size",
               (*shape, chunk),
               (_ptr(indptr), _ptr(indices), _ptr(values), _ptr(G), _ptr(row_div), _ptr(sel),
                _ptr(out), *shape, chunk))


def _bwd_csc(indptr, indices, values, G, row_div, sel, edge_sel, out, shape, chunk, plan):
    col_ptr, csc_eid = plan if plan is not None else transpose_plan(indices, shape[1])
    name = "maxk_sspmm_backward_csc"
    if edge_sel is not None:  # the per-edge selectors take the selector table's place
        name, sel = name + "_sel", edge_sel
    _launch_ws(G.device, name, "maxk_sspmm_backward_csc_workspace_size", (*shape, chunk),
               (_ptr(indptr), _ptr(indices), _ptr(values), _ptr(G), _ptr(row_div), _ptr(sel),
                _ptr(col_ptr), _ptr(csc_eid), _ptr(out), *shape, chunk))


_BWD = {"dense": _bwd_dense, "hybrid": _bwd_hybrid, "pull": _bwd_pull, "bsort": _bwd_bsort,
        "atomic": _bwd_atomic, "csc": _bwd_csc}


def sspmm_backward_heads(indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor,
                         grad_output: torch.Tensor, cbsr_idx: torch.Tensor,
                         row_div: Optional[torch.Tensor] = None, chunk: int = 0,
                         out: Optional[torch.Tensor] = None, validate: Optional[bool] = None,
                         plan=None) -> torch.Tensor:
    """grad_cbsr[num_cols, k]: the feature gradient of spgemm_forward_heads, the sum over the H
    heads of sspmm_backward(..., values[h], grad_output[h], ..., mode="csc"), with the heads
    summed per edge before the contribution row is stored: one selector gather, one row written
    and one row read per edge whatever H (maxk_sspmm_backward_heads).  values [H, E],
    grad_output [H, num_rows, D], 1 <= H <= MAX_HEADS; row_div is shared by the heads.  Two-phase
    and atomic-free like mode "csc": bitwise repeatable, and at H == 1 bitwise that call.  Uses
    the graph's transpose plan (cached per `indices`, or `plan=` from transpose_plan()), which
    depends on the graph alone: weights that change every step never rebuild it.  The same
    operand checks as the other multi-head calls."""
    _need(values, "values", torch.float32)
    _need(grad_output, "grad_output", torch.float32)
    _need(indptr, "indptr", torch.int32)
    _need(indices, "indices", torch.int32)
    _need(cbsr_idx, "sparse_selector", torch.uint8)
    if grad_output.dim() != 3 or not 1 <= grad_output.shape[0] <= MAX_HEADS:
        raise RuntimeError(f"grad_output must be [H, num_rows, dim_origin] with 1 <= H <= "
                           f"{MAX_HEADS}")
    H, _, D = grad_output.shape
    if cbsr_idx.dim() != 2:
        raise RuntimeError("sparse_selector must be [V, k]")
    num_cols, k = cbsr_idx.shape
    num_rows = indptr.numel() - 1
    E = indices.numel()
    if grad_output.shape[1] != num_rows:
        raise RuntimeError("grad_output must be [H, num_rows, dim_origin]")
    if tuple(values.shape) != (H, E):
        raise RuntimeError("values must be [H, num_e], H that of grad_output")
    if row_div is not None:
        _need(row_div, "row_div", torch.float32)
        if row_div.numel() != num_rows:
            raise RuntimeError("row_div must have num_rows entries")
    _validate_call(validate, indptr, indices, num_cols, cbsr_idx, D)
    dev = grad_output.device
    out = _heads_out(out, (num_cols, k), dev, "[num_cols, k]")
    col_ptr, csc_eid = plan if plan is not None else transpose_plan(indices, num_cols)
    shape = (num_rows, num_cols, E, D, k, H, chunk)
    _launch_ws(dev, "maxk_sspmm_backward_heads", "maxk_sspmm_backward_heads_workspace_size", shape,
               (_ptr(indptr), _ptr(indices), _ptr(values), _ptr(grad_output), _ptr(row_div),
                _ptr(cbsr_idx), _ptr(col_ptr), _ptr(csc_eid), _ptr(out), *shape))
    return out


HEADS_MAX_COLS = 1 << 24  # the multi-head entries reject tables of this many columns


def heads_backward_route(k: int, num_e: int, num_cols: int, num_rows: int,
                         num_heads: Optional[int] = None) -> str:
    """How a multi-head aggregation's feature backward runs (MaxKSpGEMMHeadsFunction.backward):
    "heads", one sspmm_backward_heads call, or "calls", H sspmm_backward calls in
    graph_only_mode's mode added in head order.  Measured (profiles/r13/heads_bwd/, DESIGN.md
    5.8), heads / calls at H = 2, 4, 8: Reddit-sized k = 16 0.54, 0.29, 0.16; products-sized
    k = 32 0.53, 0.31, 0.21; products-sized k = 8, where the calls run bsort, 0.70, 0.42, 0.33
    -- each far past the calls' run-to-run spread of at most 2.9 %, so the rule needs no
    threshold: "heads" on every graph the entry takes.  Only one head shares nothing: the
    single call is the same work (csc: 1.07 and 1.02) or the faster bsort (1.25), so
    num_heads == 1, when given, returns "calls".
    "calls" also for a table the multi-head entry rejects (HEADS_MAX_COLS columns or more) and,
    unless MAXK_HEADS_BWD=heads|calls forces a route, when MAXK_BWD_MODE forces a backward mode
    (graph_only_mode returns None: the forced mode is what the H calls then run)."""
    if num_cols >= HEADS_MAX_COLS:
        return "calls"
    forced = os.environ.get("MAXK_HEADS_BWD", "")
    if forced in ("heads", "calls"):
        return forced
    if graph_only_mode(k, num_e, num_cols) is None or num_heads == 1:
        return "calls"
    return "heads"


EDGE_SEL_KMAX = 16


def edge_selectors_wanted(k: int) -> bool:
    """The rule for the per-edge selector stream given a csc / bsort backward: k % 4 == 0 and
    k <= EDGE_SEL_KMAX by default (MAXK_EDGE_SEL=auto); MAXK_EDGE_SEL=0 never, =1 at every
    k % 4 == 0.  Measured on the ogbn-products-sized graph: the forward that
    writes the stream takes +0.68 / +0.80 / +0.79 ms at k = 8 / 16 / 32, the csc backward that
    reads it -1.16 / -1.08 / -0.93 ms.  At k = 32 that nets +1 % on the bench step and -1.5 % on
    the 3-layer training epoch (r04, one box, alternating runs: 13.46 -> 13.31 ms, 100.1 ->
    101.6 ms; profiles/r04/tune/es32/), for num_e * k bytes (4 GB) held per layer from the
    forward to the backward, so the default stops at 16; none at 64 (+2.15 / -1.33 ms)."""
    mode = os.environ.get("MAXK_EDGE_SEL", "auto")
    if k % 4 or mode == "0":
        return False
    return mode == "1" or k <= EDGE_SEL_KMAX


def edge_selector_mode(indptr: torch.Tensor, indices: torch.Tensor, k: int, num_cols: int,
                       dim: Optional[int] = None, mode: Optional[str] = None) -> Optional[str]:
    """The backward mode a forward should write the per-edge selector stream for
    (spgemm_forward(edge_sel_out=) -> sspmm_backward(edge_sel=, mode=)), or None: the backward
    resolves to "csc" or "bsort" (large sparse graphs without locality, where phase 1
    otherwise gathers a 128-B line of the selector table per edge) and
    edge_selectors_wanted(k).  The stream holds num_e * k bytes until the backward.  `mode`:
    the backward's mode when the caller has already resolved it (graph_only_mode)."""
    if indices.numel() == 0 or not edge_selectors_wanted(k):
        return None
    if mode is None:
        mode = _bwd_mode(None, k, indices.numel(), num_cols, indptr.numel() - 1, dim,
                         (indptr, indices))
    return mode if mode in ("csc", "bsort") else None


def use_edge_selectors(indptr: torch.Tensor, indices: torch.Tensor, k: int, num_cols: int,
                       dim: Optional[int] = None) -> bool:
    """Whether a forward should write the per-edge selector stream (edge_selector_mode)."""
    return edge_selector_mode(indptr, indices, k, num_cols, dim) is not None


def edge_selectors(indices: torch.Tensor, cbsr_idx: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [E, k]: edge e's destination selectors, cbsr_idx[indices[e]] (any k, any
    alignment), for sspmm_backward(..., edge_sel=) (maxk_edge_selectors)."""
    _need(indices, "indices", torch.int32)
    _need(cbsr_idx, "sparse_selector", torch.uint8)
    E, k = indices.numel(), cbsr_idx.shape[1]
    if out is None:
        out = torch.empty(E, k, dtype=torch.uint8, device=indices.device)
    _launch(indices.device, "maxk_edge_selectors", _ptr(indices), _ptr(cbsr_idx), E, k, _ptr(out),
            _stream(indices.device))
    return out


def spmm_maxk_forward(warp4_metadata: torch.Tensor, indices: torch.Tensor, values: torch.Tensor,
                      input_data: torch.Tensor, sparse_selector: torch.Tensor, num_warps: int,
                      dim_sparse: int, *, dim_origin: int = FULL_DIM,
                      indptr: Optional[torch.Tensor] = None,
                      row_div: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MaxK forward SpGEMM (cuda_kernel_bindings.cpp:42-104): returns f32 [V, dim_origin]."""
    _need(input_data, "input_data", torch.float32)
    if input_data.dim() != 2 or input_data.shape[1] != dim_sparse:
        raise RuntimeError("input_data must be [V, dim_sparse]")
    if indptr is None:
        indptr = warp4_to_indptr(warp4_metadata, input_data.shape[0], num_warps)
    return spgemm_forward(indptr, indices, values, input_data, sparse_selector, dim_origin,
                          row_div=row_div)


def spmm_maxk_backward(warp4_metadata: torch.Tensor, indices: torch.Tensor, values: torch.Tensor,
                       grad_output: torch.Tensor, sparse_selector: torch.Tensor, num_warps: int,
                       dim_sparse: int, *, indptr: Optional[torch.Tensor] = None,
                       row_div: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MaxK backward SSpMM (cuda_kernel_bindings.cpp:106-161): returns f32 [V, dim_sparse]."""
    _need(grad_output, "grad_output", torch.float32)
    _need(sparse_selector, "sparse_selector", torch.uint8)
    if sparse_selector.dim() != 2 or sparse_selector.shape[1] != dim_sparse:
        raise RuntimeError("sparse_selector must be [V, dim_sparse]")
    if indptr is None:
        indptr = warp4_to_indptr(warp4_metadata, grad_output.shape[0], num_warps)
    return sspmm_backward(indptr, indices, values, grad_output, sparse_selector, row_div=row_div)


# --------------------------------------------------------------------------- CBSR encode
def topk_cbsr(x: torch.Tensor, k: int, with_int32: bool = False):
    """(values, uint8 indices[, int32 indices]) = torch.topk(x, k, dim=1) on the GPU kernel."""
    if x.dim() != 2:
        raise RuntimeError("Input must be 2D tensor")
    if not x.is_cuda:
        raise RuntimeError("Input must be on CUDA")
    if x.stride(1) != 1:
        x = x.contiguous()
    V, D = x.shape
    if not (0 < k <= D):
        raise RuntimeError("Invalid k value")
    dev = x.device
    val = torch.empty(V, k, dtype=x.dtype, device=dev)
    idx = torch.empty(V, k, dtype=torch.uint8, device=dev)
    idx32 = torch.empty(V, k, dtype=torch.int32, device=dev) if with_int32 else None
    if x.dtype == torch.float32:
        name = "maxk_topk_cbsr"
    elif x.dtype == torch.uint8:
        name = "maxk_topk_cbsr_u8"
    else:
        raise RuntimeError("Input must be float32 or uint8")
    check = _checks_topk_rows(dev)
    _launch(dev, name, _ptr(x), x.stride(0), _ptr(val), _ptr(idx), _ptr(idx32), V, D, k,
            _stream(dev))
    if check:
        _check_topk_rows(dev, name)
    return (val, idx, idx32) if with_int32 else (val, idx)


def topk_error_rows(device=None, reset: bool = True) -> int:
    """Rows whose top-k search took other than k winners on `device` since the last reset
    (maxk_topk_error_rows; read in order on torch's current stream, which it synchronises).
    Always 0 unless the kernel has a bug: the kernels count such a row and keep its writes
    inside its own k winner slots."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    n = ctypes.c_int64(0)
    _launch(dev, "maxk_topk_error_rows", ctypes.byref(n), 1 if reset else 0, _stream(dev))
    return int(n.value)


def _checks_topk_rows(dev) -> bool:
    """MAXK_VALIDATE=1 outside a capture: zero the device's bad-row count before the launch
    (a count left by an earlier unvalidated call is not this launch's), so the
    read after it (_check_topk_rows) sees this launch's rows only.  Both run on the current
    stream, in order with the launch."""
    if not _validate_default() or torch.cuda.is_current_stream_capturing():
        return False
    topk_error_rows(dev, reset=True)
    return True


def _check_topk_rows(dev, name):
    """Raise if the launch just made left a row with other than k winners."""
    bad = topk_error_rows(dev)
    if bad:
        raise RuntimeError(f"{name}: {bad} rows took other than k winners (kernel bug)")


def topk_u8_reference(input: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference uint8 top-k's intended per-row convention (maxk_topk_u8_reference; rows of
    256 bytes): (values u8 [N,k], indices u8 [N,k]) -- the row's bytes above its own 8-step
    bisection threshold in ascending column order, the lane-31 overwrite and zero-filled slots
    included.  Not the CUDA kernel as built, which thresholds every row on its block's first
    row per lane, with a shared-memory race and uninitialised slots (kernels/maxk_kernel.cu:42,
    :44-48, :91-94; oracle.topk_u8_reference_as_built models it, and it agrees with this on
    0.2 % of uniform rows): parity with the CUDA kernel is unpinned."""
    _need(input, "input", torch.uint8)
    if input.dim() != 2 or input.shape[1] != 256:
        raise RuntimeError("the reference's uint8 top-k takes [N, 256] rows")
    if not 0 < k <= 256:
        raise RuntimeError("Invalid k value")
    N = input.shape[0]
    val = torch.empty(N, k, dtype=torch.uint8, device=input.device)
    idx = torch.empty(N, k, dtype=torch.uint8, device=input.device)
    _launch(input.device, "maxk_topk_u8_reference", _ptr(input), _ptr(val), _ptr(idx), N, 256,
            int(k), _stream(input.device))
    return val, idx


def cuda_topk_maxk(input: torch.Tensor, k: int,
                   reference_compat: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """uint8 top-k (cuda_kernel_bindings.cpp:164-201): (values u8 [N,k], indices u8 [N,k]).
    Exact torch.topk order by default; reference_compat=True takes the reference kernel's
    intended convention (topk_u8_reference: per-row threshold bisection, ascending columns,
    rows of 256) -- not its as-built output, which is racy; parity with it unpinned."""
    if input.dtype != torch.uint8:
        raise RuntimeError("Input must be uint8 tensor")
    if reference_compat:
        return topk_u8_reference(input, k)
    return topk_cbsr(input, k)


def cuda_topk_maxk_float(input: torch.Tensor, k: int,
                         reference_compat: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(values, int32 indices) (cuda_kernel_bindings.cpp:203-238), exact (no uint8 quantisation)
    by default.  reference_compat=True follows the reference binding: float input quantised to
    clamp(round(x * 255), 0, 255) as uint8, the reference kernel's intended top-k convention on
    that (topk_u8_reference; parity with the as-built CUDA kernel unpinned), values returned as
    float / 255; uint8 input passes through."""
    if not reference_compat:
        val, _, idx32 = topk_cbsr(input, k, with_int32=True)
        return val, idx32
    if input.dtype == torch.float32:
        q = torch.clamp((input * 255.0).round(), 0, 255).to(torch.uint8)
        v8, i8 = topk_u8_reference(q.contiguous(), k)
        # byte / 255 correctly rounded (the device divide may be off by an ulp): a 256-entry
        # table divided on the host
        table = (torch.arange(256, dtype=torch.float32) / 255.0).to(input.device)
        return table[v8.long()], i8.to(torch.int32)
    if input.dtype == torch.uint8:
        v8, i8 = topk_u8_reference(input, k)
        return v8, i8.to(torch.int32)
    raise RuntimeError("Input must be float32 or uint8")


def prepare_cbsr_format_maxk(features: torch.Tensor, maxk: int):
    """(sparse_data, sparse_indices) (cuda_kernel_bindings.cpp:240-251)."""
    return cuda_topk_maxk_float(features, maxk)


def cbsr_scatter_dense(cbsr_val: torch.Tensor, cbsr_idx: torch.Tensor, dim_origin: int,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """zeros(V, D).scatter_(1, idx, val) in one HIP pass (maxk_spgemm_function.py:152,175)."""
    _need(cbsr_val, "cbsr_val", torch.float32)
    _need(cbsr_idx, "cbsr_idx", torch.uint8)
    V, k = cbsr_val.shape
    dev = cbsr_val.device
    if out is None:
        out = torch.empty(V, dim_origin, dtype=torch.float32, device=dev)
    _launch(dev, "maxk_cbsr_scatter_dense", _ptr(cbsr_val), _ptr(cbsr_idx), _ptr(out), V,
            dim_origin, k, _stream(dev))
    return out


def topk_cbsr_dense(x: torch.Tensor, k: int):
    """Fused MaxK forward: (dense masked x, values, uint8 indices) from one HIP kernel --
    torch.topk + zeros_like + scatter_ of model_integrated_v3.py:28-38 in a single pass."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        raise RuntimeError("x must be a float32 CUDA tensor")
    if x.dim() != 2:
        raise RuntimeError("Input must be 2D tensor")
    if x.stride(1) != 1:
        x = x.contiguous()
    V, D = x.shape
    if not (0 < k <= D):
        raise RuntimeError("Invalid k value")
    dev = x.device
    val = torch.empty(V, k, dtype=torch.float32, device=dev)
    idx = torch.empty(V, k, dtype=torch.uint8, device=dev)
    dense = torch.empty(V, D, dtype=torch.float32, device=dev)
    check = _checks_topk_rows(dev)
    _launch(dev, "maxk_topk_cbsr_dense", _ptr(x), x.stride(0), _ptr(val), _ptr(idx), _ptr(dense),
            V, D, k, _stream(dev))
    if check:
        _check_topk_rows(dev, "maxk_topk_cbsr_dense")
    return dense, val, idx


def topk_backward(grad_val: Optional[torch.Tensor], grad_dense: Optional[torch.Tensor],
                  cbsr_idx: torch.Tensor, dim_origin: int,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused MaxK backward: grad_x = scatter(grad_val + grad_dense[sel]) over the selected
    columns, zero elsewhere, in one HIP pass (OPTMaxK.backward, model_integrated_v3.py:39-43,
    with the topk_values gradient it drops; maxk_spgemm_function.py:152,175)."""
    _need(cbsr_idx, "cbsr_idx", torch.uint8)
    V, k = cbsr_idx.shape
    dev = cbsr_idx.device
    if grad_val is not None:
        _need(grad_val, "grad_val", torch.float32)
        if tuple(grad_val.shape) != (V, k):
            raise RuntimeError("grad_val must be [V, k]")
    if grad_dense is not None:
        _need(grad_dense, "grad_dense", torch.float32)
        if tuple(grad_dense.shape) != (V, dim_origin):
            raise RuntimeError("grad_dense must be [V, dim_origin]")
    if out is None:
        out = torch.empty(V, dim_origin, dtype=torch.float32, device=dev)
    else:
        _need(out, "out", torch.float32)
        if tuple(out.shape) != (V, dim_origin):
            raise RuntimeError("out must be [V, dim_origin]")
    _launch(dev, "maxk_topk_backward", _ptr(grad_val), _ptr(grad_dense), _ptr(cbsr_idx), _ptr(out),
            V, dim_origin, k, _stream(dev))
    return out


def generate_sparse_selector(num_v: int, dim_origin: int, dim_sparse: int) -> torch.Tensor:
    """k distinct random columns per row, seed 123 (cuda_kernel_bindings.cpp:320-340).
    Same distribution as the reference's per-row randperm; not the same random stream."""
    gen = torch.Generator(device="cuda").manual_seed(123)
    keys = torch.rand(num_v, dim_origin, generator=gen, device="cuda")
    return topk_cbsr(keys, dim_sparse)[1]


# --------------------------------------------------------------------------- baseline
class DenseSpMMPlan:
    """rocSPARSE Y = A . X (the reference's cuSPARSE denominator, kernels/spmm_cusparse.cu:6-62).
    Buffers are bound at construction; run() launches on the current stream."""

    def __init__(self, indptr, indices, values, x, y=None, alg: int = 0):
        for t, n, dt in ((indptr, "indptr", torch.int32), (indices, "indices", torch.int32),
                         (values, "values", torch.float32), (x, "input_features", torch.float32)):
            _need(t, n, dt)
        self.num_rows = indptr.numel() - 1
        self.x = x
        self.y = y if y is not None else torch.empty(self.num_rows, x.shape[1],
                                                     dtype=torch.float32, device=x.device)
        self._keep = (indptr, indices, values)
        self.device = x.device
        h = ctypes.c_void_p()
        _launch(self.device, "maxk_dense_spmm_plan_create", ctypes.byref(h), _ptr(indptr),
                _ptr(indices), _ptr(values), _ptr(x), _ptr(self.y), self.num_rows, x.shape[0],
                indices.numel(), x.shape[1], alg, _stream(self.device))
        self._h = h

    def run(self, x: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None
            ) -> torch.Tensor:
        """Y = A . X on the current stream; `x` / `y` rebind the dense operands (same shapes)."""
        if x is not None or y is not None:
            x = self.x if x is None else x
            y = self.y if y is None else y
            _need(x, "x", torch.float32)
            _need(y, "y", torch.float32)
            if tuple(x.shape) != tuple(self.x.shape) or tuple(y.shape) != tuple(self.y.shape):
                raise RuntimeError("rebound x / y must keep the plan's shapes")
            _launch(self.device, "maxk_dense_spmm_bind", self._h, _ptr(x), _ptr(y))
            self.x, self.y = x, y
        _launch(self.device, "maxk_dense_spmm_run", self._h, _stream(self.device))
        return self.y

    def close(self):
        if getattr(self, "_h", None):
            _lib().maxk_dense_spmm_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cusparse_spmm(indptr: torch.Tensor, indices: torch.Tensor, values: torch.Tensor,
                  input_features: torch.Tensor, timing: bool = False) -> torch.Tensor:
    """Dense SpMM reference (cuda_kernel_bindings.cpp:253-284), here on rocSPARSE."""
    plan = DenseSpMMPlan(indptr, indices, values, input_features)
    try:
        runs = 10 if timing else 1  # the reference's `timing` only repeats the call
        for _ in range(runs):
            plan.run()
        return plan.y
    finally:
        plan.close()


# --------------------------------------------------------------------------- harness helpers
class CudaTimer:
    """Event timer (cuda_kernel_bindings.cpp:343-369) on the current stream; stop() -> ms."""

    def __init__(self):
        self._a = torch.cuda.Event(enable_timing=True)
        self._b = torch.cuda.Event(enable_timing=True)

    def start(self):
        self._a.record()

    def stop(self) -> float:
        self._b.record()
        self._b.synchronize()
        return self._a.elapsed_time(self._b)


def benchmark_spmm_maxk(warp4_metadata, indices, values, input_data, sparse_selector,
                        num_warps: int, dim_sparse: int, num_runs: int = 4) -> List[float]:
    """num_runs warmup + num_runs timed forward calls (cuda_kernel_bindings.cpp:372-402)."""
    indptr = warp4_to_indptr(warp4_metadata, input_data.shape[0], num_warps)
    for _ in range(num_runs):
        spmm_maxk_forward(warp4_metadata, indices, values, input_data, sparse_selector, num_warps,
                          dim_sparse, indptr=indptr)
    torch.cuda.synchronize()
    times, timer = [], CudaTimer()
    for _ in range(num_runs):
        timer.start()
        spmm_maxk_forward(warp4_metadata, indices, values, input_data, sparse_selector, num_warps,
                          dim_sparse, indptr=indptr)
        times.append(timer.stop())
    return times


def validate_spmm_maxk(warp4_metadata, indices, values, input_data, sparse_selector,
                       reference_output, num_warps: int, dim_sparse: int,
                       tolerance: float = 0.001) -> bool:
    """mean |out - reference| < tolerance (cuda_kernel_bindings.cpp:405-427)."""
    out = spmm_maxk_forward(warp4_metadata, indices, values, input_data, sparse_selector,
                            num_warps, dim_sparse, dim_origin=reference_output.shape[1])
    diff = (out - reference_output).abs()
    print(f"Validation - Max diff: {diff.max().item()}, Avg diff: {diff.mean().item()}")
    return diff.mean().item() < tolerance


def validate_spmm_maxk_backward(warp4_metadata_csc, indices_csc, values_csc, grad_output,
                                sparse_selector, reference_grad_input, num_warps_csc: int,
                                dim_sparse: int, tolerance: float = 0.001) -> bool:
    """mean |grad - reference| < tolerance (binding_v2.py:464-486).  The arrays are the CSR of
    the forward graph: the kernel forms the A^T product itself."""
    g = spmm_maxk_backward(warp4_metadata_csc, indices_csc, values_csc, grad_output,
                           sparse_selector, num_warps_csc, dim_sparse)
    diff = (g - reference_grad_input).abs()
    print(f"Backward Validation - Max diff: {diff.max().item()}, Avg diff: {diff.mean().item()}")
    return diff.mean().item() < tolerance
