#!/usr/bin/env python3
"""Multi-head aggregation against H calls of the single-head entries it replaces.

Per workload (Reddit-sized D = 256 k = 16, products-sized D = 256 k = 32 and, for the feature
gradient, k = 8, where the single-head baseline is bsort; bench.py's synthetic graphs and
features) and per head count H, in one process, after warm-up, with device events, alternating
within every iteration so all of them see the same clocks and cache state:

  forward_heads      mk.spgemm_forward_heads         one call, values [H, E]
  forward_calls      H x mk.spgemm_forward           on the contiguous slices values[h]
  edge_grad_heads    mk.edge_weight_grad_heads       one call, grad_out [H, V, D]
  edge_grad_calls    H x mk.edge_weight_grad         on the slices grad_out[h]
  feat_grad_heads    mk.sspmm_backward_heads         one call, values [H, E], grad_out [H, V, D]
  feat_grad_calls    H x mk.sspmm_backward           on the slices, in graph_only_mode's mode (csc
                                                     or bsort), and the H - 1 add_ of the results:
                                                     MaxKSpGEMMHeadsFunction.backward's route "calls"

  softmax_fwd_heads  mk.gat_edge_softmax_heads       one call, s_dst / s_src [H, V]   (--pairs softmax)
  softmax_fwd_calls  H x mk.gat_edge_softmax         on the slices
  softmax_bwd_heads  mk.gat_edge_softmax_heads_backward   one call, w / grad_w [H, E]
  softmax_bwd_calls  H x mk.gat_edge_softmax_backward     on the slices
  layer_heads / layer_calls   MaxKMultiHeadGATConv forward plus backward under
                     MAXK_HEADS_SOFTMAX=heads / =calls, out_feats = D / H       (--pairs layer)

  attention_fwd_fused   mk.gat_attention_heads        one call, no alpha        (--pairs attention)
  attention_fwd_stored  mk.gat_edge_softmax_heads, then the forward mk.heads_forward_route picks
                        on the graph (spgemm_forward_heads, or H x spgemm_forward)
  alpha_fused / alpha_stored   mk.gat_edge_alpha_heads from the statistics against
                        mk.gat_edge_softmax_heads: what the fused backward pays to rebuild alpha
  step_fused / step_stored     MaxKMultiHeadGATConv forward plus backward, attention="fused"
                        against "stored", out_feats = D / H, with torch.cuda.max_memory_allocated
                        of one step of each

  attention_bwd_fused    mk.gat_attention_heads_backward   one call      (--pairs attention_bwd)
  attention_bwd_rebuilt  mk.gat_edge_alpha_heads, mk.edge_weight_grad_heads,
                        mk.gat_edge_softmax_heads_backward and the feature gradient
                        mk.heads_backward_route picks: the rebuilt backward it replaces
  step_stored / step_fused_rebuilt / step_fused_fused   the layer's forward plus backward for
                        attention stored, fused with the rebuilt backward and fused with the
                        fused backward, with the peak memory of one step of each

  attention_dropout_fwd / attention_fwd   mk.gat_attention_heads with dropout = 0.6 against
                        without: the mask's cost in the walk            (--pairs attention_dropout)
  attention_dropout_bwd / attention_bwd   mk.gat_attention_heads_backward likewise
  step_stored / step_fused_rebuilt / step_fused_fused   the layer's forward plus backward with
                        attn_drop = 0.6 in its three modes, against step_torch_dropout: the
                        stored path with torch.nn.functional.dropout on alpha, what a user would
                        write without the mask entries; the peak memory of one step of each

  dot_attention_fwd_fused   mk.dot_attention_heads       one call, no logits, no alpha
                                                                        (--pairs dot_attention)
  dot_attention_fwd_stored  exactly what it replaces: mk.edge_weight_grad_heads(grad_output=q),
                        the scale, H x mk.edge_softmax, then mk.spgemm_forward_heads
  dot_alpha_fused / dot_alpha_stored   mk.dot_edge_alpha_heads from the statistics against the
                        logits and the H softmaxes: what the fused backward pays to rebuild alpha
  step_fused / step_stored     MaxKTransformerConv forward plus backward, attention="fused"
                        against "stored", out_feats = D / H, with the peak memory of one step

  dot_attention_bwd_fused    mk.dot_attention_heads_backward   one call
                                                                    (--pairs dot_attention_bwd)
  dot_attention_bwd_rebuilt  exactly what it replaces: mk.dot_edge_alpha_heads,
                        mk.edge_weight_grad_heads, H x mk.edge_softmax_backward,
                        mk.spgemm_forward_heads and the scale, two mk.sspmm_backward_heads and
                        the add_: MaxKDotAttentionHeadsFunction's rebuilt backward
  step_stored / step_fused_rebuilt / step_fused_fused   MaxKTransformerConv forward plus backward
                        for attention stored, fused with the rebuilt backward and fused with the
                        fused backward, with the peak memory of one step of each

  dot_attention_dropout_fwd / dot_attention_fwd   mk.dot_attention_heads with dropout = 0.6
                        against without: the mask's cost in the walk (--pairs dot_attention_dropout)
  dot_attention_dropout_bwd / dot_attention_bwd   mk.dot_attention_heads_backward likewise
  step_stored / step_fused_rebuilt / step_fused_fused   MaxKTransformerConv forward plus backward
                        with attn_drop = 0.6: the stored path, what a user writes without
                        fused_attn_drop, against the masked fused walk with either backward; the
                        peak memory of one step of each

It reports the medians, the ratio heads / calls of each pair, and the run-to-run spread of the
single-head baselines in this run, (max - min) / median over the iterations: the heads kernel
counts as faster only where 1 - ratio exceeds that spread.  For the feature gradient it also
records the largest difference between the two results over the largest magnitude, at the size
timed.  Writes one JSON file and prints it.

  python tools/heads_bench.py [--graphs reddit:16,products:32] [--heads 4,8] [--iters 20]
                              [--pairs forward,edge_grad,feat_grad]
  python tools/heads_bench.py --pairs softmax,layer --heads 1,2,4,8 --out FILE
  python tools/heads_bench.py --pairs attention --heads 1,2,4,8 --out FILE
  python tools/heads_bench.py --pairs attention_dropout --heads 1,2,4,8 --out FILE
  python tools/heads_bench.py --pairs dot_attention --graphs reddit:16,reddit:32,products:16,products:32
                              --heads 1,2,4,8 --out FILE
  python tools/heads_bench.py --pairs dot_attention_bwd --graphs reddit:16,reddit:32,products:16,products:32
                              --heads 1,2,4,8 --out profiles/r20/dot_attention_bwd/bench.json
  python tools/heads_bench.py --pairs dot_attention_dropout --graphs reddit:16,reddit:32,products:16,products:32
                              --heads 1,2,4,8 --iters 10 --warmup 2
                              --out profiles/r22/dot_attn_dropout/bench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402  (the graph generators: bench.maxk_graph, as bench.py uses them)

import maxk_cuda_kernels as mk  # noqa: E402  (bench put the package on sys.path)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ts):
    med = statistics.median(ts)
    return dict(median_ms=round(med, 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                spread=round((max(ts) - min(ts)) / med, 4), n=len(ts))


PAIRS = ("forward", "edge_grad", "feat_grad")
_GRAPH = {}  # the last graph generated: the head counts of one workload share it


def run(name, k, D, H, iters, warmup, seed, dev, pairs=PAIRS):
    mg = bench.maxk_graph
    V = mg.PRESETS[name]["V"]
    if (name, seed) not in _GRAPH:
        _GRAPH.clear()
        _GRAPH[(name, seed)] = mg.synthetic_graph(name, seed, dev)
    row_ptr, col = _GRAPH[(name, seed)]
    E = col.numel()
    gen = torch.Generator(device=dev).manual_seed(123)
    w = torch.rand(H, E, generator=gen, device=dev)
    X = torch.rand(V, D, generator=gen, device=dev)
    deg = torch.diff(row_ptr).clamp(min=1).float()
    cv, ci = mk.topk_cbsr(X, k)
    del X
    y = torch.empty(H if "forward" in pairs else 1, V, D, device=dev)
    G = torch.rand(H, V, D, generator=gen, device=dev)
    ge = torch.empty(H if "edge_grad" in pairs else 0, E, device=dev)
    mode = mk.graph_only_mode(k, E, V)

    def fwd_heads():
        mk.spgemm_forward_heads(row_ptr, col, w, cv, ci, D, row_div=deg, out=y, validate=False)

    def fwd_calls():
        for h in range(H):
            mk.spgemm_forward(row_ptr, col, w[h], cv, ci, D, row_div=deg, out=y[h],
                              validate=False)

    def eg_heads():
        mk.edge_weight_grad_heads(row_ptr, col, cv, ci, G, row_div=deg, out=ge, validate=False)

    def eg_calls():
        for h in range(H):
            mk.edge_weight_grad(row_ptr, col, cv, ci, G[h], row_div=deg, out=ge[h],
                                validate=False)

    def fg_heads():
        return mk.sspmm_backward_heads(row_ptr, col, w, G, ci, row_div=deg, validate=False)

    def fg_calls():
        acc = None
        for h in range(H):
            part = mk.sspmm_backward(row_ptr, col, w[h], G[h], ci, row_div=deg, mode=mode,
                                     validate=False)
            acc = part if acc is None else acc.add_(part)
        return acc

    ops = (("forward_heads", fwd_heads), ("forward_calls", fwd_calls),
           ("edge_grad_heads", eg_heads), ("edge_grad_calls", eg_calls),
           ("feat_grad_heads", fg_heads), ("feat_grad_calls", fg_calls))
    ops = tuple(o for o in ops if o[0].rsplit("_", 1)[0] in pairs)
    mk.spgemm_forward(row_ptr, col, w[0], cv, ci, D, row_div=deg, out=y[0], validate=True)
    for _ in range(warmup):
        for _, fn in ops:
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n, _ in ops}
    for _ in range(iters):
        for n, fn in ops:
            ts[n].append(timed(fn))
    s = {n: summary(t) for n, t in ts.items()}
    r = dict(graph=name, V=V, E=E, D=D, k=k, H=H, feat_grad_calls_mode=mode, **s)
    if "feat_grad" in pairs:  # faster and different is not faster: the two results, at this size
        a, b = fg_heads(), fg_calls()
        r["feat_grad_max_diff_over_max"] = float((a - b).abs().max() / b.abs().max())
    for a in pairs:
        r[f"ratio_{a}_heads_to_calls"] = round(
            s[f"{a}_heads"]["median_ms"] / s[f"{a}_calls"]["median_ms"], 4)
        r[f"{a}_heads_faster"] = bool(
            1.0 - r[f"ratio_{a}_heads_to_calls"] > s[f"{a}_calls"]["spread"])
    return r


SOFTMAX_PAIRS = ("softmax_fwd", "softmax_bwd")


def _graph(name, seed, dev):
    if (name, seed) not in _GRAPH:
        _GRAPH.clear()
        _GRAPH[(name, seed)] = bench.maxk_graph.synthetic_graph(name, seed, dev)
    return _GRAPH[(name, seed)]


def _pair_ratios(r, s, pairs):
    for a in pairs:
        r[f"ratio_{a}_heads_to_calls"] = round(
            s[f"{a}_heads"]["median_ms"] / s[f"{a}_calls"]["median_ms"], 4)
        r[f"{a}_heads_faster"] = bool(
            1.0 - r[f"ratio_{a}_heads_to_calls"] > s[f"{a}_calls"]["spread"])


def run_softmax(name, H, iters, warmup, seed, dev, slope=0.2):
    """mk.gat_edge_softmax_heads and its backward against exactly the H single-head calls each
    replaces, alternating; the largest difference between the two results at this size."""
    V = bench.maxk_graph.PRESETS[name]["V"]
    row_ptr, col = _graph(name, seed, dev)
    E = col.numel()
    gen = torch.Generator(device=dev).manual_seed(321)
    sd = torch.randn(H, V, generator=gen, device=dev)
    ss = torch.randn(H, V, generator=gen, device=dev)
    gw = torch.randn(H, E, generator=gen, device=dev)
    w_h, w_c = torch.empty(H, E, device=dev), torch.empty(H, E, device=dev)
    g_h = (torch.empty(H, V, device=dev), torch.empty(H, V, device=dev))
    g_c = (torch.empty(H, V, device=dev), torch.empty(H, V, device=dev))
    mk.transpose_plan(col, V)  # once per graph, as in training: not part of either side

    def fwd_heads():
        mk.gat_edge_softmax_heads(row_ptr, col, sd, ss, slope, out=w_h, validate=False)

    def fwd_calls():
        for h in range(H):
            mk.gat_edge_softmax(row_ptr, col, sd[h], ss[h], slope, out=w_c[h], validate=False)

    def bwd_heads():
        mk.gat_edge_softmax_heads_backward(row_ptr, col, sd, ss, w_h, gw, slope, out=g_h,
                                           validate=False)

    def bwd_calls():
        for h in range(H):
            mk.gat_edge_softmax_backward(row_ptr, col, sd[h], ss[h], w_c[h], gw[h], slope,
                                         out=(g_c[0][h], g_c[1][h]), validate=False)

    ops = (("softmax_fwd_heads", fwd_heads), ("softmax_fwd_calls", fwd_calls),
           ("softmax_bwd_heads", bwd_heads), ("softmax_bwd_calls", bwd_calls))
    mk.gat_edge_softmax(row_ptr, col, sd[0], ss[0], slope, out=w_c[0], validate=True)
    for _ in range(warmup):
        for _, fn in ops:
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n, _ in ops}
    for _ in range(iters):
        for n, fn in ops:
            ts[n].append(timed(fn))
    s = {n: summary(t) for n, t in ts.items()}
    r = dict(kind="softmax", graph=name, V=V, E=E, H=H, **s)
    r["w_bitwise_equal"] = bool(torch.equal(w_h.view(torch.int32), w_c.view(torch.int32)))
    r["w_max_abs_diff"] = float((w_h - w_c).abs().max())
    for what, a, b in (("grad_s_dst", g_h[0], g_c[0]), ("grad_s_src", g_h[1], g_c[1])):
        r[f"{what}_max_diff_over_max"] = float((a - b).abs().max() / b.abs().max())
    r["workspace_bytes_heads_bwd"] = int(mk._lib().maxk_gat_edge_softmax_heads_backward_workspace_size(
        H, V, V, E, 0))
    r["workspace_bytes_single_bwd"] = int(mk._lib().maxk_gat_edge_softmax_backward_workspace_size(
        V, V, E, 0))
    _pair_ratios(r, s, SOFTMAX_PAIRS)
    return r


def run_layer(name, k, D, H, iters, warmup, seed, dev):
    """MaxKMultiHeadGATConv forward plus backward under MAXK_HEADS_SOFTMAX=calls against =heads,
    alternating; out_feats = D / H."""
    import maxk_layers as ML
    V = bench.maxk_graph.PRESETS[name]["V"]
    row_ptr, col = _graph(name, seed, dev)
    graph = ML.CSRGraph(row_ptr, col)
    torch.manual_seed(7)
    conv = ML.MaxKMultiHeadGATConv(D, D // H, H).to(dev)
    xs, vals, idx = ML.maxk(torch.rand(V, D, device=dev), k)
    xs = xs.detach().requires_grad_(True)
    vals = vals.detach().requires_grad_(True)

    def step(route):
        os.environ["MAXK_HEADS_SOFTMAX"] = route
        conv.zero_grad(set_to_none=True)
        xs.grad = vals.grad = None
        conv(graph, xs, vals, idx).sum().backward()

    routes = ("heads", "calls")
    saved = os.environ.get("MAXK_HEADS_SOFTMAX")
    try:
        for _ in range(warmup):
            for route in routes:
                step(route)
        torch.cuda.synchronize()
        ts = {route: [] for route in routes}
        for _ in range(iters):
            for route in routes:
                ts[route].append(timed(lambda: step(route)))
    finally:
        if saved is None:
            os.environ.pop("MAXK_HEADS_SOFTMAX", None)
        else:
            os.environ["MAXK_HEADS_SOFTMAX"] = saved
    s = {f"layer_{route}": summary(t) for route, t in ts.items()}
    r = dict(kind="layer", graph=name, V=V, E=col.numel(), D=D, k=k, H=H, out_feats=D // H, **s)
    _pair_ratios(r, s, ("layer",))
    return r


def _fused_ratios(r, s, pairs):
    """ratio fused / stored of each pair; faster only past the baseline's spread in this run."""
    for a in pairs:
        r[f"ratio_{a}_fused_to_stored"] = round(
            s[f"{a}_fused"]["median_ms"] / s[f"{a}_stored"]["median_ms"], 4)
        r[f"{a}_fused_faster"] = bool(
            1.0 - r[f"ratio_{a}_fused_to_stored"] > s[f"{a}_stored"]["spread"])


def run_attention(name, k, D, H, iters, warmup, seed, dev, slope=0.2):
    """mk.gat_attention_heads against the softmax and the forward it replaces,
    mk.gat_edge_alpha_heads against the softmax it replaces in the backward, and the layer's
    training step under attention="fused" against "stored", alternating inside every
    iteration; the peak memory of one step of each."""
    import maxk_layers as ML
    V = bench.maxk_graph.PRESETS[name]["V"]
    row_ptr, col = _graph(name, seed, dev)
    E = col.numel()
    gen = torch.Generator(device=dev).manual_seed(654)
    sd = torch.randn(H, V, generator=gen, device=dev)
    ss = torch.randn(H, V, generator=gen, device=dev)
    cv, ci = mk.topk_cbsr(torch.rand(V, D, generator=gen, device=dev), k)
    route = mk.heads_forward_route(V, E)
    y_f, y_s = torch.empty(H, V, D, device=dev), torch.empty(H, V, D, device=dev)
    w = torch.empty(H, E, device=dev)
    w2 = torch.empty(H, E, device=dev)
    stats = []

    def fwd_fused():
        stats[:] = mk.gat_attention_heads(row_ptr, col, sd, ss, cv, ci, D, slope, out=y_f,
                                          validate=False)[1:]

    def fwd_stored():
        mk.gat_edge_softmax_heads(row_ptr, col, sd, ss, slope, out=w, validate=False)
        if route == "heads":
            mk.spgemm_forward_heads(row_ptr, col, w, cv, ci, D, out=y_s, validate=False)
        else:
            for h in range(H):
                mk.spgemm_forward(row_ptr, col, w[h], cv, ci, D, out=y_s[h], validate=False)

    def alpha_fused():
        mk.gat_edge_alpha_heads(row_ptr, col, sd, ss, stats[0], stats[1], slope, out=w2,
                                validate=False)

    def alpha_stored():
        mk.gat_edge_softmax_heads(row_ptr, col, sd, ss, slope, out=w, validate=False)

    ops = (("attention_fwd_fused", fwd_fused), ("attention_fwd_stored", fwd_stored),
           ("alpha_fused", alpha_fused), ("alpha_stored", alpha_stored))
    mk.gat_attention_heads(row_ptr, col, sd, ss, cv, ci, D, slope, out=y_f, validate=True)
    for _ in range(warmup):
        for _, fn in ops:
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n, _ in ops}
    for _ in range(iters):
        for n, fn in ops:
            ts[n].append(timed(fn))
    s = {n: summary(t) for n, t in ts.items()}
    r = dict(kind="attention", graph=name, V=V, E=E, D=D, k=k, H=H, stored_forward_route=route,
             **s)
    r["out_max_diff_over_max"] = float((y_f - y_s).abs().max() / y_s.abs().max())
    r["alpha_max_abs_diff"] = float((w2 - w).abs().max())
    r["workspace_bytes_fused"] = int(mk._lib().maxk_gat_attention_heads_workspace_size(
        V, V, E, D, k, H, 0))
    r["alpha_bytes"] = 4 * H * E
    del y_f, y_s, w, w2
    stats.clear()
    torch.cuda.empty_cache()

    graph = ML.CSRGraph(row_ptr, col)
    torch.manual_seed(7)
    conv = ML.MaxKMultiHeadGATConv(D, D // H, H).to(dev)
    xs, vals, idx = ML.maxk(torch.rand(V, D, device=dev), k)
    xs = xs.detach().requires_grad_(True)
    vals = vals.detach().requires_grad_(True)
    mk.transpose_plan(col, V)

    def step(mode):
        conv.attention = mode
        conv.zero_grad(set_to_none=True)
        xs.grad = vals.grad = None
        conv(graph, xs, vals, idx).sum().backward()

    modes = ("fused", "stored")
    saved = os.environ.pop("MAXK_HEADS_ATTN", None)
    try:
        for _ in range(warmup):
            for mode in modes:
                step(mode)
        torch.cuda.synchronize()
        tl = {mode: [] for mode in modes}
        for _ in range(iters):
            for mode in modes:
                tl[mode].append(timed(lambda: step(mode)))
        for mode in modes:  # the peak of one step, the other mode's buffers released
            conv.zero_grad(set_to_none=True)
            xs.grad = vals.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step(mode)
            torch.cuda.synchronize()
            r[f"step_{mode}_peak_bytes"] = int(torch.cuda.max_memory_allocated())
            r[f"step_{mode}_peak_over_resident_bytes"] = int(torch.cuda.max_memory_allocated()
                                                             - base)
    finally:
        if saved is not None:
            os.environ["MAXK_HEADS_ATTN"] = saved
    sl = {f"step_{mode}": summary(t) for mode, t in tl.items()}
    r.update(sl)
    s.update(sl)
    _fused_ratios(r, s, ("attention_fwd", "alpha", "step"))
    return r


def run_attention_bwd(name, k, D, H, iters, warmup, seed, dev, slope=0.2):
    """mk.gat_attention_heads_backward against exactly what it replaces (gat_edge_alpha_heads,
    edge_weight_grad_heads, gat_edge_softmax_heads_backward and the feature gradient
    heads_backward_route picks), alternating inside every iteration; then the layer's training
    step for attention stored, fused with the rebuilt backward and fused with the fused one, and
    the peak memory of one step of each."""
    import maxk_layers as ML
    V = bench.maxk_graph.PRESETS[name]["V"]
    row_ptr, col = _graph(name, seed, dev)
    E = col.numel()
    gen = torch.Generator(device=dev).manual_seed(987)
    sd = torch.randn(H, V, generator=gen, device=dev)
    ss = torch.randn(H, V, generator=gen, device=dev)
    cv, ci = mk.topk_cbsr(torch.rand(V, D, generator=gen, device=dev), k)
    G = torch.randn(H, V, D, generator=gen, device=dev)
    out, m, z = mk.gat_attention_heads(row_ptr, col, sd, ss, cv, ci, D, slope, validate=True)
    plan = mk.transpose_plan(col, V)  # once per graph, as in training: not part of either side
    route = mk.heads_backward_route(k, E, V, V, H)
    mode = mk.graph_only_mode(k, E, V)
    keep = {}

    def bwd_fused():
        keep["fused"] = mk.gat_attention_heads_backward(row_ptr, col, sd, ss, cv, ci, out, m, z,
                                                        G, slope, validate=False, plan=plan)

    def bwd_rebuilt():  # MaxKGATAttentionHeadsFunction.backward, route "rebuilt"
        alpha = mk.gat_edge_alpha_heads(row_ptr, col, sd, ss, m, z, slope, validate=False)
        gw = mk.edge_weight_grad_heads(row_ptr, col, cv, ci, G, validate=False)
        g_dst, g_src = mk.gat_edge_softmax_heads_backward(row_ptr, col, sd, ss, alpha, gw, slope,
                                                          validate=False)
        del gw
        if route == "heads":
            g_tv = mk.sspmm_backward_heads(row_ptr, col, alpha, G, ci, validate=False, plan=plan)
        else:
            g_tv = None
            for h in range(H):
                part = mk.sspmm_backward(row_ptr, col, alpha[h], G[h], ci, mode=mode,
                                         validate=False)
                g_tv = part if g_tv is None else g_tv.add_(part)
        keep["rebuilt"] = (g_dst, g_src, g_tv)

    ops = (("attention_bwd_fused", bwd_fused), ("attention_bwd_rebuilt", bwd_rebuilt))
    for _ in range(warmup):
        for _, fn in ops:
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n, _ in ops}
    for _ in range(iters):
        for n, fn in ops:
            ts[n].append(timed(fn))
    s = {n: summary(t) for n, t in ts.items()}
    r = dict(kind="attention_bwd", graph=name, V=V, E=E, D=D, k=k, H=H,
             rebuilt_feature_route=route, **s)
    for what, a, b in zip(("grad_s_dst", "grad_s_src", "grad_cbsr"), keep["fused"],
                          keep["rebuilt"]):
        r[f"{what}_max_diff_over_max"] = float((a - b).abs().max() / b.abs().max())
    r["workspace_bytes_fused"] = int(mk._lib().maxk_gat_attention_heads_backward_workspace_size(
        V, V, E, D, k, H, 0))
    r["alpha_bytes"] = 4 * H * E
    for n, fn in ops:  # the peak of one backward over what is resident before it
        keep.clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        r[f"{n}_peak_over_resident_bytes"] = int(torch.cuda.max_memory_allocated() - base)
    keep.clear()
    del out, m, z, G
    torch.cuda.empty_cache()

    graph = ML.CSRGraph(row_ptr, col)
    torch.manual_seed(7)
    conv = ML.MaxKMultiHeadGATConv(D, D // H, H).to(dev)
    xs, vals, idx = ML.maxk(torch.rand(V, D, device=dev), k)
    xs = xs.detach().requires_grad_(True)
    vals = vals.detach().requires_grad_(True)
    modes = {"stored": ("stored", "rebuilt"), "fused_rebuilt": ("fused", "rebuilt"),
             "fused_fused": ("fused", "fused")}

    def step(mode):
        conv.attention, conv.attention_backward = modes[mode]
        conv.zero_grad(set_to_none=True)
        xs.grad = vals.grad = None
        conv(graph, xs, vals, idx).sum().backward()

    saved = {v: os.environ.pop(v, None) for v in ("MAXK_HEADS_ATTN", "MAXK_HEADS_ATTN_BWD")}
    try:
        for _ in range(warmup):
            for mode in modes:
                step(mode)
        torch.cuda.synchronize()
        tl = {mode: [] for mode in modes}
        for _ in range(iters):
            for mode in modes:
                tl[mode].append(timed(lambda: step(mode)))
        for mode in modes:  # the peak of one step, the other modes' buffers released
            conv.zero_grad(set_to_none=True)
            xs.grad = vals.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step(mode)
            torch.cuda.synchronize()
            r[f"step_{mode}_peak_bytes"] = int(torch.cuda.max_memory_allocated())
            r[f"step_{mode}_peak_over_resident_bytes"] = int(torch.cuda.max_memory_allocated()
                                                             - base)
    finally:
        for v, x in saved.items():
            if x is not None:
                os.environ[v] = x
    sl = {f"step_{mode}": summary(t) for mode, t in tl.items()}
    r.update(sl)
    r["ratio_attention_bwd_fused_to_rebuilt"] = round(
        s["attention_bwd_fused"]["median_ms"] / s["attention_bwd_rebuilt"]["median_ms"], 4)
    r["attention_bwd_fused_faster"] = bool(
        1.0 - r["ratio_attention_bwd_fused_to_rebuilt"] > s["attention_bwd_rebuilt"]["spread"])
    r["attention_bwd_fused_slower"] = bool(
        r["ratio_attention_bwd_fused_to_rebuilt"] - 1.0 > s["attention_bwd_rebuilt"]["spread"])
    for a, b in (("fused_fused", "fused_rebuilt"), ("fused_fused", "stored"),
                 ("fused_rebuilt", "stored")):
        r[f"ratio_step_{a}_to_{b}"] = round(
            sl[f"step_{a}"]["median_ms"] / sl[f"step_{b}"]["median_ms"], 4)
    return r


def run_attention_dropout(name, k, D, H, iters, warmup, seed, dev, slope=0.2, p=0.6):
    """The mask's cost: mk.gat_attention_heads and mk.gat_attention_heads_backward with
    dropout = p against the same calls without, alternating inside every iteration; then the
    layer's training step with attn_drop = p in its three modes against the stored path with
    torch.nn.functional.dropout on alpha, and the peak memory of one step of each."""
    import maxk_layers as ML
    V = bench.maxk_graph.PRESETS[name]["V"]
    row_ptr, col = _graph(name, seed, dev)
    E = col.numel()
    gen = torch.Generator(device=dev).manual_seed(987)
    sd = torch.randn(H, V, generator=gen, device=dev)
    ss = torch.randn(H, V, generator=gen, device=dev)
    cv, ci = mk.topk_cbsr(torch.rand(V, D, generator=gen, device=dev), k)
    G = torch.randn(H, V, D, generator=gen, device=dev)
    y = torch.empty(H, V, D, device=dev)
    plan = mk.transpose_plan(col, V)
    mseed = 0x5EED0001
    fw = {False: mk.gat_attention_heads(row_ptr, col, sd, ss, cv, ci, D, slope, validate=True),
          True: mk.gat_attention_heads(row_ptr, col, sd, ss, cv, ci, D, slope, validate=False,
                                       dropout=p, seed=mseed)}
    keep = {}

    def fwd(drop):
        mk.gat_attention_heads(row_ptr, col, sd, ss, cv, ci, D, slope, out=y, validate=False,
                               dropout=p if drop else 0.0, seed=mseed)

    def bwd(drop):
        keep[drop] = mk.gat_attention_heads_backward(
            row_ptr, col, sd, ss, cv, ci, *fw[drop], G, slope, validate=False, plan=plan,
            dropout=p if drop else 0.0, seed=mseed)

    ops = (("attention_dropout_fwd", lambda: fwd(True)), ("attention_fwd", lambda: fwd(False)),
           ("attention_dropout_bwd", lambda: bwd(True)), ("attention_bwd", lambda: bwd(False)))
    for _ in range(warmup):
        for _, fn in ops:
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n, _ in ops}
    for _ in range(iters):
        for n, fn in ops:
            ts[n].append(timed(fn))
    s = {n: summary(t) for n, t in ts.items()}
    r = dict(kind="attention_dropout", graph=name, V=V, E=E, D=D, k=k, H=H, p=p, **s)
    r["dropped_fraction_of_out_zero"] = float((fw[True][0] == 0).float().mean()
                                              - (fw[False][0] == 0).float().mean())
    for what in ("fwd", "bwd"):
        ratio = s[f"attention_dropout_{what}"]["median_ms"] / s[f"attention_{what}"]["median_ms"]
        spread = s[f"attention_{what}"]["spread"]
        r[f"ratio_attention_dropout_{what}_to_plain"] = round(ratio, 4)
        r[f"attention_dropout_{what}_slower"] = bool(ratio - 1.0 > spread)
    keep.clear()
    del fw, G, y
    torch.cuda.empty_cache()

    graph = ML.CSRGraph(row_ptr, col)
    torch.manual_seed(7)
    conv = ML.MaxKMultiHeadGATConv(D, D // H, H, attn_drop=p).to(dev)
    xs, vals, idx = ML.maxk(torch.rand(V, D, device=dev), k)
    xs = xs.detach().requires_grad_(True)
    vals = vals.detach().requires_grad_(True)
    modes = {"stored": ("stored", "rebuilt"), "fused_rebuilt": ("fused", "rebuilt"),
             "fused_fused": ("fused", "fused"), "torch_dropout": None}

    def torch_dropout_forward():  # MaxKMultiHeadGATConv.forward, stored, with F.dropout on alpha
        O = conv.out_feats
        W = conv.fc.weight.view(H, O, D)
        v = torch.cat((torch.einsum("hoi,ho->ih", W, conv.attn_dst),
                       torch.einsum("hoi,ho->ih", W, conv.attn_src)), 1)
        sc = (xs @ v).t().contiguous()
        alpha = ML.gat_edge_softmax_heads(graph, sc[:H], sc[H:], conv.negative_slope)
        alpha = torch.nn.functional.dropout(alpha, p, training=True)
        agg = graph.aggregate_heads(vals, idx, D, alpha)
        return torch.bmm(agg, W.transpose(1, 2)).transpose(0, 1) + conv.bias

    def step(mode):
        conv.zero_grad(set_to_none=True)
        xs.grad = vals.grad = None
        if modes[mode] is None:
            torch_dropout_forward().sum().backward()
        else:
            conv.attention, conv.attention_backward = modes[mode]
            conv(graph, xs, vals, idx).sum().backward()

    saved = {v: os.environ.pop(v, None) for v in ("MAXK_HEADS_ATTN", "MAXK_HEADS_ATTN_BWD")}
    try:
        for _ in range(warmup):
            for mode in modes:
                step(mode)
        torch.cuda.synchronize()
        tl = {mode: [] for mode in modes}
        for _ in range(iters):
            for mode in modes:
                tl[mode].append(timed(lambda: step(mode)))
        for mode in modes:  # the peak of one step, the other modes' buffers released
            conv.zero_grad(set_to_none=True)
            xs.grad = vals.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step(mode)
            torch.cuda.synchronize()
            r[f"step_{mode}_peak_bytes"] = int(torch.cuda.max_memory_allocated())
            r[f"step_{mode}_peak_over_resident_bytes"] = int(torch.cuda.max_memory_allocated()
                                                             - base)
    finally:
        for v, x in saved.items():
            if x is not None:
                os.environ[v] = x
    sl = {f"step_{mode}": summary(t) for mode, t in tl.items()}
    r.update(sl)
    for mode in ("stored", "fused_rebuilt", "fused_fused"):
        r[f"ratio_step_{mode}_to_torch_dropout"] = round(
            sl[f"step_{mode}"]["median_ms"] / sl["step_torch_dropout"]["median_ms"], 4)
    return r


def run_dot_attention(name, k, D, H, iters, warmup, seed, dev):
    """mk.dot_attention_heads against the scores, the H softmaxes and the forward it replaces,
    mk.dot_edge_alpha_heads against the scores and softmaxes it replaces in the backward, and
    MaxKTransformerConv's training step under attention="fused" against "stored", alternating
    inside every iteration; the peak memory of one step of each."""
    import maxk_layers as ML
    V = bench.maxk_graph.PRESETS[name]["V"]
    row_ptr, col = _graph(name, seed, dev)
    E = col.numel()
    gen = torch.Generator(device=dev).manual_seed(655)
    q = torch.randn(H, V, D, generator=gen, device=dev)
    cv, ci = mk.topk_cbsr(torch.rand(V, D, generator=gen, device=dev), k)
    scale = float(D // H) ** -0.5
    y_f, y_s = torch.empty(H, V, D, device=dev), torch.empty(H, V, D, device=dev)
    lg = torch.empty(H, E, device=dev)
    w = torch.empty(H, E, device=dev)
    w2 = torch.empty(H, E, device=dev)
    stats = []

    def scores_and_softmax():
        mk.edge_weight_grad_heads(row_ptr, col, cv, ci, q, out=lg, validate=False)
        lg.mul_(scale)
        for h in range(H):
            mk.edge_softmax(row_ptr, lg[h], out=w[h], validate=False)

    def fwd_fused():
        stats[:] = mk.dot_attention_heads(row_ptr, col, q, cv, ci, D, scale, out=y_f,
                                          validate=False)[1:]

    def fwd_stored():
        scores_and_softmax()
        mk.spgemm_forward_heads(row_ptr, col, w, cv, ci, D, out=y_s, validate=False)

    def alpha_fused():
        mk.dot_edge_alpha_heads(row_ptr, col, q, cv, ci, D, scale, stats[0], stats[1], out=w2,
                                validate=False)

    ops = (("dot_attention_fwd_fused", fwd_fused), ("dot_attention_fwd_stored", fwd_stored),
           ("dot_alpha_fused", alpha_fused), ("dot_alpha_stored", scores_and_softmax))
    mk.dot_attention_heads(row_ptr, col, q, cv, ci, D, scale, out=y_f, validate=True)
    for _ in range(warmup):
        for _, fn in ops:
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n, _ in ops}
    for _ in range(iters):
        for n, fn in ops:
            ts[n].append(timed(fn))
    s = {n: summary(t) for n, t in ts.items()}
    r = dict(kind="dot_attention", graph=name, V=V, E=E, D=D, k=k, H=H, scale=scale, **s)
    r["out_max_diff_over_max"] = float((y_f - y_s).abs().max() / y_s.abs().max())
    r["alpha_max_abs_diff"] = float((w2 - w).abs().max())
    r["workspace_bytes_fused"] = int(mk._lib().maxk_dot_attention_heads_workspace_size(
        V, V, E, D, k, H, 0))
    r["alpha_bytes"] = 4 * H * E
    del y_f, y_s, w, w2, lg, q
    stats.clear()
    torch.cuda.empty_cache()

    graph = ML.CSRGraph(row_ptr, col)
    torch.manual_seed(7)
    conv = ML.MaxKTransformerConv(D, D // H, H).to(dev)
    xs, vals, idx = ML.maxk(torch.rand(V, D, device=dev), k)
    xs = xs.detach().requires_grad_(True)
    vals = vals.detach().requires_grad_(True)
    mk.transpose_plan(col, V)

    def step(mode):
        conv.attention = mode
        conv.zero_grad(set_to_none=True)
        xs.grad = vals.grad = None
        conv(graph, xs, vals, idx).sum().backward()

    modes = ("fused", "stored")
    saved = os.environ.pop("MAXK_DOT_ATTN", None)
    try:
        for _ in range(warmup):
            for mode in modes:
                step(mode)
        torch.cuda.synchronize()
        tl = {mode: [] for mode in modes}
        for _ in range(iters):
            for mode in modes:
                tl[mode].append(timed(lambda: step(mode)))
        for mode in modes:  # the peak of one step, the other mode's buffers released
            conv.zero_grad(set_to_none=True)
            xs.grad = vals.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step(mode)
            torch.cuda.synchronize()
            r[f"step_{mode}_peak_bytes"] = int(torch.cuda.max_memory_allocated())
            r[f"step_{mode}_peak_over_resident_bytes"] = int(torch.cuda.max_memory_allocated()
                                                             - base)
    finally:
        if saved is not None:
            os.environ["MAXK_DOT_ATTN"] = saved
    sl = {f"step_{mode}": summary(t) for mode, t in tl.items()}
    r.update(sl)
    s.update(sl)
    _fused_ratios(r, s, ("dot_attention_fwd", "dot_alpha", "step"))
    return r


def run_dot_attention_bwd(name, k, D, H, iters, warmup, seed, dev):
    """mk.dot_attention_heads_backward against exactly the rebuilt sequence it replaces
    (MaxKDotAttentionHeadsFunction.backward), on the same inputs, alternating inside every
    iteration; then MaxKTransformerConv's training step for attention stored, fused with the
    rebuilt backward and fused with the fused one, and the peak memory of one step of each."""
    import maxk_layers as ML
    V = bench.maxk_graph.PRESETS[name]["V"]
    row_ptr, col = _graph(name, seed, dev)
    E = col.numel()
    gen = torch.Generator(device=dev).manual_seed(655)
    q = torch.randn(H, V, D, generator=gen, device=dev)
    cv, ci = mk.topk_cbsr(torch.rand(V, D, generator=gen, device=dev), k)
    G = torch.randn(H, V, D, generator=gen, device=dev)
    scale = float(D // H) ** -0.5
    out, m, z = mk.dot_attention_heads(row_ptr, col, q, cv, ci, D, scale, validate=True)
    plan = mk.transpose_plan(col, V)  # once per graph, as in training: not part of either side
    keep = {}

    def bwd_fused():
        keep["fused"] = mk.dot_attention_heads_backward(row_ptr, col, q, cv, ci, out, m, z, G,
                                                        scale, validate=False, plan=plan)

    def bwd_rebuilt():  # MaxKDotAttentionHeadsFunction.backward, backward="rebuilt"
        alpha = mk.dot_edge_alpha_heads(row_ptr, col, q, cv, ci, D, scale, m, z, validate=False)
        grad_a = mk.edge_weight_grad_heads(row_ptr, col, cv, ci, G, validate=False)
        grad_l = torch.empty_like(grad_a)
        for h in range(H):
            mk.edge_softmax_backward(row_ptr, alpha[h], grad_a[h], out=grad_l[h])
        del grad_a
        g_q = mk.spgemm_forward_heads(row_ptr, col, grad_l, cv, ci, D, validate=False).mul_(scale)
        g_tv = mk.sspmm_backward_heads(row_ptr, col, alpha, G, ci, validate=False, plan=plan)
        g_tv.add_(mk.sspmm_backward_heads(row_ptr, col, grad_l, q, ci, validate=False, plan=plan),
                  alpha=scale)
        keep["rebuilt"] = (g_q, g_tv)

    ops = (("dot_attention_bwd_fused", bwd_fused), ("dot_attention_bwd_rebuilt", bwd_rebuilt))
    for _ in range(warmup):
        for _, fn in ops:
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n, _ in ops}
    for _ in range(iters):
        for n, fn in ops:
            ts[n].append(timed(fn))
    s = {n: summary(t) for n, t in ts.items()}
    r = dict(kind="dot_attention_bwd", graph=name, V=V, E=E, D=D, k=k, H=H, scale=scale, **s)
    for what, a, b in zip(("grad_q", "grad_cbsr"), keep["fused"], keep["rebuilt"]):
        r[f"{what}_max_diff_over_max"] = float((a - b).abs().max() / b.abs().max())
    HP = 2 if H <= 2 else 4 if H <= 4 else 8
    r["workspace_bytes_fused"] = int(mk._lib().maxk_dot_attention_heads_backward_workspace_size(
        V, V, E, D, k, H, 0))
    r["T_bytes"], r["glT_bytes"], r["out_bytes"] = 4 * (E + 1) * k, 4 * HP * E, 4 * H * V * D
    r["alpha_bytes"] = 4 * H * E
    for n, fn in ops:  # the peak of one backward over what is resident before it
        keep.clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        r[f"{n}_peak_over_resident_bytes"] = int(torch.cuda.max_memory_allocated() - base)
    keep.clear()
    del out, m, z, G, q
    torch.cuda.empty_cache()

    graph = ML.CSRGraph(row_ptr, col)
    torch.manual_seed(7)
    conv = ML.MaxKTransformerConv(D, D // H, H).to(dev)
    xs, vals, idx = ML.maxk(torch.rand(V, D, device=dev), k)
    xs = xs.detach().requires_grad_(True)
    vals = vals.detach().requires_grad_(True)
    modes = {"stored": ("stored", "rebuilt"), "fused_rebuilt": ("fused", "rebuilt"),
             "fused_fused": ("fused", "fused")}

    def step(mode):
        conv.attention, conv.attention_backward = modes[mode]
        conv.zero_grad(set_to_none=True)
        xs.grad = vals.grad = None
        conv(graph, xs, vals, idx).sum().backward()

    saved = {v: os.environ.pop(v, None) for v in ("MAXK_DOT_ATTN", "MAXK_DOT_ATTN_BWD")}
    try:
        for _ in range(warmup):
            for mode in modes:
                step(mode)
        torch.cuda.synchronize()
        tl = {mode: [] for mode in modes}
        for _ in range(iters):
            for mode in modes:
                tl[mode].append(timed(lambda: step(mode)))
        for mode in modes:  # the peak of one step, the other modes' buffers released
            conv.zero_grad(set_to_none=True)
            xs.grad = vals.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step(mode)
            torch.cuda.synchronize()
            r[f"step_{mode}_peak_bytes"] = int(torch.cuda.max_memory_allocated())
            r[f"step_{mode}_peak_over_resident_bytes"] = int(torch.cuda.max_memory_allocated()
                                                             - base)
    finally:
        for v, x in saved.items():
            if x is not None:
                os.environ[v] = x
    sl = {f"step_{mode}": summary(t) for mode, t in tl.items()}
    r.update(sl)
    r["ratio_dot_attention_bwd_fused_to_rebuilt"] = round(
        s["dot_attention_bwd_fused"]["median_ms"] / s["dot_attention_bwd_rebuilt"]["median_ms"], 4)
    r["dot_attention_bwd_fused_faster"] = bool(
        1.0 - r["ratio_dot_attention_bwd_fused_to_rebuilt"]
        > s["dot_attention_bwd_rebuilt"]["spread"])
    r["dot_attention_bwd_fused_slower"] = bool(
        r["ratio_dot_attention_bwd_fused_to_rebuilt"] - 1.0
        > s["dot_attention_bwd_rebuilt"]["spread"])
    for a, b in (("fused_fused", "fused_rebuilt"), ("fused_fused", "stored"),
                 ("fused_rebuilt", "stored")):
        r[f"ratio_step_{a}_to_{b}"] = round(
            sl[f"step_{a}"]["median_ms"] / sl[f"step_{b}"]["median_ms"], 4)
    return r


def run_dot_attention_dropout(name, k, D, H, iters, warmup, seed, dev, p=0.6):
    """The mask's cost: mk.dot_attention_heads and mk.dot_attention_heads_backward with
    dropout = p against the same calls without, alternating inside every iteration; then
    MaxKTransformerConv's training step with attn_drop = p: the stored path (what a user writes
    without fused_attn_drop) against the masked fused walk with the rebuilt and with the fused
    backward, and the peak memory of one step of each."""
    import maxk_layers as ML
    V = bench.maxk_graph.PRESETS[name]["V"]
    row_ptr, col = _graph(name, seed, dev)
    E = col.numel()
    gen = torch.Generator(device=dev).manual_seed(655)
    q = torch.randn(H, V, D, generator=gen, device=dev)
    cv, ci = mk.topk_cbsr(torch.rand(V, D, generator=gen, device=dev), k)
    G = torch.randn(H, V, D, generator=gen, device=dev)
    scale = float(D // H) ** -0.5
    y = torch.empty(H, V, D, device=dev)
    plan = mk.transpose_plan(col, V)
    mseed = 0x5EED0001
    fw = {False: mk.dot_attention_heads(row_ptr, col, q, cv, ci, D, scale, validate=True),
          True: mk.dot_attention_heads(row_ptr, col, q, cv, ci, D, scale, validate=False,
                                       dropout=p, seed=mseed)}
    keep = {}

    def fwd(drop):
        mk.dot_attention_heads(row_ptr, col, q, cv, ci, D, scale, out=y, validate=False,
                               dropout=p if drop else 0.0, seed=mseed)

    def bwd(drop):
        keep[drop] = mk.dot_attention_heads_backward(
            row_ptr, col, q, cv, ci, *fw[drop], G, scale, validate=False, plan=plan,
            dropout=p if drop else 0.0, seed=mseed)

    ops = (("dot_attention_dropout_fwd", lambda: fwd(True)),
           ("dot_attention_fwd", lambda: fwd(False)),
           ("dot_attention_dropout_bwd", lambda: bwd(True)),
           ("dot_attention_bwd", lambda: bwd(False)))
    for _ in range(warmup):
        for _, fn in ops:
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n, _ in ops}
    for _ in range(iters):
        for n, fn in ops:
            ts[n].append(timed(fn))
    s = {n: summary(t) for n, t in ts.items()}
    r = dict(kind="dot_attention_dropout", graph=name, V=V, E=E, D=D, k=k, H=H, p=p, scale=scale,
             **s)
    r["dropped_fraction_of_out_zero"] = float((fw[True][0] == 0).float().mean()
                                              - (fw[False][0] == 0).float().mean())
    for what in ("fwd", "bwd"):
        ratio = (s[f"dot_attention_dropout_{what}"]["median_ms"]
                 / s[f"dot_attention_{what}"]["median_ms"])
        spread = s[f"dot_attention_{what}"]["spread"]
        r[f"ratio_dot_attention_dropout_{what}_to_plain"] = round(ratio, 4)
        r[f"dot_attention_dropout_{what}_slower"] = bool(ratio - 1.0 > spread)
    keep.clear()
    del fw, G, y, q
    torch.cuda.empty_cache()

    graph = ML.CSRGraph(row_ptr, col)
    torch.manual_seed(7)
    conv = ML.MaxKTransformerConv(D, D // H, H, attn_drop=p, fused_attn_drop=True).to(dev)
    xs, vals, idx = ML.maxk(torch.rand(V, D, device=dev), k)
    xs = xs.detach().requires_grad_(True)
    vals = vals.detach().requires_grad_(True)
    modes = {"stored": ("stored", "rebuilt"), "fused_rebuilt": ("fused", "rebuilt"),
             "fused_fused": ("fused", "fused")}

    def step(mode):
        conv.attention, conv.attention_backward = modes[mode]
        conv.zero_grad(set_to_none=True)
        xs.grad = vals.grad = None
        conv(graph, xs, vals, idx, attn_seed=mseed).sum().backward()

    saved = {v: os.environ.pop(v, None) for v in ("MAXK_DOT_ATTN", "MAXK_DOT_ATTN_BWD")}
    try:
        for _ in range(warmup):
            for mode in modes:
                step(mode)
        torch.cuda.synchronize()
        tl = {mode: [] for mode in modes}
        for _ in range(iters):
            for mode in modes:
                tl[mode].append(timed(lambda: step(mode)))
        for mode in modes:  # the peak of one step, the other modes' buffers released
            conv.zero_grad(set_to_none=True)
            xs.grad = vals.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step(mode)
            torch.cuda.synchronize()
            r[f"step_{mode}_peak_bytes"] = int(torch.cuda.max_memory_allocated())
            r[f"step_{mode}_peak_over_resident_bytes"] = int(torch.cuda.max_memory_allocated()
                                                             - base)
    finally:
        for v, x in saved.items():
            if x is not None:
                os.environ[v] = x
    sl = {f"step_{mode}": summary(t) for mode, t in tl.items()}
    r.update(sl)
    r["alpha_bytes"] = 4 * H * E
    for a in ("fused_rebuilt", "fused_fused"):
        ratio = sl[f"step_{a}"]["median_ms"] / sl["step_stored"]["median_ms"]
        spread = sl["step_stored"]["spread"]
        r[f"ratio_step_{a}_to_stored"] = round(ratio, 4)
        r[f"step_{a}_faster"] = bool(1.0 - ratio > spread)
        r[f"step_{a}_slower"] = bool(ratio - 1.0 > spread)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--graphs", default="reddit:16,products:32")
    ap.add_argument("--heads", default="4,8")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--pairs", default=",".join(PAIRS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "heads", "bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
               build_config=mk._lib().maxk_build_config().decode(), workloads=[])
    asked = args.pairs.split(",")
    pairs = tuple(p for p in PAIRS if p in asked)
    for spec in args.graphs.split(","):
        name, k = spec.split(":")
        for H in (int(h) for h in args.heads.split(",")):
            rs = []
            if pairs:
                rs.append(run(name, int(k), args.dim, H, args.iters, args.warmup, args.seed, dev,
                              pairs))
            if "softmax" in asked:
                rs.append(run_softmax(name, H, args.iters, args.warmup, args.seed, dev))
            if "attention" in asked:
                rs.append(run_attention(name, int(k), args.dim, H, args.iters, args.warmup,
                                        args.seed, dev))
            if "attention_bwd" in asked:
                rs.append(run_attention_bwd(name, int(k), args.dim, H, args.iters, args.warmup,
                                            args.seed, dev))
            if "attention_dropout" in asked:
                rs.append(run_attention_dropout(name, int(k), args.dim, H, args.iters,
                                                args.warmup, args.seed, dev))
            if "dot_attention" in asked:
                rs.append(run_dot_attention(name, int(k), args.dim, H, args.iters, args.warmup,
                                            args.seed, dev))
            if "dot_attention_bwd" in asked:
                rs.append(run_dot_attention_bwd(name, int(k), args.dim, H, args.iters,
                                                args.warmup, args.seed, dev))
            if "dot_attention_dropout" in asked:
                rs.append(run_dot_attention_dropout(name, int(k), args.dim, H, args.iters,
                                                    args.warmup, args.seed, dev))
            if "layer" in asked and H >= 2:
                rs.append(run_layer(name, int(k), args.dim, H, args.iters, args.warmup,
                                    args.seed, dev))
            for r in rs:
                print(json.dumps(r), flush=True)
                res["workloads"].append(r)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
