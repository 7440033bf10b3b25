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

It reports the medians, the ratio heads / calls of each pair, and the run-to-run spread of the
single-head baselines in this run, (max - min) / median over the iterations: the heads kernel
counts as faster only where 1 - ratio exceeds that spread.  For the feature gradient it also
records the largest difference between the two results over the largest magnitude, at the size
timed.  Writes one JSON file and prints it.

  python tools/heads_bench.py [--graphs reddit:16,products:32] [--heads 4,8] [--iters 20]
                              [--pairs forward,edge_grad,feat_grad]
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
    for spec in args.graphs.split(","):
        name, k = spec.split(":")
        for H in (int(h) for h in args.heads.split(",")):
            r = run(name, int(k), args.dim, H, args.iters, args.warmup, args.seed, dev,
                    tuple(p for p in PAIRS if p in args.pairs.split(",")))
            print(json.dumps(r), flush=True)
            res["workloads"].append(r)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
