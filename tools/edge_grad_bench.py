#!/usr/bin/env python3
"""Edge-weight gradient against the forward it is the adjoint of, and the plan build it avoids.

Per workload (Reddit-sized D = 256 k = 16, products-sized D = 256 k = 32; bench.py's synthetic
graphs, values and features), in one process, after warm-up, with device events:

  forward      mk.spgemm_forward      -- the yardstick: the same E record gathers
  edge_grad    mk.edge_weight_grad    -- alternating with the forward, 20 iterations each
  pull_plan    mk.pull_plan(cache=False) -- what a weight tensor that changes every step would
               rebuild per call if the feature backward took a weight-embedding plan
               (maxk_cuda_kernels.graph_only_mode avoids it)

and the byte model of DESIGN.md: B = 4(V+1) + 4E + E*RS + 4VD + 4E + the pack.  Writes one JSON
file (default profiles/r07/edge_grad/bench.json) and prints it.

  python tools/edge_grad_bench.py [--graphs reddit:16,products:32] [--iters 20] [--out FILE]
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


def record_stride(k, num_cols):
    """csrc/cbsr_pack.h record_stride."""
    b = 6 * k
    if b <= 128:
        s = 16
        while s < b:
            s <<= 1
        return s
    s64 = (b + 63) // 64 * 64
    return s64 if s64 * num_cols <= (128 << 20) else (b + 127) // 128 * 128


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ts):
    return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4),
                max_ms=round(max(ts), 4), n=len(ts))


def run(name, k, D, iters, warmup, seed, dev):
    mg = bench.maxk_graph
    V = mg.PRESETS[name]["V"]
    row_ptr, col = mg.synthetic_graph(name, seed, dev)
    E = col.numel()
    gen = torch.Generator(device=dev).manual_seed(123)
    val = torch.rand(E, generator=gen, device=dev)
    X = torch.rand(V, D, generator=gen, device=dev)
    G = torch.rand(V, D, generator=gen, device=dev)
    deg = torch.diff(row_ptr).clamp(min=1).float()
    cv, ci = mk.topk_cbsr(X, k)
    del X
    y = torch.empty(V, D, device=dev)
    ge = torch.empty(E, device=dev)

    def fwd():
        mk.spgemm_forward(row_ptr, col, val, cv, ci, D, row_div=deg, out=y, validate=False)

    def egrad():
        mk.edge_weight_grad(row_ptr, col, cv, ci, G, row_div=deg, out=ge, validate=False)

    def plan():
        mk.pull_plan(row_ptr, col, val, V, k, D, cache=False)

    mk.spgemm_forward(row_ptr, col, val, cv, ci, D, row_div=deg, out=y, validate=True)
    for _ in range(warmup):
        fwd()
        egrad()
    plan()
    torch.cuda.synchronize()
    t_f, t_g, t_p = [], [], []
    for _ in range(iters):  # alternating: both ops see the same clocks and cache state
        t_f.append(timed(fwd))
        t_g.append(timed(egrad))
    for _ in range(iters):
        t_p.append(timed(plan))
    RS = record_stride(k, V)
    pack = V * 5 * k + V * RS
    b_grad = 4 * (V + 1) + 4 * E + E * RS + 4 * V * D + 4 * E + pack
    b_fwd = 4 * (V + 1) + 8 * E + E * RS + 4 * V * D + pack
    f, g, p = summary(t_f), summary(t_g), summary(t_p)
    return dict(graph=name, V=V, E=E, D=D, k=k, record_stride=RS, forward=f, edge_grad=g,
                pull_plan=p,
                ratio_edge_grad_to_forward=round(g["median_ms"] / f["median_ms"], 4),
                ratio_of_mins=round(g["min_ms"] / f["min_ms"], 4),
                pull_plan_in_forwards=round(p["median_ms"] / f["median_ms"], 2),
                model_bytes=dict(edge_grad=b_grad, forward=b_fwd,
                                 ratio=round(b_grad / b_fwd, 4)),
                model_gbs=dict(edge_grad=round(b_grad / g["median_ms"] / 1e6, 1),
                               forward=round(b_fwd / f["median_ms"] / 1e6, 1)),
                backward_mode=dict(auto=mk._bwd_mode("auto", k, E, V, V, D, (row_ptr, col)),
                                   with_weight_grad=mk.graph_only_mode(k, E, V)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--graphs", default="reddit:16,products:32")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "edge_grad",
                                                  "bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
               build_config=mk._lib().maxk_build_config().decode(), workloads=[])
    for spec in args.graphs.split(","):
        name, k = spec.split(":")
        r = run(name, int(k), args.dim, args.iters, args.warmup, args.seed, dev)
        print(json.dumps(r), flush=True)
        res["workloads"].append(r)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
