#!/usr/bin/env python3
"""The max aggregation against the mean aggregation, and against torch's own segment maximum.

Two kinds of step, each run as a child process of its own under `timeout`, one at a time (at most
one process has the GPU open), so a step that faults or hangs ends the run instead of being
followed by more work on the same card:

  ops:GRAPH:K      on bench.py's synthetic GRAPH (reddit, products) at D = --dim, in one process,
                   after warm-up, with device events, alternating within every iteration:
                     max_fwd        mk.spgemm_max_forward             out and arg
                     max_fwd_noarg  mk.spgemm_max_forward(want_arg=False)   the inference path
                     mean_fwd       mk.spgemm_forward with the in-degrees as divisor
                     max_bwd        mk.spgemm_max_backward            from the forward's arg
                     mean_bwd       mk.sspmm_backward in the mode the library picks
                   The mean is the denominator: it is the library's existing code.
  torch:GRAPH:K    the path a user has without the op, on the masked dense features x_sparse:
                     torch_fwd / torch_step   torch.segment_reduce(x_sparse[indices], "max",
                                              offsets=indptr), alone and with its autograd backward
                     max_fwd / max_step       CSRGraph.aggregate_max on the CBSR of the same
                                              features, alone and with its backward
                   with torch.cuda.max_memory_allocated over one step of each.  The [E, D] gather
                   (and its gradient) must fit in memory: flickr by default.

Reports medians, min, max, the spread (max - min) / median over the iterations and the ratios.
Writes one JSON file and prints it.

  python tools/max_bench.py [--steps ops:reddit:16,ops:reddit:32,ops:products:16,ops:products:32,torch:flickr:16]
                            [--dim 256] [--iters 20] [--warmup 3] [--step-timeout 240]
                            [--out profiles/r23/max_aggregate/bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = "ops:reddit:16,ops:reddit:32,ops:products:16,ops:products:32,torch:flickr:16"


def summary(ts):
    med = statistics.median(ts)
    return dict(median_ms=round(med, 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                spread=round((max(ts) - min(ts)) / med, 4), n=len(ts))


def time_alternating(fns, iters, warmup):
    """{name: summary} of the callables, each timed with device events once per iteration."""
    import torch
    ts = {n: [] for n in fns}
    for it in range(warmup + iters):
        for n, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= warmup:
                ts[n].append(a.elapsed_time(b))
    return {n: summary(v) for n, v in ts.items()}


def peak_of(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def problem(name, k, D, seed, dev):
    import torch

    import bench  # the graph generators, as bench.py uses them
    import maxk_cuda_kernels as mk
    row_ptr, col = bench.maxk_graph.synthetic_graph(name, seed, dev)
    V = row_ptr.numel() - 1
    gen = torch.Generator(device=dev).manual_seed(123)
    x = torch.randn(V, D, generator=gen, device=dev)
    dense, vals, idx = mk.topk_cbsr_dense(x, k)
    G = torch.randn(V, D, generator=gen, device=dev)
    return mk, row_ptr, col, dense, vals, idx, G


def step_ops(name, k, D, iters, warmup, seed):
    import torch
    dev = torch.device("cuda:0")
    mk, row_ptr, col, _, vals, idx, G = problem(name, k, D, seed, dev)
    E = col.numel()
    ones = torch.ones(E, device=dev)
    deg = torch.diff(row_ptr).float().clamp(min=1.0)
    _, arg = mk.spgemm_max_forward(row_ptr, col, vals, idx, D)
    mk.sspmm_backward(row_ptr, col, ones, G, idx, row_div=deg)  # builds the backward's plan
    fns = {
        "max_fwd": lambda: mk.spgemm_max_forward(row_ptr, col, vals, idx, D),
        "max_fwd_noarg": lambda: mk.spgemm_max_forward(row_ptr, col, vals, idx, D, want_arg=False),
        "mean_fwd": lambda: mk.spgemm_forward(row_ptr, col, ones, vals, idx, D, row_div=deg),
        "max_bwd": lambda: mk.spgemm_max_backward(row_ptr, col, idx, arg, G, k),
        "mean_bwd": lambda: mk.sspmm_backward(row_ptr, col, ones, G, idx, row_div=deg),
    }
    r = time_alternating(fns, iters, warmup)
    m = {n: r[n]["median_ms"] for n in r}
    r["ratios"] = {"max_fwd/mean_fwd": round(m["max_fwd"] / m["mean_fwd"], 4),
                   "max_fwd_noarg/mean_fwd": round(m["max_fwd_noarg"] / m["mean_fwd"], 4),
                   "max_bwd/mean_bwd": round(m["max_bwd"] / m["mean_bwd"], 4)}
    r["shape"] = dict(graph=name, V=row_ptr.numel() - 1, E=E, D=D, k=k,
                      winners=int((arg >= 0).sum()))
    return r


def step_torch(name, k, D, iters, warmup, seed):
    import torch

    import bench  # noqa: F401  (puts the package on sys.path)
    import maxk_layers as ML
    dev = torch.device("cuda:0")
    mk, row_ptr, col, dense, vals, idx, G = problem(name, k, D, seed, dev)
    graph = ML.CSRGraph(row_ptr, col)
    col64, off64 = col.long(), row_ptr.long()
    xs = dense.clone().requires_grad_(True)
    tv = vals.clone().requires_grad_(True)

    def torch_fwd():
        with torch.no_grad():
            return torch.segment_reduce(dense[col64], "max", offsets=off64)

    def torch_step():
        xs.grad = None
        torch.segment_reduce(xs[col64], "max", offsets=off64).backward(G)

    def max_fwd():
        with torch.no_grad():
            return graph.aggregate_max(vals, idx, D)

    def max_step():
        tv.grad = None
        graph.aggregate_max(tv, idx, D).backward(G)

    # same numbers wherever a row has edges (an empty segment's maximum is -inf in torch)
    a, b = torch_fwd(), max_fwd()
    has = torch.diff(row_ptr) > 0
    fns = {"torch_fwd": torch_fwd, "max_fwd": max_fwd, "torch_step": torch_step,
           "max_step": max_step}
    r = time_alternating(fns, iters, warmup)
    m = {n: r[n]["median_ms"] for n in r}
    r["ratios"] = {"torch_fwd/max_fwd": round(m["torch_fwd"] / m["max_fwd"], 2),
                   "torch_step/max_step": round(m["torch_step"] / m["max_step"], 2)}
    r["peak_bytes"] = {n: peak_of(fns[n]) for n in ("torch_step", "max_step")}
    r["same_values"] = bool(torch.equal(a[has], b[has]))
    r["shape"] = dict(graph=name, V=row_ptr.numel() - 1, E=col.numel(), D=D, k=k,
                      gather_bytes=col.numel() * D * 4)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", default=STEPS)
    ap.add_argument("--step", help="run one step in this process and print its JSON (children)")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "max_aggregate",
                                                  "bench.json"))
    a = ap.parse_args()
    if a.step:
        kind, name, k = a.step.split(":")
        fn = {"ops": step_ops, "torch": step_torch}[kind]
        print("RESULT " + json.dumps(fn(name, int(k), a.dim, a.iters, a.warmup, a.seed)))
        return 0
    results = {}
    for step in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
               "--step", step, "--dim", str(a.dim), "--iters", str(a.iters), "--warmup",
               str(a.warmup), "--seed", str(a.seed)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            # a fault, an abort or a time limit: nothing more is started on the GPU
            results[step] = dict(failed=p.returncode, stderr=p.stderr[-2000:])
            print(f"{step}: exit status {p.returncode}; stopping", file=sys.stderr)
            break
        results[step] = json.loads(lines[-1][len("RESULT "):])
        print(step, json.dumps(results[step].get("ratios")), flush=True)
    out = dict(dim=a.dim, iters=a.iters, warmup=a.warmup, seed=a.seed, steps=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))
    return 1 if any("failed" in r for r in results.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
