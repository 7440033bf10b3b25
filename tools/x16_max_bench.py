#!/usr/bin/env python3
"""The max aggregation on 16-bit selectors (x16_max.hip) against what a user has past 256 columns
and against the library's own denominators.

Steps, each a child process of its own under `timeout`, one at a time (a step that faults or
hangs ends the run), on bench.py's synthetic graphs, timed as tools/max_bench.py times (device
events, warm-up, sides alternating inside every iteration, medians with min, max and spread):

  torch:GRAPH:D:K  the path a user has at D > 256, on the masked dense features x_sparse:
                     torch_fwd / torch_step   torch.segment_reduce(x_sparse[indices], "max",
                                              offsets=indptr), alone and with its backward
                     max_fwd / max_step       CSRGraph.aggregate_max on the int16 CBSR of the same
                                              features, alone and with its backward
                   and torch.cuda.max_memory_allocated over one step of each.  The [E, D] gather
                   and its gradient must fit in memory: flickr.  (On the Reddit-sized graph the
                   gather alone is E * D * 4 = 235 GB at D = 512; it is not attempted.)
  mean:GRAPH:D:K   x16 max forward (with and without arg) and backward against the x16 mean
                   forward and backward (spgemm_forward_x16 / sspmm_backward_x16), same graph, k.
  u8:GRAPH:D:K     D <= 256: the u8 max forward and backward (spgemm_max.hip) against the x16 max
                   entries on the same selectors -- the straightforward max backward against the
                   two-phase one.

  python tools/x16_max_bench.py [--steps torch:flickr:384:32,...] [--iters 20] [--warmup 3]
                                [--out profiles/r27/x16_max/bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from max_bench import peak_of, time_alternating  # noqa: E402  (tools/ is the script's directory)

STEPS = "torch:flickr:384:32,torch:flickr:512:32,mean:reddit:512:32,u8:reddit:256:32"


def problem(name, k, D, seed, dev):
    import torch

    import bench  # the graph generators, as bench.py uses them
    import maxk_cuda_kernels as mk
    row_ptr, col = bench.maxk_graph.synthetic_graph(name, seed, dev)
    V = row_ptr.numel() - 1
    gen = torch.Generator(device=dev).manual_seed(123)
    x = torch.randn(V, D, generator=gen, device=dev)
    dense, vals, idx = mk.topk_cbsr_dense_x16(x, k)
    G = torch.randn(V, D, generator=gen, device=dev)
    return mk, row_ptr, col, dense, vals, idx, G


def ratios(r, pairs):
    return {f"{a}/{b}": round(r[a]["median_ms"] / r[b]["median_ms"], 4) for a, b in pairs}


def step_mean(name, k, D, iters, warmup, seed):
    import torch
    dev = torch.device("cuda:0")
    mk, row_ptr, col, _, vals, idx, G = problem(name, k, D, seed, dev)
    ones = torch.ones(col.numel(), device=dev)
    deg = torch.diff(row_ptr).float().clamp(min=1.0)
    _, arg = mk.spgemm_max_forward_x16(row_ptr, col, vals, idx, D)
    fns = {
        "max_fwd": lambda: mk.spgemm_max_forward_x16(row_ptr, col, vals, idx, D),
        "max_fwd_noarg": lambda: mk.spgemm_max_forward_x16(row_ptr, col, vals, idx, D,
                                                           want_arg=False),
        "mean_fwd": lambda: mk.spgemm_forward_x16(row_ptr, col, ones, vals, idx, D, row_div=deg),
        "max_bwd": lambda: mk.spgemm_max_backward_x16(row_ptr, col, idx, arg, G, k),
        "mean_bwd": lambda: mk.sspmm_backward_x16(row_ptr, col, ones, G, idx, row_div=deg),
    }
    r = time_alternating(fns, iters, warmup)
    r["ratios"] = ratios(r, [("max_fwd", "mean_fwd"), ("max_fwd_noarg", "mean_fwd"),
                             ("max_bwd", "mean_bwd")])
    r["shape"] = dict(graph=name, V=row_ptr.numel() - 1, E=col.numel(), D=D, k=k)
    return r


def step_u8(name, k, D, iters, warmup, seed):
    import torch
    dev = torch.device("cuda:0")
    mk, row_ptr, col, _, vals, idx, G = problem(name, k, D, seed, dev)
    idx8 = idx.to(torch.uint8)
    out8, arg8 = mk.spgemm_max_forward(row_ptr, col, vals, idx8, D)
    out, arg = mk.spgemm_max_forward_x16(row_ptr, col, vals, idx, D)
    g8 = mk.spgemm_max_backward(row_ptr, col, idx8, arg8, G, k)
    g = mk.spgemm_max_backward_x16(row_ptr, col, idx, arg, G, k)
    fns = {
        "u8_fwd": lambda: mk.spgemm_max_forward(row_ptr, col, vals, idx8, D),
        "x16_fwd": lambda: mk.spgemm_max_forward_x16(row_ptr, col, vals, idx, D),
        "u8_bwd": lambda: mk.spgemm_max_backward(row_ptr, col, idx8, arg8, G, k),
        "x16_bwd": lambda: mk.spgemm_max_backward_x16(row_ptr, col, idx, arg, G, k),
    }
    r = time_alternating(fns, iters, warmup)
    r["ratios"] = ratios(r, [("x16_fwd", "u8_fwd"), ("x16_bwd", "u8_bwd")])
    r["same_forward_bytes"] = bool(torch.equal(out.view(torch.int32), out8.view(torch.int32))
                                   and torch.equal(arg, arg8))
    r["backward_max_abs_diff"] = float((g - g8).abs().max())
    r["shape"] = dict(graph=name, V=row_ptr.numel() - 1, E=col.numel(), D=D, k=k)
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
    r["ratios"] = ratios(r, [("torch_fwd", "max_fwd"), ("torch_step", "max_step")])
    r["peak_bytes"] = {n: peak_of(fns[n]) for n in ("torch_step", "max_step")}
    r["same_values"] = bool(torch.equal(a[has], b[has]))
    r["shape"] = dict(graph=name, V=row_ptr.numel() - 1, E=col.numel(), D=D, k=k,
                      gather_bytes=col.numel() * D * 4)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", default=STEPS)
    ap.add_argument("--step", help="run one step in this process and print its JSON (children)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27", "x16_max", "bench.json"))
    a = ap.parse_args()
    if a.step:
        kind, name, D, k = a.step.split(":")
        fn = {"mean": step_mean, "u8": step_u8, "torch": step_torch}[kind]
        print("RESULT " + json.dumps(fn(name, int(k), int(D), a.iters, a.warmup, a.seed)))
        return 0
    results = {}
    for step in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable,
               os.path.abspath(__file__), "--step", step, "--iters", str(a.iters), "--warmup",
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
    out = dict(iters=a.iters, warmup=a.warmup, seed=a.seed, steps=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))
    return 1 if any("failed" in r for r in results.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
