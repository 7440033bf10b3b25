#!/usr/bin/env python3
"""The three CBSR linear kernels against exactly the torch sequences they replace.

One step per (SIZE, K), each a child process of its own under `timeout`, one at a time, so a step
that faults or hangs ends the run.  In one process, after warm-up, with device events,
alternating within every iteration, at V = the vertex count of SIZE and D = O = --dim:

  fwd / fwd_dense      mk.cbsr_linear_forward(vals, idx, W)            x_sparse @ W^T
  gval / gval_dense    mk.cbsr_linear_backward_values(g, idx, W)       mk.topk_backward(None, g @ W, idx, D)
                       (what _Linear.backward and MaxK.backward run: the product, then the
                       gather at the selected columns written back as a dense row)
  wgrad / wgrad_dense  mk.cbsr_linear_backward_weight(g, vals, idx, D) maxk_layers._wgrad(g, x_sparse)

Reports medians, min, max, the spread over the iterations, the ratios dense / kernel (above 1:
the kernel wins), and the largest deviation of each kernel from its dense counterpart.

  python tools/cbsr_linear_bench.py [--steps reddit:8,...,products:64] [--dim 256] [--iters 20]
                                    [--warmup 3] [--out profiles/r24/cbsr_linear/bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from max_bench import time_alternating  # noqa: E402

SIZES = {"reddit": 232965, "products": 2449029}
STEPS = ",".join(f"{s}:{k}" for s in SIZES for k in (8, 16, 32, 64))


def step(size, k, D, iters, warmup):
    import torch

    import bench  # noqa: F401  (puts the package on sys.path)
    import maxk_cuda_kernels as mk
    import maxk_layers as ML
    dev = torch.device("cuda:0")
    V, O = SIZES[size], D
    gen = torch.Generator(device=dev).manual_seed(123)
    xs, vals, idx = mk.topk_cbsr_dense(torch.randn(V, D, generator=gen, device=dev), k)
    W = torch.randn(O, D, generator=gen, device=dev) / D ** 0.5
    g = torch.randn(V, O, generator=gen, device=dev)
    fns = {
        "fwd": lambda: mk.cbsr_linear_forward(vals, idx, W),
        "fwd_dense": lambda: xs @ W.t(),
        "gval": lambda: mk.cbsr_linear_backward_values(g, idx, W),
        "gval_dense": lambda: mk.topk_backward(None, g @ W, idx, D),
        "wgrad": lambda: mk.cbsr_linear_backward_weight(g, vals, idx, D),
        "wgrad_dense": lambda: ML._wgrad(g, xs),
    }
    dev_of = {}
    for n in ("fwd", "wgrad"):
        a, b = fns[n](), fns[n + "_dense"]()
        dev_of[n] = float((a - b).abs().max() / b.abs().max())
    a, b = fns["gval"](), fns["gval_dense"]().gather(1, idx.long())
    dev_of["gval"] = float((a - b).abs().max() / b.abs().max())
    r = time_alternating(fns, iters, warmup)
    r["ratios"] = {n: round(r[n + "_dense"]["median_ms"] / r[n]["median_ms"], 3)
                   for n in ("fwd", "gval", "wgrad")}
    r["max_rel_deviation"] = dev_of
    r["shape"] = dict(size=size, V=V, D=D, O=O, k=k)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", default=STEPS)
    ap.add_argument("--step", help="run one step in this process and print its JSON (children)")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "cbsr_linear",
                                                  "bench.json"))
    a = ap.parse_args()
    if a.step:
        size, k = a.step.split(":")
        print("RESULT " + json.dumps(step(size, int(k), a.dim, a.iters, a.warmup)))
        return 0
    results = {}
    for s in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable,
               os.path.abspath(__file__), "--step", s, "--dim", str(a.dim), "--iters",
               str(a.iters), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            # a fault, an abort or a time limit: nothing more is started on the GPU
            results[s] = dict(failed=p.returncode, stderr=p.stderr[-2000:])
            print(f"{s}: exit status {p.returncode}; stopping", file=sys.stderr)
            break
        results[s] = json.loads(lines[-1][len("RESULT "):])
        print(s, json.dumps(results[s]["ratios"]), flush=True)
    out = dict(dim=a.dim, iters=a.iters, warmup=a.warmup, steps=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return 1 if any("failed" in r for r in results.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
