#!/usr/bin/env python3
"""The 16-bit-selector path (D up to 1024) per op, against the two things a user has without it.

One step per (graph, D, k), each a child process of its own under `timeout`, one at a time (at
most one process has the GPU open), so a step that faults or hangs ends the run instead of being
followed by more work on the same card.  GRAPH is `yelp` (a synthetic graph of Yelp's size,
V = 716,847, E ~ 13.95 M, built by maxk_graph.make_graph) or a preset of maxk_graph (reddit).
Edge weights are 1 and the divisor is the in-degree (the SAGE mean); the graphs are symmetric, so
the transposed dense product is the same rocSPARSE plan.

In one process, after warm-up, with device events, alternating within every iteration:
  x16_encode   mk.topk_cbsr_dense_x16 at D            x16_fwd   mk.spgemm_forward_x16
  x16_bwd      mk.sspmm_backward_x16 (two-phase csc)
  dense_encode torch.topk + scatter_ at D (the masked dense features)
  dense_fwd    mk.DenseSpMMPlan.run on the masked dense features [V, D] (rocSPARSE; the plan is
               built once, outside the timing); dense_bwd is the same product on grad_out
  u8_encode / u8_fwd / u8_bwd / u8_bwd_csc   the u8 path at D = 256 on the same graph and k:
               mk.topk_cbsr_dense, mk.spgemm_forward, mk.sspmm_backward in the mode the library
               picks and forced to "csc" (the x16 backward's own form)

Reports medians, min, max, the spread (max - min) / median over the iterations and the ratios.
Writes one JSON file and prints it.

  python tools/x16_bench.py [--steps yelp:384:8,yelp:384:16,yelp:384:32,yelp:384:64,reddit:512:32,reddit:1024:32]
                            [--iters 10] [--warmup 2] [--step-timeout 240]
                            [--out profiles/r26/x16/bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from max_bench import time_alternating  # noqa: E402  (the timing loop, as the other benches)

STEPS = "yelp:384:8,yelp:384:16,yelp:384:32,yelp:384:64,reddit:512:32,reddit:1024:32"
YELP = dict(V=716_847, E=13_954_819, alpha=0.8, i0=100)


def step(name, D, k, iters, warmup, seed):
    import torch

    import bench  # the graph generators, as bench.py uses them
    import maxk_cuda_kernels as mk
    dev = torch.device("cuda:0")
    if name == "yelp":
        E = YELP["E"] - ((YELP["E"] - YELP["V"]) % 2)
        row_ptr, col = bench.maxk_graph.make_graph(YELP["V"], E, YELP["alpha"], YELP["i0"], seed,
                                                   dev)
    else:
        row_ptr, col = bench.maxk_graph.synthetic_graph(name, seed, dev)
    V, E = row_ptr.numel() - 1, col.numel()
    gen = torch.Generator(device=dev).manual_seed(123)
    x = torch.randn(V, D, generator=gen, device=dev)
    G = torch.randn(V, D, generator=gen, device=dev)
    x8, G8 = x[:, :256].contiguous(), G[:, :256].contiguous()
    ones = torch.ones(E, device=dev)
    deg = torch.diff(row_ptr).float().clamp(min=1.0)
    dense, vals, idx = mk.topk_cbsr_dense_x16(x, k)
    _, vals8, idx8 = mk.topk_cbsr_dense(x8, k)
    plan = mk.DenseSpMMPlan(row_ptr, col, ones, dense)
    plan_g = mk.DenseSpMMPlan(row_ptr, col, ones, G)
    mk.transpose_plan(col, V)  # cached: the backwards' plan
    auto = mk.sspmm_backward(row_ptr, col, ones, G8, idx8, row_div=deg)  # builds its plan
    csc = mk.sspmm_backward(row_ptr, col, ones, G8, idx8, row_div=deg, mode="csc")
    same = bool(torch.allclose(auto, csc, rtol=1e-4, atol=1e-4))

    def dense_encode():
        tv, ti = torch.topk(x, k, dim=1)
        return torch.zeros_like(x).scatter_(1, ti, tv)

    fns = {
        "x16_encode": lambda: mk.topk_cbsr_dense_x16(x, k),
        "x16_fwd": lambda: mk.spgemm_forward_x16(row_ptr, col, ones, vals, idx, D, row_div=deg),
        "x16_bwd": lambda: mk.sspmm_backward_x16(row_ptr, col, ones, G, idx, row_div=deg),
        "dense_encode": dense_encode,
        "dense_fwd": plan.run,
        "dense_bwd": plan_g.run,
        "u8_encode": lambda: mk.topk_cbsr_dense(x8, k),
        "u8_fwd": lambda: mk.spgemm_forward(row_ptr, col, ones, vals8, idx8, 256, row_div=deg),
        "u8_bwd": lambda: mk.sspmm_backward(row_ptr, col, ones, G8, idx8, row_div=deg),
        "u8_bwd_csc": lambda: mk.sspmm_backward(row_ptr, col, ones, G8, idx8, row_div=deg,
                                                mode="csc"),
    }
    r = time_alternating(fns, iters, warmup)
    m = {n: r[n]["median_ms"] for n in r}
    r["ratios"] = {f"{a}/{b}": round(m[a] / m[b], 3) for a, b in (
        ("dense_encode", "x16_encode"), ("dense_fwd", "x16_fwd"), ("dense_bwd", "x16_bwd"),
        ("x16_encode", "u8_encode"), ("x16_fwd", "u8_fwd"), ("x16_bwd", "u8_bwd"),
        ("x16_bwd", "u8_bwd_csc"))}
    r["shape"] = dict(graph=name, V=V, E=E, D=D, k=k, u8_modes_agree=same)
    plan.close()
    plan_g.close()
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", default=STEPS)
    ap.add_argument("--step", help="run one step in this process and print its JSON (children)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26", "x16", "bench.json"))
    a = ap.parse_args()
    if a.step:
        name, D, k = a.step.split(":")
        print("RESULT " + json.dumps(step(name, int(D), int(k), a.iters, a.warmup, a.seed)))
        return 0
    results = {}
    for s in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
               "--step", s, "--iters", str(a.iters), "--warmup", str(a.warmup), "--seed",
               str(a.seed)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            # a fault, an abort or a time limit: nothing more is started on the GPU
            results[s] = dict(failed=p.returncode, stderr=p.stderr[-2000:])
            print(f"{s}: exit status {p.returncode}; stopping", file=sys.stderr)
            break
        results[s] = json.loads(lines[-1][len("RESULT "):])
        print(s, json.dumps(results[s].get("ratios")), flush=True)
    out = dict(iters=a.iters, warmup=a.warmup, seed=a.seed, steps=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))
    return 1 if any("failed" in r for r in results.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
