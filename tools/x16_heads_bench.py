#!/usr/bin/env python3
"""The multi-head 16-bit-selector kernels (x16_heads.hip) per op, against what a user has
without them.

One step per (graph, D, k, H), each a child process of its own under `timeout`, one at a time (at
most one process has the GPU open), so a step that faults or hangs ends the run instead of being
followed by more work on the same card.  GRAPH is a preset of maxk_graph (reddit).  The divisor is
the in-degree; weights and gradients are random.

In one process, after warm-up, with device events, alternating within every iteration:
  heads_fwd   mk.spgemm_forward_heads_x16          calls_fwd  H mk.spgemm_forward_x16 calls
  heads_bwd   mk.sspmm_backward_heads_x16          calls_bwd  H mk.sspmm_backward_x16 calls, added
  heads_edge  mk.edge_weight_grad_heads_x16
  gat_step    forward + backward of MaxKMultiHeadGATConv(D, 8, H) on MaxK features (time only: the
              torch formulation of the step needs an [H, E, D] intermediate, 234 GB Reddit-sized
              at H = 1, and is not measured)
and, `--torch-iters` times, torch_edge: the edge gradient on the masked dense features, per head
(X[col] * G[h][rows]).sum(-1) / deg[rows] in slices of 2^20 edges (the whole [E, D] gather does
not fit).

Reports medians, min, max, the spread (max - min) / median over the iterations and the ratios.
Writes one JSON file and prints it.

  python tools/x16_heads_bench.py [--steps reddit:512:32:1,reddit:512:32:4,reddit:512:32:8]
                                  [--iters 10] [--warmup 2] [--torch-iters 2]
                                  [--step-timeout 400] [--out profiles/r28/x16_heads/bench.json]
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

STEPS = "reddit:512:32:1,reddit:512:32:4,reddit:512:32:8"


def step(name, D, k, H, iters, warmup, torch_iters, seed):
    import torch

    import bench  # the graph generators, as bench.py uses them
    import maxk_cuda_kernels as mk
    import maxk_layers as ML
    dev = torch.device("cuda:0")
    row_ptr, col = bench.maxk_graph.synthetic_graph(name, seed, dev)
    V, E = row_ptr.numel() - 1, col.numel()
    gen = torch.Generator(device=dev).manual_seed(123)
    x = torch.randn(V, D, generator=gen, device=dev)
    G = torch.randn(H, V, D, generator=gen, device=dev)
    w = torch.rand(H, E, generator=gen, device=dev)
    deg = torch.diff(row_ptr).float().clamp(min=1.0)
    dense, vals, idx = mk.topk_cbsr_dense_x16(x, k)
    mk.transpose_plan(col, V)  # cached: the backwards' plan
    graph = ML.CSRGraph(row_ptr, col)
    layer = ML.MaxKMultiHeadGATConv(D, 8, H).to(dev)
    rows = graph.edge_rows()

    def calls_fwd():
        out = torch.empty(H, V, D, device=dev)
        for h in range(H):
            mk.spgemm_forward_x16(row_ptr, col, w[h], vals, idx, D, row_div=deg, out=out[h])
        return out

    def calls_bwd():
        acc = mk.sspmm_backward_x16(row_ptr, col, w[0], G[0], idx, row_div=deg)
        for h in range(1, H):
            acc.add_(mk.sspmm_backward_x16(row_ptr, col, w[h], G[h], idx, row_div=deg))
        return acc

    def torch_edge():
        out = torch.empty(H, E, device=dev)
        for e0 in range(0, E, 1 << 20):
            e = slice(e0, min(E, e0 + (1 << 20)))
            xe, r = dense[col[e].long()], rows[e]
            for h in range(H):
                out[h, e] = (xe * G[h][r]).sum(-1) / deg[r]
        return out

    def gat_step():
        xs, tv, ti = ML.maxk(x.requires_grad_(True), k)
        layer(graph, xs, tv, ti).sum().backward()

    fns = {
        "heads_fwd": lambda: mk.spgemm_forward_heads_x16(row_ptr, col, w, vals, idx, D,
                                                         row_div=deg),
        "calls_fwd": calls_fwd,
        "heads_bwd": lambda: mk.sspmm_backward_heads_x16(row_ptr, col, w, G, idx, row_div=deg),
        "calls_bwd": calls_bwd,
        "heads_edge": lambda: mk.edge_weight_grad_heads_x16(row_ptr, col, vals, idx, G,
                                                            row_div=deg),
        "gat_step": gat_step,
    }
    agree = dict(
        fwd=bool(torch.allclose(fns["heads_fwd"](), calls_fwd(), rtol=1e-4, atol=1e-4)),
        bwd=bool(torch.allclose(fns["heads_bwd"](), calls_bwd(), rtol=1e-4, atol=1e-3)))
    if torch_iters > 0:
        agree["edge"] = bool(torch.allclose(fns["heads_edge"](), torch_edge(), rtol=1e-4,
                                            atol=1e-4))
    r = time_alternating(fns, iters, warmup)
    pairs = [("heads_fwd", "calls_fwd"), ("heads_bwd", "calls_bwd")]
    if torch_iters > 0:
        r.update(time_alternating({"torch_edge": torch_edge}, torch_iters, 1))
        pairs.append(("heads_edge", "torch_edge"))
    m = {n: r[n]["median_ms"] for n in r}
    r["ratios"] = {f"{a}/{b}": round(m[a] / m[b], 3) for a, b in pairs}
    r["shape"] = dict(graph=name, V=V, E=E, D=D, k=k, H=H, outputs_agree=agree)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", default=STEPS)
    ap.add_argument("--step", help="run one step in this process and print its JSON (children)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-iters", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "r28", "x16_heads", "bench.json"))
    a = ap.parse_args()
    if a.step:
        name, D, k, H = a.step.split(":")
        print("RESULT " + json.dumps(step(name, int(D), int(k), int(H), a.iters, a.warmup,
                                          a.torch_iters, a.seed)))
        return 0
    results = {}
    for s in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
               "--step", s, "--iters", str(a.iters), "--warmup", str(a.warmup), "--torch-iters",
               str(a.torch_iters), "--seed", str(a.seed)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            # a fault, an abort or a time limit: nothing more is started on the GPU
            results[s] = dict(failed=p.returncode, stderr=p.stderr[-2000:])
            print(f"{s}: exit status {p.returncode}; stopping", file=sys.stderr)
            break
        results[s] = json.loads(lines[-1][len("RESULT "):])
        print(s, json.dumps(results[s].get("ratios")), flush=True)
    out = dict(iters=a.iters, warmup=a.warmup, torch_iters=a.torch_iters, seed=a.seed,
               steps=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))
    return 1 if any("failed" in r for r in results.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
