#!/usr/bin/env python3
"""GAT edge softmax against the aggregation it feeds and the PyTorch composition it replaces.

Per workload (Reddit-sized and products-sized; bench.py's synthetic graphs), in one process,
after warm-up, with device events, alternating so every op sees the same clocks and cache state:

  aggregate    mk.spgemm_forward at D = 256 and the workload's k -- the yardstick, a kernel the
               softmax does not change
  softmax_fwd  mk.gat_edge_softmax           (scores -> weights)
  softmax_bwd  mk.gat_edge_softmax_backward  (weights, their gradient -> score gradients)
  composition  the same function in PyTorch on the CSR: repeat_interleave row ids (built once,
               outside the timing), two gathers, leaky_relu, scatter_reduce(amax), exp,
               index_add_, a division -- forward, then its autograd backward

and the byte model of DESIGN.md 5.6.  Writes one JSON file (default
profiles/r10/edge_softmax/bench.json) and prints it.

  python tools/edge_softmax_bench.py [--graphs reddit:16,products:32] [--iters 20] [--out FILE]
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

SLOPE = 0.2


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


def composition(rows, col, s_dst, s_src, num_rows):
    """The edge softmax a user writes without the kernel; returns w with its autograd graph."""
    l = torch.nn.functional.leaky_relu(s_dst[rows] + s_src[col], SLOPE)
    m = torch.zeros(num_rows, device=l.device).scatter_reduce(0, rows, l.detach(), "amax",
                                                              include_self=False)
    p = torch.exp(l - m[rows])
    s = torch.zeros(num_rows, device=l.device).index_add_(0, rows, p)
    return p / s[rows]


def run(name, k, D, iters, comp_iters, warmup, seed, dev):
    mg = bench.maxk_graph
    V = mg.PRESETS[name]["V"]
    row_ptr, col = mg.synthetic_graph(name, seed, dev)
    E = col.numel()
    gen = torch.Generator(device=dev).manual_seed(123)
    val = torch.rand(E, generator=gen, device=dev)
    X = torch.rand(V, D, generator=gen, device=dev)
    s_dst = torch.randn(V, generator=gen, device=dev)
    s_src = torch.randn(V, generator=gen, device=dev)
    gw = torch.randn(E, generator=gen, device=dev)
    cv, ci = mk.topk_cbsr(X, k)
    del X
    y = torch.empty(V, D, device=dev)
    w = torch.empty(E, device=dev)
    g_dst, g_src = torch.empty(V, device=dev), torch.empty(V, device=dev)

    def agg():
        mk.spgemm_forward(row_ptr, col, val, cv, ci, D, out=y, validate=False)

    def fwd():
        mk.gat_edge_softmax(row_ptr, col, s_dst, s_src, SLOPE, out=w, validate=False)

    def bwd():
        mk.gat_edge_softmax_backward(row_ptr, col, s_dst, s_src, w, gw, SLOPE,
                                     out=(g_dst, g_src), validate=False)

    mk.spgemm_forward(row_ptr, col, val, cv, ci, D, out=y, validate=True)
    mk.transpose_plan(col, V)  # once per graph, as the csc backward's
    for _ in range(warmup):
        agg()
        fwd()
        bwd()
    torch.cuda.synchronize()
    t_a, t_f, t_b = [], [], []
    for _ in range(iters):
        t_a.append(timed(agg))
        t_f.append(timed(fwd))
        t_b.append(timed(bwd))

    a, f, b = summary(t_a), summary(t_f), summary(t_b)
    res = dict(graph=name, V=V, E=E, D=D, k=k, aggregate=a, softmax_fwd=f, softmax_bwd=b,
               fwd_to_aggregate=round(f["median_ms"] / a["median_ms"], 4),
               bwd_to_aggregate=round(b["median_ms"] / a["median_ms"], 4))
    if comp_iters > 0:  # the composition on the same inputs; its results are compared too
        rows = torch.repeat_interleave(torch.arange(V, device=dev), torch.diff(row_ptr).long())
        col64 = col.long()
        sd = s_dst.clone().requires_grad_(True)
        ss = s_src.clone().requires_grad_(True)
        t_cf, t_cb = [], []
        wc = None
        for i in range(comp_iters + 1):
            sd.grad = ss.grad = None
            box = []
            tf = timed(lambda: box.append(composition(rows, col64, sd, ss, V)))
            wc = box[0]
            tb = timed(lambda: wc.backward(gw))
            if i:  # the first pass warms the allocator
                t_cf.append(tf)
                t_cb.append(tb)
        has = torch.diff(row_ptr)[rows] > 0
        cf, cb = summary(t_cf), summary(t_cb)
        res.update(composition_fwd=cf, composition_bwd=cb,
                   composition_to_fused=round((cf["median_ms"] + cb["median_ms"])
                                              / (f["median_ms"] + b["median_ms"]), 2),
                   max_abs_diff_to_composition=dict(
                       w=float((wc.detach() - w)[has].abs().max()),
                       grad_s_dst=float((sd.grad - g_dst).abs().max()),
                       grad_s_src=float((ss.grad - g_src).abs().max())))
        del wc, rows, col64
    # DRAM bytes of DESIGN.md 5.6: forward col_idx in, w out; backward w, grad_w and col_idx in,
    # gz out, then csc_eid in and one 64-B sector per gz gathered through it.  The score
    # gathers, the staged logits' rereads and the per-item partials are left to the caches.
    b_fwd = 4 * (V + 1) + 8 * E + 8 * V
    b_bwd = 8 * (V + 1) + 16 * E + 4 * E + 64 * E + 16 * V
    res.update(model_bytes=dict(fwd=b_fwd, bwd=b_bwd),
               model_gbs=dict(fwd=round(b_fwd / f["median_ms"] / 1e6, 1),
                              bwd=round(b_bwd / b["median_ms"] / 1e6, 1)))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--graphs", default="reddit:16,products:32")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--comp-iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "edge_softmax",
                                                  "bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup,
               build_config=mk._lib().maxk_build_config().decode(), workloads=[])
    for spec in args.graphs.split(","):
        name, k = spec.split(":")
        r = run(name, int(k), args.dim, args.iters, args.comp_iters, args.warmup, args.seed, dev)
        print(json.dumps(r), flush=True)
        res["workloads"].append(r)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
