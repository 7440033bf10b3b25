#!/usr/bin/env python3
"""Times the fused linear + MaxK forward against exactly what it replaces, in one process.

  fused      mk.linear_maxk_forward(x, W, b, k=k)
  two_step   torch.addmm(b, x, W.t()) then the encode (mk.topk_cbsr, or the same C entry of
             --parent-lib: the parent commit's libmaxk_hip.so)
  addmm / encode / encode_parent   the parts, the last two being the encode's before / after

at V = 232,965 and 2,449,029, (I, D) = (256, 256), (602, 256), (100, 256), k = 8, 16, 32, 64,
callables alternating inside every iteration (device events, medians, min / max as the spread),
and the peak memory (torch.cuda.max_memory_allocated over the call) of both.  --epochs times the
MaxKGCN training epoch with and without fused_linear_maxk instead (maxk_train_bench).

  python tools/linear_maxk_bench.py [--parent-lib PATH] [--sizes reddit,products] [--iters 20]
                                    [--warmup 3] [--out profiles/r25/linear_maxk/forward.json]
  python tools/linear_maxk_bench.py --epochs [--out profiles/r25/linear_maxk/epochs.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from max_bench import peak_of, time_alternating  # noqa: E402

SIZES = {"reddit": 232965, "products": 2449029}
DIMS = ((256, 256), (602, 256), (100, 256))
KS = (8, 16, 32, 64)


def parent_encode(path):
    """topk_cbsr(h, k) through maxk_topk_cbsr of another build of the library."""
    import torch
    lib = ctypes.CDLL(path)
    p, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    lib.maxk_topk_cbsr.argtypes = [p, i64, p, p, p, i64, i32, i32, p]

    def encode(h, k):
        V, D = h.shape
        val = torch.empty(V, k, dtype=torch.float32, device=h.device)
        idx = torch.empty(V, k, dtype=torch.uint8, device=h.device)
        rc = lib.maxk_topk_cbsr(h.data_ptr(), h.stride(0), val.data_ptr(), idx.data_ptr(), None,
                                V, D, k, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return val, idx
    return encode


def forward(a):
    import torch

    import bench  # noqa: F401  (puts the package on sys.path)
    import maxk_cuda_kernels as mk
    dev = torch.device("cuda:0")
    enc_parent = parent_encode(a.parent_lib) if a.parent_lib else None
    points = []
    for size in a.sizes.split(","):
        V = SIZES[size]
        for I, D in DIMS:
            gen = torch.Generator(device=dev).manual_seed(123)
            x = torch.randn(V, I, generator=gen, device=dev)
            W = torch.randn(D, I, generator=gen, device=dev) / I ** 0.5
            b = torch.randn(D, generator=gen, device=dev)
            h = torch.addmm(b, x, W.t())
            for k in KS:
                enc = enc_parent or mk.topk_cbsr
                fns = {"fused": lambda: mk.linear_maxk_forward(x, W, b, k=k),
                       "two_step": lambda: enc(torch.addmm(b, x, W.t()), k),
                       "addmm": lambda: torch.addmm(b, x, W.t()),
                       "encode": lambda: mk.topk_cbsr(h, k)}
                if enc_parent:
                    fns["encode_parent"] = lambda: enc_parent(h, k)
                (fv, fi), (tv, ti) = fns["fused"](), fns["two_step"]()
                r = time_alternating(fns, a.iters, a.warmup)
                if enc_parent and I == DIMS[0][0]:  # the encode alone, in both orders: a call
                    r["encode_abba"] = time_alternating(  # right after one on the same h gains
                        {"parent_1": fns["encode_parent"], "new_2": fns["encode"],
                         "new_3": fns["encode"], "parent_4": fns["encode_parent"]},
                        a.iters, a.warmup)
                r["shape"] = dict(size=size, V=V, I=I, D=D, k=k)
                r["two_step_over_fused"] = round(r["two_step"]["median_ms"] /
                                                 r["fused"]["median_ms"], 3)
                r["rows_with_other_winners"] = int((fi != ti).any(1).sum())
                r["max_abs_value_difference"] = float((fv - tv).abs().max())
                r["peak_bytes"] = {n: peak_of(fns[n]) for n in ("fused", "two_step")}
                r["bad_rows"] = mk.topk_error_rows()
                points.append(r)
                print(json.dumps({**r["shape"], "fused_ms": r["fused"]["median_ms"],
                                  "two_step_ms": r["two_step"]["median_ms"],
                                  "ratio": r["two_step_over_fused"]}), flush=True)
            del x, h
    return dict(iters=a.iters, warmup=a.warmup, parent_lib=bool(a.parent_lib), points=points)


def epochs(a):
    import bench  # noqa: F401
    import maxk_train_bench
    runs = []
    for size in a.sizes.split(","):
        for k in (16, 32):
            for flag in ([], ["--fused-linear-maxk"]):
                runs.append(maxk_train_bench.main(
                    [size, "--model", "gcn", "--k", str(k), "--no-library", "--epochs",
                     str(a.iters), "--warmup", str(a.warmup)] + flag))
    return dict(runs=runs)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--epochs", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--sizes", default="reddit,products")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = a.out or os.path.join(ROOT, "profiles", "r25", "linear_maxk",
                                "epochs.json" if a.epochs else "forward.json")
    res = epochs(a) if a.epochs else forward(a)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
