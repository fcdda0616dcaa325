#!/usr/bin/env python3
"""Device-event timing of the kNN search (csrc/knn.hip through dgll_amd.knn.knn_graph) at the Dynamic Graph CNN shapes

    (B, N, D, k) = (32, 1024, 3 / 64 / 128, 20), (32, 2048, 3 / 64, 40), one segment of 65 536 points at D = 3 and 64 (k = 20)

in fp32 and bf16, next to:

  (a) the torch composition it replaces, cdist + topk over a [B, N, N] array (squared, on the same card, fp32 inputs cast from the
      same points), skipped where that array does not fit the free memory;
  (b) the peak memory of both above their inputs;
  (c) one nn.EdgeConv forward + backward (D -> 64) on the graph, split into the search, graph.transpose() (a sort per dynamic graph)
      and the rest of the layer (the dense products, the segment max and their backward, the transpose already built).

    python tools/knn_bench.py [--reps 5 --rounds 1 --shapes dgcnn,wide,single --dtypes fp32,bf16]

HIP events round `reps` calls after two warm-up calls, one process on the card; the median of `rounds` is reported.  Prints a table
and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dgll_amd import knn as K  # noqa: E402
from dgll_amd.nn.Convolution import EdgeConv  # noqa: E402

SHAPES = {"dgcnn": [(32, 1024, 3, 20), (32, 1024, 64, 20), (32, 1024, 128, 20)],
          "wide": [(32, 2048, 3, 40), (32, 2048, 64, 40)],
          "single": [(1, 65536, 3, 20), (1, 65536, 64, 20)]}


def timeit(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def peak_mb(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--shapes", default="dgcnn,wide,single")
    ap.add_argument("--dtypes", default="fp32,bf16")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    med = lambda fn: statistics.median(timeit(fn, args.reps) for _ in range(args.rounds))      # noqa: E731
    result = {}
    for B, N, D, k in (s for name in args.shapes.split(",") for s in SHAPES[name]):
        for name in args.dtypes.split(","):
            dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[name]
            x = torch.randn(B, N, D, device=dev).to(dtype)
            row = {"knn ms": med(lambda: K.knn_graph(x, k)), "knn peak MB": peak_mb(lambda: K.knn_graph(x, k, return_dist=True))}
            pair_bytes = B * N * N * 4
            if name == "fp32":
                free = torch.cuda.mem_get_info(dev)[0]
                if 3 * pair_bytes > free:
                    print("  cdist + topk skipped: the [B, N, N] array is %.1f GB, %.1f GB are free" % (pair_bytes / 1e9, free / 1e9))
                else:
                    composed = lambda: torch.cdist(x, x).square_().topk(k, dim=2, largest=False)      # noqa: E731
                    row["cdist+topk ms"], row["cdist+topk peak MB"] = med(composed), peak_mb(composed)
                    torch.cuda.empty_cache()
            # one EdgeConv forward + backward on the dynamic graph: the search, the transpose (a sort), the rest
            conv = EdgeConv(D, 64).to(dev)
            h = x.reshape(-1, D).clone().requires_grad_(True)
            go = torch.randn(B * N, 64, device=dev).to(dtype)

            def transpose():
                g._transpose = None
                g.transpose()

            def layer():
                conv(g, h).backward(go)
                h.grad = None

            g = K.knn_graph(x, k)
            row["transpose ms"] = med(transpose)
            row["edgeconv fwd+bwd (graph and transpose given) ms"] = med(layer)
            label = "B%d_N%d_D%d_k%d_%s" % (B, N, D, k, name)
            print(label + ": one [B, N, N] fp32 array would be %.1f MB" % (pair_bytes / 1e6), flush=True)
            for key, v in row.items():
                print("  %-50s %10.3f" % (key, v), flush=True)
            result[label] = {key: round(v, 4) for key, v in row.items()}
            del x, h, go, g, conv
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
