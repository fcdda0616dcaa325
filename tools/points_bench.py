#!/usr/bin/env python3
"""Device-event timing of farthest point sampling (csrc/fps.hip through dgll_amd.points.fps) and of the fixed-radius search
(csrc/radius.hip through points.radius) at the PointNet++ shapes

    fps     (B, N, m) = (32, 1024, 512), (32, 4096, 1024), (1, 65536, 1024) at D = 3 and D = 32, fp32 and bf16
    radius  32 x 1024 candidates, 32 x 512 queries (an fps of them), K = 32 / 64, r with about K / 2 and about 4 K points in the ball

next to the torch compositions they replace -- for fps the loop of one cdist column, minimum and argmax per sample (3 launches and an
[N] temporary per sample, plus a gather and an index write), for radius cdist + mask + topk of the indices over a [B, M, N] array -- to knn_graph at k = K on the same
points, the peak memory of each above its inputs, and one nn.SetAbstraction forward + backward split into its three parts.

    python tools/points_bench.py [--reps 5 --rounds 1 --parts fps,radius,sa --dtypes fp32,bf16]

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

from dgll_amd import knn, points as P  # noqa: E402
from dgll_amd.nn.Convolution import PointNetConv  # noqa: E402
from tools.knn_bench import peak_mb, timeit  # noqa: E402

FPS_SHAPES = [(32, 1024, 512), (32, 4096, 1024), (1, 65536, 1024)]


def torch_fps(x, m):
    """the composition: x [B, N, D] -> [B, m] offsets; per sample one cdist column, a minimum and an argmax, plus what a working loop
    cannot do without: the gather of the chosen rows and the write of the index (five launches per sample)"""
    B, N, _ = x.shape
    idx = torch.zeros(B, m, dtype=torch.int64, device=x.device)
    dmin = torch.full((B, N), float("inf"), device=x.device)
    cur = torch.zeros(B, dtype=torch.int64, device=x.device)
    rows = torch.arange(B, device=x.device)
    for t in range(1, m):
        dmin = torch.minimum(dmin, torch.cdist(x, x[rows, cur].unsqueeze(1)).squeeze(2).square_())
        cur = dmin.argmax(1)
        idx[:, t] = cur
    return idx


def torch_radius(x, y, r, K):
    """the composition: x [B, N, D], y [B, M, D] -> the first K indices within r per query ([B, M, K], N where there are fewer)"""
    N = x.shape[1]
    inside = torch.cdist(y, x) <= r
    ids = torch.where(inside, torch.arange(N, device=x.device), N)
    return ids.topk(K, dim=2, largest=False).values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--parts", default="fps,radius,sa")
    ap.add_argument("--dtypes", default="fp32,bf16")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    med = lambda fn: statistics.median(timeit(fn, args.reps) for _ in range(args.rounds))      # noqa: E731
    dtypes = [(name, {"bf16": torch.bfloat16, "fp32": torch.float32}[name]) for name in args.dtypes.split(",")]
    result = {}

    def report(label, row):
        print(label, flush=True)
        for key, v in row.items():
            print("  %-50s %10.3f" % (key, v), flush=True)
        result[label] = {key: round(v, 4) for key, v in row.items()}

    parts = args.parts.split(",")
    if "fps" in parts:
        for B, N, m in FPS_SHAPES:
            for D in (3, 32):
                for name, dtype in dtypes:
                    x = torch.rand(B, N, D, device=dev).to(dtype)
                    row = {"fps ms": med(lambda: P.fps(x, npoints=m)), "fps peak MB": peak_mb(lambda: P.fps(x, npoints=m, return_dmin=True))}
                    if name == "fp32":
                        row["torch loop ms"] = med(lambda: torch_fps(x, m))
                        row["torch loop peak MB"] = peak_mb(lambda: torch_fps(x, m))
                    report("fps_B%d_N%d_m%d_D%d_%s" % (B, N, m, D, name), row)
    if "radius" in parts or "sa" in parts:
        B, N, M = 32, 1024, 512
        x = torch.rand(B, N, 3, device=dev)
        centres = x.reshape(-1, 3)[P.fps(x, npoints=M)]
        for K in (32, 64):
            for fill, inside in (("half", K / 2), ("4x", 4 * K)):
                r = (inside / N * 3 / (4 * 3.14159265)) ** (1.0 / 3)            # a ball of volume inside / N in the unit cube
                for name, dtype in dtypes:
                    xs, ys = x.reshape(-1, 3).to(dtype), centres.to(dtype)
                    search = lambda: P.radius(xs, ys, r, [N] * B, [M] * B, max_num_neighbors=K)      # noqa: E731
                    g = search()
                    row = {"mean degree": g.col.numel() / (B * M), "radius ms": med(search),
                           "radius peak MB": peak_mb(lambda: P.radius(xs, ys, r, [N] * B, [M] * B, max_num_neighbors=K, return_dist=True)),
                           "knn_graph k = K on the candidates ms": med(lambda: knn.knn_graph(xs, K, [N] * B))}
                    if name == "fp32" and "radius" in parts:
                        composed = lambda: torch_radius(x, centres.view(B, M, 3), r, K)      # noqa: E731
                        row["cdist+mask+topk ms"], row["cdist+mask+topk peak MB"] = med(composed), peak_mb(composed)
                    if "radius" in parts:
                        report("radius_K%d_%s_%s" % (K, fill, name), row)
        if "sa" in parts:
            for name, dtype in dtypes:
                pos = x.reshape(-1, 3).to(dtype)
                feats = torch.randn(B * N, 64, device=dev).to(dtype).requires_grad_(True)
                conv = PointNetConv(torch.nn.Sequential(torch.nn.Linear(67, 128), torch.nn.ReLU())).to(dev)
                idx = P.fps(pos, [N] * B, ratio=0.5)
                graph = P.radius(pos, pos[idx], 0.2, [N] * B, idx.seg_sizes, max_num_neighbors=32)
                go = torch.randn(graph.n_rows, 128, device=dev).to(dtype)

                def layer():
                    conv(graph, feats, (pos, pos[idx])).backward(go)
                    feats.grad = None

                report("set_abstraction_B32_N1024_ratio0.5_r0.2_K32_C64_F128_%s" % name,
                       {"fps ms": med(lambda: P.fps(pos, [N] * B, ratio=0.5)),
                        "radius ms": med(lambda: P.radius(pos, pos[idx], 0.2, [N] * B, idx.seg_sizes, max_num_neighbors=32)),
                        "pointnetconv fwd+bwd (graph given) ms": med(layer), "mean degree": graph.col.numel() / graph.n_rows})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
