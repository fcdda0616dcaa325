#!/usr/bin/env python3
"""Device-event timing of the selection-pooling path (csrc/seg_sort.hip through dgll_amd.ops_pool) at two shapes

    small   512 graphs of 16..256 nodes (sizes drawn once from a seed), F = 128, ratio 0.5      -- the wave / workgroup kernels
    long    one segment of 100 000 rows, F = 128, ratio 0.5                                      -- past DGLL_SEGSORT_TILE: the merge path

in fp32 and bf16, next to the torch composition it replaces, on the same card and the same inputs: PyG's top-k (scatter the scores
into a dense [B, max_n] array padded with -inf, torch.sort along the rows, mask the first ceil(ratio * size) of every row), then
x[perm] * tanh(score[perm]) with torch autograd for the backward.

    python tools/pool_bench.py [--reps 20 --rounds 3 --shapes small,long --dtypes fp32,bf16]

HIP events round `reps` calls after two warm-up calls, one process on the card, the two implementations alternating inside every round;
the median of `rounds` is reported.  Prints a table and one JSON line.
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dgll_amd import _lib, ops_pool  # noqa: E402


def sizes_of(shape):
    if shape == "long":
        return [100000]
    g = torch.Generator().manual_seed(1)
    return torch.randint(16, 257, (512,), generator=g).tolist()


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="small,long")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--feat", type=int, default=128)
    args = ap.parse_args()
    dev, ratio, F = torch.device("cuda:0"), 0.5, args.feat
    torch.manual_seed(0)
    result = {}
    for shape in args.shapes.split(","):
        sizes = sizes_of(shape)
        n, B, max_n = sum(sizes), len(sizes), max(sizes)
        sizes_t = torch.tensor(sizes, device=dev)
        ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        ptr[1:] = sizes_t.cumsum(0)
        batch = torch.repeat_interleave(torch.arange(B, device=dev), sizes_t)
        keep = torch.tensor([math.ceil(ratio * s) for s in sizes], device=dev)
        for name in args.dtypes.split(","):
            dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[name]
            x = torch.randn(n, F, device=dev).to(dtype).requires_grad_(True)
            score = torch.randn(n, device=dev).to(dtype).requires_grad_(True)
            go = torch.randn(int(keep.sum()), F, device=dev).to(dtype)

            def torch_topk():
                dense = torch.full((B * max_n,), float("-inf"), dtype=score.dtype, device=dev)
                dense[torch.arange(n, device=dev) - ptr[batch] + batch * max_n] = score.detach()
                perm = dense.view(B, max_n).sort(dim=-1, descending=True)[1] + ptr[:-1].view(-1, 1)
                return perm.view(-1)[(torch.arange(max_n, device=dev).view(1, -1) < keep.view(-1, 1)).view(-1)]

            def torch_step():
                perm = torch_topk()
                (x[perm] * torch.tanh(score[perm]).unsqueeze(-1)).backward(go)
                x.grad = score.grad = None

            def hip_step():
                perm, inv = ops_pool.segment_topk(score, sizes, ratio=ratio, return_inverse=True)
                ops_pool.select(x, score, perm, inv, act="tanh").backward(go)
                x.grad = score.grad = None

            cases = {"hip segment_topk ms": lambda: ops_pool.segment_topk(score, sizes, ratio=ratio, return_inverse=True),
                     "torch pad+sort+mask ms": torch_topk, "hip topk+select fwd+bwd ms": hip_step, "torch topk+select fwd+bwd ms": torch_step}
            rounds = {key: [] for key in cases}
            for _ in range(args.rounds):                       # alternating: the same round sees the same neighbours on the card
                for key, fn in cases.items():
                    rounds[key].append(timeit(fn, args.reps))
            row = {key: statistics.median(v) for key, v in rounds.items()}
            with _lib.LaunchTimer() as timer:                   # events round the three entry points alone, inside the whole step
                for _ in range(args.reps):
                    hip_step()
            for tag, (_, avg) in timer.summary().items():
                row["  of which %s ms" % tag[0]] = avg
                rounds["  of which %s ms" % tag[0]] = [avg]
            same = torch.equal(ops_pool.segment_topk(score, sizes, ratio=ratio).as_subclass(torch.Tensor), torch_topk())
            label = "%s_B%d_n%d_F%d_%s" % (shape, B, n, F, name)
            print(label + ": max segment %d, %d rows kept, same perm as torch: %s" % (max_n, int(keep.sum()), same), flush=True)
            for key, v in row.items():
                print("  %-40s %10.4f   (rounds: %s)" % (key, v, " ".join("%.4f" % t for t in rounds[key])), flush=True)
            result[label] = {key: round(v, 4) for key, v in row.items()}
            del x, score, go
    print(json.dumps(result))


if __name__ == "__main__":
    main()
