#!/usr/bin/env python3
"""ms and peak memory of the grouped products (dgll_amd.ops_segmm) on one MI355X:

    python tools/segment_mm_bench.py [--quick] [--repeats 7] [--out FILE.json]

For (M, K, N) = (2^20, 128, 128) and (2^20, 256, 256), bf16 and fp32, R in {4, 64, 1024}, equal and Zipf-skewed segment lengths, rows
sorted by type (segment_mm) and unsorted (gather_mm's path: device sort + row index): the forward, grad_a and grad_b, each timed on its
own with device events -- warm-up launches first, then `--repeats` timed runs; the median, the fastest and the slowest are printed, and
the peak memory above the operands.  Next to them
  loop    a Python loop of dense.linear (and dense.input_grad / dense.grad_weight) over the segments, on rows permuted into type order
          first and put back afterwards when they are unsorted -- what a user had before these operators;
  floor   ONE dense.linear of all rows by a single matrix (and its two gradients): no grouped product can be faster.
A line where the new path is slower than the loop ends in "LOSES".
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dgll_amd import dense, ops_segmm  # noqa: E402


def timed(fn, warmup, repeats):
    """(median, min, max) ms over `repeats` runs after `warmup`, and the peak bytes above what was allocated before."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1], torch.cuda.max_memory_allocated() - before


def lengths(m, r, skew, gen):
    if not skew:
        out = torch.full((r,), m // r, dtype=torch.int64)
    else:
        w = 1.0 / torch.arange(1, r + 1, dtype=torch.float64)
        out = (w / w.sum() * m).long()[torch.randperm(r, generator=gen)]
    out[0] += m - int(out.sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="M = 2^17 and R in {4, 64} only")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    m = 1 << (17 if args.quick else 20)
    results = []
    for k, n in ((128, 128), (256, 256)):
        for dtype in (torch.bfloat16, torch.float32):
            a = torch.randn(m, k, device=dev).to(dtype)
            g = torch.randn(m, n, device=dev).to(dtype)
            w1 = torch.randn(k, n, device=dev) * 0.1
            floor = [timed(f, args.warmup, args.repeats) for f in (lambda: dense.linear(a, w1), lambda: dense.input_grad(g, w1),
                                                                   lambda: dense.grad_weight(a, g))]
            print("M=%d K=%d N=%d %s  floor (one matrix): fwd %.3f  grad_a %.3f  grad_b %.3f ms" % (
                m, k, n, str(dtype)[6:], floor[0][0], floor[1][0], floor[2][0]), flush=True)
            for r in ((4, 64) if args.quick else (4, 64, 1024)):
                b = torch.randn(r, k, n, device=dev) * 0.1
                for skew in (False, True):
                    seg = lengths(m, r, skew, gen)
                    offs = [0] + torch.cumsum(seg, 0).tolist()
                    seg_dev = seg.to(dev)
                    idx = torch.repeat_interleave(torch.arange(r), seg)[torch.randperm(m, generator=gen)].to(dev)
                    for is_sorted in (True, False):
                        if is_sorted:
                            group = lambda: (seg_dev, None)                                      # noqa: E731
                            to_sorted = from_sorted = lambda t, _p=None: t                       # noqa: E731
                        else:
                            def group():
                                ids, perm = torch.sort(idx, stable=True)
                                bounds = torch.searchsorted(ids, torch.arange(r + 1, device=dev))
                                return bounds[1:] - bounds[:-1], perm
                            to_sorted = lambda t, p: t[p]                                        # noqa: E731

                            def from_sorted(t, p):
                                out = torch.empty_like(t)
                                out[p] = t
                                return out

                        def loop(rowwise, left, right=None):
                            """The user's loop: rows into type order (unsorted only), one product per segment, rows back (row-wise results)."""
                            p = None if is_sorted else torch.sort(idx, stable=True)[1]
                            xs = to_sorted(left, p)
                            ys = None if right is None else to_sorted(right, p)
                            parts = [rowwise(xs[offs[i]:offs[i + 1]], b[i]) if right is None else
                                     dense.grad_weight(xs[offs[i]:offs[i + 1]], ys[offs[i]:offs[i + 1]]) for i in range(r) if offs[i + 1] > offs[i]]
                            return from_sorted(torch.cat(parts), p) if right is None else parts

                        new = [timed(f, args.warmup, args.repeats) for f in (
                            lambda: ops_segmm._product_raw(a, b, *group(), False),
                            lambda: ops_segmm._product_raw(g, b, *group(), True),
                            lambda: ops_segmm._gradw_raw(a, g, *group(), r))]
                        old = [timed(f, 1, max(3, args.repeats // 2)) for f in (
                            lambda: loop(dense.linear, a), lambda: loop(dense.input_grad, g), lambda: loop(None, a, g))]
                        for name, nw, ol, fl in zip(("forward", "grad_a", "grad_b"), new, old, floor):
                            results.append(dict(M=m, K=k, N=n, dtype=str(dtype)[6:], R=r, skew=skew, sorted=is_sorted, product=name,
                                                new_ms=nw[:3], new_peak_mib=nw[3] / 2 ** 20, loop_ms=ol[:3], loop_peak_mib=ol[3] / 2 ** 20,
                                                floor_ms=fl[:3]))
                            print("  R=%-4d %-5s %-8s %-7s new %.3f [%.3f, %.3f] ms %.1f MiB | loop %.3f [%.3f, %.3f] ms %.1f MiB | floor %.3f%s" % (
                                r, "zipf" if skew else "equal", "sorted" if is_sorted else "unsorted", name, nw[0], nw[1], nw[2],
                                nw[3] / 2 ** 20, ol[0], ol[1], ol[2], ol[3] / 2 ** 20, fl[0], "  LOSES" if nw[0] > ol[0] else ""), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
