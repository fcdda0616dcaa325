#!/usr/bin/env python3
"""Per-pass timing of the three multi-aggregator passes (csrc/multi_agg.hip: FORWARD, ROWS, COLS) at F = 64 and 256, bf16 and fp32,
with the default four aggregators (mean, max, min, std) and three scalers, next to what the engine offered for the same numbers
before: ops.spmm of x, ops.spmm of x^2 and two ops.segment_max (of x and of -x) forward; their four backwards (two spmm over A^T, two
segment_max_bwd).  The composition's element-wise work (squaring, negating, the scalers, the concatenation into 12 blocks) is NOT
timed: it only counts launches that sweep the adjacency, which favours the composition.

    python tools/pna_bench.py --graph reddit|products [--reps 5 --rounds 3 --widths 64,256 --dtypes bf16,fp32]

Synthetic graphs (reddit-shaped: 232 965 nodes, 57.3 M undirected edges; products-shaped: synth.products_like_graph defaults), with
self-loops.  HIP events round `reps` launches after two warm-up launches, one process on the card; the fused passes and the
composition are timed alternately, `rounds` times, and the median is reported.  Prints a table and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dgll_amd import ops, ops_agg, synth  # noqa: E402

GRAPHS = {"products": dict(), "reddit": dict(n=232_965, n_undirected=57_300_000)}
AGGS = tuple(ops_agg.AGGREGATORS[a] for a in ("mean", "max", "min", "std"))
SCALERS = tuple(ops_agg.SCALERS[s] for s in ("identity", "amplification", "attenuation"))


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
    ap.add_argument("--graph", choices=sorted(GRAPHS), default="reddit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--widths", default="64,256")
    ap.add_argument("--dtypes", default="bf16,fp32")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = synth.products_like_graph(dev, seed=0, locality=0.9, self_loops=True, **GRAPHS[args.graph])
    gt, _ = g.transpose()
    g.plan(), gt.plan()
    n = g.n_rows
    delta = ops_agg.pna_delta(g)
    print("%s-shaped graph: %d nodes, %d entries, delta %.4f" % (args.graph, n, g.nnz, delta), flush=True)
    result = {"graph": args.graph, "nodes": n, "nnz": g.nnz, "shapes": {}}
    torch.manual_seed(0)
    for name in args.dtypes.split(","):
        dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[name]
        for F in (int(w) for w in args.widths.split(",")):
            x = torch.randn(n, F, device=dev).to(dtype)
            y = torch.randn(n, F, device=dev).to(dtype)
            go = torch.randn(n, len(AGGS) * len(SCALERS) * F, device=dev).to(dtype)
            gf = go[:, :F].contiguous()
            _, stats, arg = ops_agg.forward_raw(g, x, y, AGGS, SCALERS, delta, want_stats=True, want_arg=True)
            coef, _ = ops_agg.rows_raw(g, go, stats, AGGS, SCALERS, delta)
            xs = x.clone().requires_grad_()
            top = ops.segment_max(g, xs)
            fused = {"forward": lambda: ops_agg.forward_raw(g, x, y, AGGS, SCALERS, delta, want_stats=True, want_arg=True),
                     "rows": lambda: ops_agg.rows_raw(g, go, stats, AGGS, SCALERS, delta),
                     "cols": lambda: ops_agg.cols_raw(g, x, coef, arg, AGGS, SCALERS, delta)}
            parts = {"spmm": lambda: ops.spmm_raw(g, x, reduce="mean"),
                     "segment_max": lambda: ops.segment_max(g, x),
                     "spmm_bwd": lambda: ops.spmm_raw(gt, gf, reduce="sum"),
                     "segment_max_bwd": lambda: torch.autograd.grad(top, xs, gf, retain_graph=True)}
            samples = {k: [] for k in list(fused) + list(parts)}
            for _ in range(args.rounds):            # alternating: fused, composition, fused, ...
                for table in (fused, parts):
                    for key, fn in table.items():
                        samples[key].append(timeit(fn, args.reps))
            row = {k: statistics.median(v) for k, v in samples.items()}
            row["composed_forward"] = 2 * row["spmm"] + 2 * row["segment_max"]
            row["composed_backward"] = 2 * row["spmm_bwd"] + 2 * row["segment_max_bwd"]
            row["fused_backward"] = row["rows"] + row["cols"]
            print("F = %d %s" % (F, name), flush=True)
            for key, ms in row.items():
                print("  %-18s %9.3f ms" % (key, ms), flush=True)
            result["shapes"]["%s_F%d" % (name, F)] = {k: round(ms, 4) for k, ms in row.items()}
            del x, y, go, gf, stats, arg, coef, xs, top, fused, parts
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
