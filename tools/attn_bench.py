#!/usr/bin/env python3
"""Per-pass timing of the three sparse dot-product attention passes (csrc/sparse_attn.hip) at 8 x 32 and 1 x 64 bf16, with separate
k / v and with k and v one buffer (DotGatConv: one gather per edge), next to ops.spmm at the same width and the three GATv2 passes
(csrc/gatv2.hip) on the same graph.

    python tools/attn_bench.py --graph reddit|products [--reps 10]

Synthetic graphs (reddit-shaped: 232 965 nodes, 57.3 M undirected edges; products-shaped: synth.products_like_graph defaults), with
self-loops.  HIP events round `reps` launches after two warm-up launches, one process on the card.  Prints a table and one JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dgll_amd import ops, ops_attn, ops_gatv2, synth  # noqa: E402

GRAPHS = {"products": dict(), "reddit": dict(n=232_965, n_undirected=57_300_000)}


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
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = synth.products_like_graph(dev, seed=0, locality=0.9, self_loops=True, **GRAPHS[args.graph])
    gt, _ = g.transpose()
    g.plan(), gt.plan()
    n = g.n_rows
    print("%s-shaped graph: %d nodes, %d entries" % (args.graph, n, g.nnz), flush=True)
    result = {"graph": args.graph, "nodes": n, "nnz": g.nnz, "shapes": {}}
    torch.manual_seed(0)
    for heads, D in ((8, 32), (1, 64)):
        F, scale = heads * D, D ** -0.5
        q, k, v, go = (torch.randn(n, F, device=dev).to(torch.bfloat16) for _ in range(4))
        row = {}
        row["spmm"] = timeit(lambda: ops.spmm_raw(g, v, reduce="mean"), args.reps)
        for tag, vv in (("attn", v), ("attn_kv1", k)):          # attn_kv1: k and v one buffer
            _, lse = ops_attn.sparse_attention_forward_raw(g, q, k, vv, heads, scale)
            row[tag + "_fwd"] = timeit(lambda: ops_attn.sparse_attention_forward_raw(g, q, k, vv, heads, scale), args.reps)
            rows_only = timeit(lambda: ops_attn.sparse_attention_backward_raw(g, q, k, vv, heads, scale, lse, go, need_kv=False), args.reps)
            both = timeit(lambda: ops_attn.sparse_attention_backward_raw(g, q, k, vv, heads, scale, lse, go, need_kv=True), args.reps)
            row[tag + "_rows"], row[tag + "_cols"] = rows_only, both - rows_only
        attn = torch.randn(heads, D, device=dev) / D ** 0.5
        _, lse = ops_gatv2.gatv2_forward_raw(g, k, q, attn, heads, 0.2)
        row["gatv2_fwd"] = timeit(lambda: ops_gatv2.gatv2_forward_raw(g, k, q, attn, heads, 0.2), args.reps)
        rows_only = timeit(lambda: ops_gatv2.gatv2_backward_raw(g, k, q, attn, heads, 0.2, lse, go, need_xl=False), args.reps)
        both = timeit(lambda: ops_gatv2.gatv2_backward_raw(g, k, q, attn, heads, 0.2, lse, go, need_xl=True), args.reps)
        row["gatv2_rows"], row["gatv2_cols"] = rows_only, both - rows_only
        base = row["spmm"]
        print("%d x %d bf16:" % (heads, D), flush=True)
        for name, ms in row.items():
            print("  %-14s %8.3f ms  (%.2fx spmm)" % (name, ms, ms / base), flush=True)
        result["shapes"]["%dx%d" % (heads, D)] = {name: round(ms, 4) for name, ms in row.items()}
        del q, k, v, go
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
