#!/usr/bin/env python3
"""Per-pass timing of the typed-edge aggregation (csrc/typed_spmm.hip): EXPAND, CONTRACT, EDGE_DOTS and the per-type SpMM that turns
the edge dots into grad coeff, at F = 64 and 256 bf16, B in {2, 4, 8} bases, R = 16 edge types -- next to the formulation it replaces,
timed in the same process: B calls of ops.spmm_raw(graph.with_values(norm * C[etype, b]), x) INCLUDING the time to form those B value
vectors, and next to one ops.spmm_raw at that width (the floor: one gather, one accumulator).

    python tools/rgcn_bench.py --graph reddit|products [--reps 10]

Synthetic graphs (reddit-shaped: 232 965 nodes, 57.3 M undirected edges; products-shaped: synth.products_like_graph defaults), with
self-loops; types hashed from the entry index, norm uniform in [0.25, 1.25).  HIP events round `reps` launches after two warm-up
launches, one process on the card.  Prints a table and one JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dgll_amd import _lib, ops, ops_typed, synth  # noqa: E402

GRAPHS = {"products": dict(), "reddit": dict(n=232_965, n_undirected=57_300_000)}
R = 16


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
    torch.manual_seed(0)
    etypes = ((torch.arange(g.nnz, device=dev) * 7919 + g.col.long() * 31) % R).to(torch.int32)
    norm = torch.rand(g.nnz, device=dev) + 0.25
    edges = ops_typed.TypedEdges(g, etypes, R, norm)
    t_etypes, t_norm = edges.transposed()
    by_type = edges.by_type()
    by_type.plan()
    print("%s-shaped graph: %d nodes, %d entries, %d edge types" % (args.graph, n, g.nnz, R), flush=True)
    result = {"graph": args.graph, "nodes": n, "nnz": g.nnz, "R": R, "shapes": {}}
    for F in (64, 256):
        x = torch.randn(n, F, device=dev).to(torch.bfloat16)
        floor = timeit(lambda: ops.spmm_raw(g, x), args.reps)
        for B in (2, 4, 8):
            coeff = torch.randn(R, B, device=dev)
            dz = torch.randn(n, B * F, device=dev).to(torch.bfloat16)
            p = torch.empty((g.nnz, (B + 3) // 4 * 4), dtype=torch.float32, device=dev)
            row = {"spmm_once": floor}
            row["expand"] = timeit(lambda: ops_typed.typed_spmm_forward_raw(g, edges, x, coeff), args.reps)
            row["contract"] = timeit(lambda: ops_typed.typed_spmm_backward_raw(g, edges, x, coeff, dz, need_x=True, need_coeff=False), args.reps)
            row["edge_dots"] = timeit(lambda: ops_typed._launch(_lib.TYPED_EDGE_DOTS, g, None, None, R, B, F, None, x=x, dz=dz, p=p), args.reps)
            row["dc_spmm"] = timeit(lambda: ops.spmm_raw(by_type, p), args.reps)

            def replaced():     # what EXPAND replaces: B value vectors formed, B weighted gathers
                for b in range(B):
                    ops.spmm_raw(g.with_values(norm * coeff[etypes.long(), b]), x)

            row["b_spmm_calls"] = timeit(replaced, args.reps)
            print("F = %d bf16, B = %d:" % (F, B), flush=True)
            for name, ms in row.items():
                print("  %-14s %8.3f ms  (%.2fx one spmm)" % (name, ms, ms / floor), flush=True)
            result["shapes"]["F%d_B%d" % (F, B)] = {name: round(ms, 4) for name, ms in row.items()}
            del coeff, dz, p
            torch.cuda.empty_cache()
        del x
    print(json.dumps(result))


if __name__ == "__main__":
    main()
