#!/usr/bin/env python3
"""Per-pass timing of the three edge-feature passes (csrc/edge_feat.hip: FORWARD, COLS, EDGE) for the three ops (add, add_relu, mul)
at F = 64 and 256, bf16 and fp32, next to ops.spmm of the same width over A and over A^T (the floor by traffic is that SpMM plus one
streamed read of e, nnz * F * sizeof; COLS reaches e through perm, a scattered read per entry) and, on the Reddit shape only, the
torch composition the passes replace: relu(x[col] + e) into index_add_, and its autograd backward (its three [nnz, F] temporaries do
not fit at the products shape).

    python tools/edge_feat_bench.py --graph reddit|products [--reps 3 --rounds 1 --widths 64,256 --dtypes bf16,fp32]

Synthetic graphs (reddit-shaped: 232 965 nodes, 57.3 M undirected edges; products-shaped: synth.products_like_graph defaults), with
self-loops.  HIP events round `reps` launches after two warm-up launches, one process on the card; the median of `rounds` is
reported.  e and grad_e are real [nnz, F] arrays: their bytes are printed, and a shape whose arrays do not fit the card's free memory
is skipped with a note (as is the composition where its temporaries do not fit).  Prints a table and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dgll_amd import _lib, ops, ops_ef, synth  # noqa: E402

GRAPHS = {"products": dict(), "reddit": dict(n=232_965, n_undirected=57_300_000)}
OPS = (("add", _lib.EF_ADD), ("add_relu", _lib.EF_ADD_RELU), ("mul", _lib.EF_MUL))


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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--widths", default="64,256")
    ap.add_argument("--dtypes", default="bf16,fp32")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = synth.products_like_graph(dev, seed=0, locality=0.9, self_loops=True, **GRAPHS[args.graph])
    gt, _ = g.transpose()
    g.plan(), gt.plan()
    n, nnz = g.n_rows, g.nnz
    print("%s-shaped graph: %d nodes, %d entries" % (args.graph, n, nnz), flush=True)
    result = {"graph": args.graph, "nodes": n, "nnz": nnz, "shapes": {}}
    torch.manual_seed(0)
    for name in args.dtypes.split(","):
        dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[name]
        for F in (int(w) for w in args.widths.split(",")):
            key = "%s_F%d" % (name, F)
            e_bytes = nnz * F * (2 if dtype == torch.bfloat16 else 4)
            free = torch.cuda.mem_get_info(dev)[0]
            print("F = %d %s: e is %.2f GB (grad_e as much)" % (F, name, e_bytes / 1e9), flush=True)
            if 2.2 * e_bytes > free:
                print("  skipped: e and grad_e need %.1f GB, %.1f GB are free" % (2.2 * e_bytes / 1e9, free / 1e9), flush=True)
                result["shapes"][key] = {"e_bytes": e_bytes, "skipped": "memory"}
                continue
            x = torch.randn(n, F, device=dev).to(dtype)
            go = torch.randn(n, F, device=dev).to(dtype)
            e = torch.empty(nnz, F, device=dev, dtype=dtype).normal_()
            ge = torch.empty(nnz, F, device=dev, dtype=dtype)
            table = {"spmm": lambda: ops.spmm_raw(g, x, reduce="sum"), "spmm_t": lambda: ops.spmm_raw(gt, go, reduce="sum")}
            for op_name, op in OPS:
                table["forward " + op_name] = lambda op=op: ops_ef.forward_raw(g, x, e, op)
                table["cols " + op_name] = lambda op=op: ops_ef.cols_raw(g, x, e, go, op)
                table["edge " + op_name] = lambda op=op: ops_ef.edge_raw(g, x, e, go, op, out=ge)
            samples = {k: [] for k in table}
            for _ in range(args.rounds):
                for k, fn in table.items():
                    samples[k].append(timeit(fn, args.reps))
            row = {k: statistics.median(v) for k, v in samples.items()}
            del ge
            torch.cuda.empty_cache()
            if args.graph == "reddit":
                # x[col], the sum, its relu, the copies autograd keeps and the gradients of the same size: about seven arrays like e
                free = torch.cuda.mem_get_info(dev)[0]
                if 7 * e_bytes > free:
                    print("  torch composition skipped: its [nnz, F] temporaries need about %.1f GB, %.1f GB are free"
                          % (7 * e_bytes / 1e9, free / 1e9), flush=True)
                else:
                    rows, col = g.row_index(), g.col.long()

                    def composed(backward):
                        xs, es = (x.detach().requires_grad_(backward), e.detach().requires_grad_(backward))
                        out = torch.zeros(n, F, device=dev, dtype=dtype).index_add_(0, rows, torch.relu(xs[col] + es))
                        if backward:
                            out.backward(go)

                    fwd = statistics.median(timeit(lambda: composed(False), args.reps) for _ in range(args.rounds))
                    both = statistics.median(timeit(lambda: composed(True), args.reps) for _ in range(args.rounds))
                    row["torch forward add_relu"], row["torch backward add_relu"] = fwd, both - fwd
                    del rows, col
            for k, ms in row.items():
                print("  %-26s %9.3f ms" % (k, ms), flush=True)
            result["shapes"][key] = dict({k: round(ms, 4) for k, ms in row.items()}, e_bytes=e_bytes)
            del x, go, e, table
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
