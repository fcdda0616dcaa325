#!/usr/bin/env python3
"""Per-pass timing of the Gaussian-mixture aggregation (csrc/gmm.hip): EXPAND, CONTRACT, the dots pass that feeds PARAM, and PARAM with
grad_pseudo, at F = 64 and 256, bf16 and fp32, (K, dim) = (3, 2) and (8, 3) -- next to, timed in the same process:

    typed_expand / typed_contract   ops_typed's pass of the same name at B = K bases and one edge type: the SAME gather with the
                                    coefficient read from a table, so the ratio is the price of the Gaussian
    spmm_once                       one ops.spmm_raw at that width (the floor: one gather, one accumulator)
    composition (--graph reddit, K = 3, F = 64 only)
                                    the forward in DGL's order with torch ops: project to K * out columns, gather them per entry, weight,
                                    reduce -- it forms the [nnz, K, out] message tensor

    python tools/gmm_bench.py --graph reddit|products [--reps 5] [--no-composition]

Synthetic graphs (reddit-shaped: 232 965 nodes, 57.3 M undirected edges; products-shaped: synth.products_like_graph defaults), with
self-loops; pseudo uniform in [-1, 1], mu 0.5 N(0, 1), inv_sigma uniform in [0.5, 2].  HIP events round `reps` launches after two
warm-up launches, one process on the card.  Prints a table and one JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dgll_amd import ops, ops_gmm, ops_typed, synth  # noqa: E402

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


def composition(g, row, x, fc, pseudo, mu, sigma):
    """DGL's order of operations, forward only"""
    K = mu.shape[0]
    out = fc.shape[0] // K
    proj = (x @ fc.t()).view(-1, K, out)
    t = (pseudo.unsqueeze(1) - mu.unsqueeze(0)) * sigma.unsqueeze(0)
    w = torch.exp(-0.5 * (t * t).sum(-1)).to(x.dtype)
    msg = proj[g.col.long()] * w.unsqueeze(-1)
    return torch.zeros(g.n_rows, K, out, dtype=x.dtype, device=x.device).index_add_(0, row, msg).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=sorted(GRAPHS), default="reddit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-composition", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = synth.products_like_graph(dev, seed=0, locality=0.9, self_loops=True, **GRAPHS[args.graph])
    gt, _ = g.transpose()
    g.plan(), gt.plan()
    n = g.n_rows
    torch.manual_seed(0)
    one_type = ops_typed.TypedEdges(g, torch.zeros(g.nnz, dtype=torch.int32, device=dev), 1, None, check=False)
    one_type.transposed()
    print("%s-shaped graph: %d nodes, %d entries" % (args.graph, n, g.nnz), flush=True)
    result = {"graph": args.graph, "nodes": n, "nnz": g.nnz, "shapes": {}}
    for K, dim in ((3, 2), (8, 3)):
        pseudo = torch.rand(g.nnz, dim, device=dev) * 2 - 1
        mu = 0.5 * torch.randn(K, dim, device=dev)
        sigma = 0.5 + 1.5 * torch.rand(K, dim, device=dev)
        table = torch.rand(1, K, device=dev)
        for dtype, F in ((torch.bfloat16, 64), (torch.bfloat16, 256), (torch.float32, 64), (torch.float32, 256)):
            x = torch.randn(n, F, device=dev).to(dtype)
            dz = torch.randn(n, K * F, device=dev).to(dtype)
            row = {"spmm_once": timeit(lambda: ops.spmm_raw(g, x), args.reps)}
            row["expand"] = timeit(lambda: ops_gmm.expand_raw(g, x, pseudo, mu, sigma), args.reps)
            row["typed_expand"] = timeit(lambda: ops_typed.typed_spmm_forward_raw(g, one_type, x, table), args.reps)
            row["contract"] = timeit(lambda: ops_gmm.contract_raw(g, pseudo, mu, sigma, dz), args.reps)
            row["typed_contract"] = timeit(lambda: ops_typed.typed_spmm_backward_raw(g, one_type, x, table, dz, need_x=True, need_coeff=False),
                                           args.reps)
            row["dots"] = timeit(lambda: ops_gmm.edge_dots_raw(g, x, dz, K), args.reps)
            p = ops_gmm.edge_dots_raw(g, x, dz, K)
            row["param"] = timeit(lambda: ops_gmm.param_raw(p, pseudo, mu, sigma, want_pseudo=True), args.reps)
            del p
            if args.graph == "reddit" and not args.no_composition and K == 3 and F == 64:
                fc = torch.randn(K * F, F, device=dev).to(dtype)
                rows = g.row_index()
                try:
                    with torch.no_grad():
                        row["composition"] = timeit(lambda: composition(g, rows, x, fc, pseudo, mu, sigma), max(1, args.reps // 2))
                except torch.OutOfMemoryError:
                    row["composition"] = float("nan")
                del fc, rows
            name = "F%d_%s_K%d_dim%d" % (F, "bf16" if dtype == torch.bfloat16 else "fp32", K, dim)
            print(name + ":", flush=True)
            for key, ms in row.items():
                ratio = ""
                if key in ("expand", "contract"):
                    ratio = "  (%.2fx the typed pass, %.2fx one spmm)" % (ms / row["typed_" + key], ms / row["spmm_once"])
                print("  %-15s %8.3f ms%s" % (key, ms, ratio), flush=True)
            result["shapes"][name] = {key: round(ms, 4) for key, ms in row.items()}
            del x, dz
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
