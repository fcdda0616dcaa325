#!/usr/bin/env python3
"""Per-pass timing of the six message-passing passes (csrc/mp_ops.hip) at 8 x 32 and 1 x 64 bf16 node matrices (per-edge tensors are
fp32 [nnz, heads]), over A and -- where a backward uses it -- over A^T with perm, next to ops.spmm at the same width and the three
fused sparse-attention passes (csrc/sparse_attn.hip) on the same graph.  The fused passes are the baseline this general path is
allowed to lose to: they store nothing per edge.

    python tools/mp_bench.py --graph reddit|products [--reps 10]

Synthetic graphs (reddit-shaped: 232 965 nodes, 57.3 M undirected edges; products-shaped: synth.products_like_graph defaults), with
self-loops.  HIP events round `reps` launches after two warm-up launches, one process on the card.  Prints a table and one JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dgll_amd import ops, ops_attn, ops_mp, synth  # noqa: E402

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
        e = torch.randn(g.nnz, heads, device=dev)
        ge = torch.randn(g.nnz, heads, device=dev)
        a = torch.randn(n, heads, device=dev)
        print("%d x %d bf16: a per-edge tensor is %.2f GB" % (heads, D, 4e-9 * g.nnz * heads), flush=True)
        row = {}
        row["spmm"] = timeit(lambda: ops.spmm_raw(g, v, reduce="mean"), args.reps)
        _, lse = ops_attn.sparse_attention_forward_raw(g, q, k, v, heads, scale)
        row["attn_fwd"] = timeit(lambda: ops_attn.sparse_attention_forward_raw(g, q, k, v, heads, scale), args.reps)
        rows_only = timeit(lambda: ops_attn.sparse_attention_backward_raw(g, q, k, v, heads, scale, lse, go, need_kv=False), args.reps)
        both = timeit(lambda: ops_attn.sparse_attention_backward_raw(g, q, k, v, heads, scale, lse, go, need_kv=True), args.reps)
        row["attn_rows"], row["attn_cols"] = rows_only, both - rows_only
        del lse
        alpha = ops_mp.edge_softmax_raw(g, e)
        row["u_dot_v"] = timeit(lambda: ops_mp.u_dot_v_raw(g, k, q, heads), args.reps)
        row["edge_softmax"] = timeit(lambda: ops_mp.edge_softmax_raw(g, e), args.reps)
        row["edge_softmax_T"] = timeit(lambda: ops_mp.edge_softmax_raw(g, e, transposed=True), args.reps)
        row["edge_softmax_bwd"] = timeit(lambda: ops_mp.edge_softmax_bwd_raw(g, alpha, ge), args.reps)
        row["u_mul_e_sum"] = timeit(lambda: ops_mp.u_mul_e_sum_raw(g, v, alpha, heads), args.reps)
        row["u_mul_e_sum_T"] = timeit(lambda: ops_mp.u_mul_e_sum_raw(g, go, alpha, heads, transposed=True), args.reps)
        row["u_add_v"] = timeit(lambda: ops_mp.u_add_v_raw(g, a, a, heads), args.reps)
        row["e_sum"] = timeit(lambda: ops_mp.e_sum_raw(g, e), args.reps)
        row["e_sum_T"] = timeit(lambda: ops_mp.e_sum_raw(g, e, transposed=True), args.reps)
        # the attention step composed of the family: forward (3 passes) and backward (softmax backward, 2 dots' and 2 sums' gradients)
        row["composed_fwd"] = row["u_dot_v"] + row["edge_softmax"] + row["u_mul_e_sum"]
        row["composed_bwd"] = row["u_mul_e_sum_T"] + row["u_dot_v"] + row["edge_softmax_bwd"] + row["u_mul_e_sum"] + row["u_mul_e_sum_T"]
        base = row["spmm"]
        for name, ms in row.items():
            print("  %-18s %8.3f ms  (%.2fx spmm)" % (name, ms, ms / base), flush=True)
        result["shapes"]["%dx%d" % (heads, D)] = {name: round(ms, 4) for name, ms in row.items()}
        del q, k, v, go, e, ge, a, alpha
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
