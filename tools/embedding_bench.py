#!/usr/bin/env python3
"""Throughput of the embedding kernels on the products-shaped synthetic graph: walk steps/s (uniform, node2vec, and both again
edge-weighted through the alias table, whose build time is reported too), skip-gram
pairs/s of one sgns_step at D = 128, L = 80, W = 5, K = 5, and the bytes/s the W_out pass adds atomically (every existing pair
adds K rows for its negatives; the positives of a position are summed first and add one row); and struc2vec on a smaller graph
of the same shape (--struc-nodes, stated in the output): the context build split into BFS, pairs, DTW, graph and alias seconds,
DTW tasks/s and cells/s, and the multilayer walk's steps/s.  Prints one JSON line.

    python tools/embedding_bench.py [--nodes N] [--walks 4096] [--reps 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dgll_amd import embedding, synth  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) * 1e-3)
    return best


def struc2vec_section(dev, args):
    """Context build (opt1 and opt2 on) and multilayer walk on a products-shaped graph of --struc-nodes nodes."""
    from dgll_amd.embedding import struc2vec as s2v

    sn = args.struc_nodes
    g = synth.products_like_graph(dev, n=sn, n_undirected=max(sn, int(args.edges * (sn / args.nodes))))
    s2v.StrucContext.from_graph(g, True, True, args.struc_layers)             # warm-up: allocator, SpMM plan
    ctx = s2v.StrucContext.from_graph(g, True, True, args.struc_layers)
    res = {"nodes": g.n_rows, "nnz": g.nnz, "levels": ctx.n_layers, "pairs": int(ctx.pairs.shape[0]), "stacked_edges": ctx.graph.nnz,
           "build_s": {k: v for k, v in ctx.timings.items()}}
    lens = ctx.seqs.lengths()
    pl = ctx.pairs.to(torch.int64)
    valid = ctx.dist >= 0
    cells = int((lens[pl[:, 0]] * lens[pl[:, 1]])[valid].sum())
    t = timed(lambda: s2v.struc_dtw(ctx.seqs, ctx.pairs), args.reps)            # includes the length check's blocking read
    res.update(dtw_s=t, dtw_tasks_per_s=int(valid.sum()) / t, dtw_cells_per_s=cells / t, dtw_mean_cells_per_task=cells / max(int(valid.sum()), 1))
    starts = torch.randint(0, g.n_rows, (args.walks,), device=dev)
    t = timed(lambda: s2v.struc_walks(ctx, starts, args.length, 0.3, 1, 0), args.reps)
    walks = s2v.struc_walks(ctx, starts, args.length, 0.3, 1, 0)
    res["walk_steps_per_s"] = int((walks[:, 1:] >= 0).sum()) / t
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=synth.PRODUCTS_NODES)
    ap.add_argument("--edges", type=int, default=synth.PRODUCTS_UNDIRECTED_EDGES)
    ap.add_argument("--walks", type=int, default=4096)
    ap.add_argument("--length", type=int, default=80)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--negatives", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--struc-nodes", type=int, default=20000, help="struc2vec section: nodes of its graph (0 skips the section)")
    ap.add_argument("--struc-layers", type=int, default=3, help="struc2vec section: opt3_num_layers")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = synth.products_like_graph(dev, n=args.nodes, n_undirected=args.edges)
    n, L, D, W, K = args.walks, args.length, args.dim, args.window, args.negatives
    starts = torch.randint(0, g.n_rows, (n,), device=dev)
    out = {"nodes": g.n_rows, "nnz": g.nnz, "walks": n, "length": L, "dim": D, "window": W, "negatives": K}
    for name, (p, q) in (("uniform", (1.0, 1.0)), ("node2vec_p0.5_q2", (0.5, 2.0))):
        embedding.random_walks(g, starts, 2, p=p, q=q)            # the one-off row-order check is not part of the rate
        t = timed(lambda: embedding.random_walks(g, starts, L, p=p, q=q, seed=1), args.reps)
        walks = embedding.random_walks(g, starts, L, p=p, q=q, seed=1)
        steps = int((walks[:, 1:] >= 0).sum())
        out["walk_steps_per_s_" + name] = steps / t
    # edge weights 2^u, u uniform in [-2, 2): the table build (one lane per row, once per graph) and the same two walks through it
    gw = g.with_values(torch.exp2(torch.rand(g.nnz, device=dev) * 4.0 - 2.0))

    def build_table():
        gw._alias = None
        return embedding.AliasTable.from_graph(gw)

    out["alias_build_s"] = timed(build_table, args.reps)                  # includes the blocking read of the info word
    alias = embedding.AliasTable.from_graph(gw)
    out["alias_table_bytes"] = alias.table.numel() * 4
    for name, (p, q) in (("weighted", (1.0, 1.0)), ("weighted_node2vec_p0.5_q2", (0.5, 2.0))):
        embedding.random_walks(gw, starts, 2, p=p, q=q, alias=alias)
        t = timed(lambda: embedding.random_walks(gw, starts, L, p=p, q=q, seed=1, alias=alias), args.reps)
        walks = embedding.random_walks(gw, starts, L, p=p, q=q, seed=1, alias=alias)
        out["walk_steps_per_s_" + name] = int((walks[:, 1:] >= 0).sum()) / t
    walks = embedding.random_walks(g, starts, L, seed=1)
    noise = embedding.NoiseTable.from_graph(g)
    w_in = torch.rand((g.n_rows, D), device=dev)
    w_out = torch.rand((g.n_rows, D), device=dev)
    negs = embedding.sgns_negatives(walks, W, 1, noise, seed=2)
    pairs = int((negs[..., 0] >= 0).sum())
    positions = int((walks >= 0).sum())
    t = timed(lambda: embedding.sgns_step(w_in, w_out, walks, W, K, noise, 1e-4, 2), args.reps)
    out["sgns_step_s"] = t
    out["sgns_pairs_per_s"] = pairs / t
    out["sgns_targets_per_s"] = pairs * (1 + K) / t
    atomic_bytes = (pairs * K + positions) * D * 4
    out["w_out_atomic_bytes_per_step"] = atomic_bytes
    out["w_out_atomic_bytes_per_s_over_whole_step"] = atomic_bytes / t
    if args.struc_nodes:
        out["struc2vec"] = struc2vec_section(dev, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
