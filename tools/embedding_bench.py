#!/usr/bin/env python3
"""Throughput of the embedding kernels on the products-shaped synthetic graph: walk steps/s (uniform, node2vec, and both again
edge-weighted through the alias table, whose build time is reported too), skip-gram
pairs/s of one sgns_step at D = 128, L = 80, W = 5, K = 5, and the bytes/s the W_out pass adds atomically (every existing pair
adds K rows for its negatives; the positives of a position are summed first and add one row).  Prints one JSON line.

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
    print(json.dumps(out))


if __name__ == "__main__":
    main()
