#!/usr/bin/env python3
"""DeepWalk / node2vec node embeddings on a synthetic planted-partition graph: walks and skip-gram with negative sampling on the
device (dgll_amd.embedding).  Prints the loss of every epoch and the mean cosine similarity inside and between the communities:

    python examples/embedding/train.py --method deepwalk
    python examples/embedding/train.py --method node2vec --p 0.5 --q 2 --communities 8 --nodes 4000 --dim 64
    python examples/embedding/train.py --method node2vec --weighted      # edges inside a community weigh 4, the others 1
    python examples/embedding/train.py --method struc2vec --stay-prob 0.3 --num-layers 3 --lr 0.0005
                                       # structural roles, not communities: the intra/inter split is only printed for comparison
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from dgll_amd import CSRGraph, embedding  # noqa: E402


def planted_partition(n, communities, deg_in, deg_out, seed):
    """Undirected graph: every node draws about deg_in neighbours in its own community and deg_out anywhere else."""
    rng = np.random.default_rng(seed)
    comm = np.arange(n) * communities // n
    size = n // communities
    src_in = np.repeat(np.arange(n), deg_in)
    dst_in = np.minimum(comm[src_in] * size + rng.integers(0, size, src_in.size), n - 1)
    src_out = np.repeat(np.arange(n), deg_out)
    dst_out = rng.integers(0, n, src_out.size)
    src, dst = np.concatenate([src_in, src_out]), np.concatenate([dst_in, dst_out])
    keep = src != dst
    src, dst = src[keep], dst[keep]
    row, col = torch.from_numpy(np.concatenate([src, dst])), torch.from_numpy(np.concatenate([dst, src]))
    return CSRGraph.from_coo(row, col, None, (n, n)).with_values(None), comm


def cosine_split(emb, comm, sample=2000, seed=0):
    rng = np.random.default_rng(seed)
    idx = rng.choice(len(comm), min(sample, len(comm)), replace=False)
    e = emb[idx] / emb[idx].norm(dim=1, keepdim=True).clamp(min=1e-30)
    sim = (e @ e.t()).cpu().numpy()
    same = comm[idx][:, None] == comm[idx][None, :]
    off = ~np.eye(len(idx), dtype=bool)
    return sim[same & off].mean(), sim[~same].mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", choices=["deepwalk", "node2vec", "struc2vec"], default="deepwalk")
    ap.add_argument("--nodes", type=int, default=2000)
    ap.add_argument("--communities", type=int, default=4)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--walk-length", type=int, default=40)
    ap.add_argument("--walks-per-vertex", type=int, default=2)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--negatives", type=int, default=5)
    ap.add_argument("--batch-walks", type=int, default=64)
    ap.add_argument("--lr", type=float, default=0.005)
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--q", type=float, default=2.0)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--stay-prob", type=float, default=0.3, help="struc2vec: probability of staying in the layer")
    ap.add_argument("--num-layers", type=int, default=3, help="struc2vec: opt3_num_layers (BFS levels 0..K); -1 = unbounded")
    ap.add_argument("--weighted", action="store_true", help="walk in proportion to edge weights (4 inside a community, 1 across)")
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    g, comm = planted_partition(args.nodes, args.communities, 12, 1, args.seed)
    g = g.to(dev)
    if args.weighted:
        same = torch.from_numpy(comm)[g.row_index().cpu()] == torch.from_numpy(comm)[g.col.cpu().long()]
        g = g.with_values(torch.where(same, 4.0, 1.0).to(dev))
    kw = dict(negatives=args.negatives, batch_walks=args.batch_walks, seed=args.seed, weighted=args.weighted)
    if args.method == "struc2vec":
        kw.pop("weighted")
        emb = embedding.Struc2Vec(g, args.walk_length, args.dim, args.walks_per_vertex, args.window, args.lr, stay_prob=args.stay_prob,
                                  opt3_num_layers=None if args.num_layers < 0 else args.num_layers, **kw)
        print("context graph: %d layers, %d pairs, build seconds %s" % (emb.context.n_layers, emb.context.pairs.shape[0],
                                                                        {k: round(v, 4) for k, v in emb.context.timings.items()}))
    elif args.method == "deepwalk":
        emb = embedding.DeepWalk(g, args.walk_length, args.dim, args.walks_per_vertex, args.window, args.lr, **kw)
    else:
        emb = embedding.Node2vec(g, args.walk_length, args.dim, args.walks_per_vertex, args.window, args.lr, args.p, args.q, **kw)
    torch.manual_seed(args.seed)
    model = embedding.SkipGramModel(emb.totalNodes, args.dim)
    print("%s on %r" % (args.method, g))
    for epoch in range(args.epochs):
        model = emb.learnNodeEmbedding(model)
        intra, inter = cosine_split(model.W1.data, comm)
        print("epoch %d  loss %.1f  cosine intra %.4f  inter %.4f" % (epoch, emb.losses[-1], intra, inter))


if __name__ == "__main__":
    main()
