#!/usr/bin/env python3
"""Subgraph-sampled training: every batch is ONE induced subgraph (ShaDow-GNN's k-hop neighbourhood of the seeds, or a GraphSAINT
node / edge / random-walk sample) built on the device, and a GraphSAGE-mean model of any depth runs its full-graph layers on it --
no per-layer blocks:
    h = W_self h + W_neigh mean_{u in N(v), u in the batch} h_u     (the mean is ops.spmm on the subgraph's 1 / kept values)
ShaDow takes the loss on the seed rows (the first rows of the subgraph), GraphSAINT on the training nodes of the subgraph.

    python examples/subgraph/train.py --sampler shadow --fanouts 10,5 --batch 1024
    python examples/subgraph/train.py --sampler saint-node --budget 6000
    python examples/subgraph/train.py --sampler saint-edge --budget 4000
    python examples/subgraph/train.py --sampler saint-walk --roots 2000 --length 4 --layers 3
    python examples/subgraph/train.py --sampler saint-node --nodes 4000 --budget 500 --batches 6      # small enough for a test
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from dgll_amd import ops, synth  # noqa: E402
from dgll_amd.sampling import SAINTSampler, ShaDowKHopSampler, layerwise  # noqa: E402


class SageMean(torch.nn.Module):
    """GraphSAGE with the mean aggregator on one graph: a (self, neighbour) pair of weights per layer, ReLU between layers."""

    def __init__(self, in_feats, h_feats, num_classes, layers=2):
        super().__init__()
        dims = [in_feats] + [h_feats] * (layers - 1) + [num_classes]
        self.w_self = torch.nn.ModuleList(torch.nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))
        self.w_neigh = torch.nn.ModuleList(torch.nn.Linear(a, b, bias=False) for a, b in zip(dims[:-1], dims[1:]))

    def forward(self, g, x):
        h = x
        for i in range(len(self.w_self)):
            h = self.w_self[i](h) + self.w_neigh[i](ops.spmm(g, h))
            if i + 1 < len(self.w_self):
                h = torch.relu(h)
        return h


def batches(args, g, train, dev):
    """Yields (nodes, subgraph, rows whose loss counts) -- `batches` of them per epoch."""
    if args.sampler == "shadow":
        sampler = ShaDowKHopSampler([int(f) for f in args.fanouts.split(",")], g)
        ids = torch.nonzero(train).flatten()
        while True:
            perm = ids[torch.randperm(ids.numel(), device=dev)]
            for i in range(0, perm.numel(), args.batch):
                seeds = perm[i:i + args.batch]
                nodes, _, sub = sampler.sample(None, seeds)
                yield nodes, sub, torch.arange(seeds.numel(), device=dev)
    mode = args.sampler.split("-")[1]
    sampler = SAINTSampler(mode, (args.roots, args.length) if mode == "walk" else args.budget, g)
    while True:
        nodes, sub = sampler.sample()
        yield nodes, sub, torch.nonzero(train[nodes]).flatten()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sampler", choices=("shadow", "saint-node", "saint-edge", "saint-walk"), default="shadow")
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--avg-degree", type=int, default=50)
    ap.add_argument("--feats", type=int, default=100)
    ap.add_argument("--classes", type=int, default=47)
    ap.add_argument("--layers", type=int, choices=(2, 3), default=2)
    ap.add_argument("--batch", type=int, default=1024, help="shadow: seeds per batch")
    ap.add_argument("--fanouts", default="10,5", help="shadow: DGL's order, the last entry is applied to the seeds first")
    ap.add_argument("--budget", type=int, default=6000, help="saint-node / saint-edge: draws per batch")
    ap.add_argument("--roots", type=int, default=2000, help="saint-walk: walks per batch")
    ap.add_argument("--length", type=int, default=4, help="saint-walk: steps per walk")
    ap.add_argument("--batches", type=int, default=50, help="batches per epoch")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this example runs the HIP kernels: a GPU is required")
    dev = torch.device("cuda:0")
    np.random.seed(args.seed)                    # sample() draws its per-batch seed from numpy's global generator
    torch.manual_seed(args.seed)
    g = synth.products_like_graph(dev, seed=0, n=args.nodes, n_undirected=args.nodes * args.avg_degree // 2, locality=0.9)
    n = g.n_rows
    labels = ((torch.arange(n) * 64 // n) % args.classes).to(dev)                 # the planted community
    feats = torch.randn(n, args.feats, device=dev) + torch.nn.functional.one_hot(labels % args.feats, args.feats) * 2.0
    train = torch.rand(n, device=dev) < 0.5
    model = SageMean(args.feats, 128, args.classes, layers=args.layers).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    cur = torch.cuda.current_stream(dev)
    stream = batches(args, g, train, dev)
    for epoch in range(args.epochs):
        t0, total, seen, correct, held, size = time.time(), 0.0, 0, 0, 0, 0
        for _ in range(args.batches):
            nodes, sub, rows = next(stream)
            layerwise.record_stream([sub], nodes, cur)      # built on the sampler's stream, used on this one
            y = labels[nodes]
            logits = model(sub, feats[nodes])
            size += nodes.numel()
            if rows.numel() == 0:
                continue
            loss = ops.cross_entropy(logits[rows], y[rows])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            total += float(loss) * rows.numel()
            seen += rows.numel()
            rest = ~train[nodes]                            # the batch's nodes outside the training set
            correct += int((logits[rest].argmax(1) == y[rest]).sum())
            held += int(rest.sum())
        torch.cuda.synchronize()
        print("epoch %d  loss %.4f  held-out acc %.3f  %.0f nodes / batch  %.2f s"
              % (epoch, total / max(seen, 1), correct / max(held, 1), size / args.batches, time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
