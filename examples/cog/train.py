#!/usr/bin/env python3
"""CoG / CommGNN training: size-capped Louvain (or, with --method leiden, Leiden) communities found on the device, merged into groups of at least a batch, the graph
relabelled so that every group is a contiguous id range, and a 2-layer GCN trained on one group's induced subgraph at a time (the
reference's cog.py + CommGNN_train.py; Cluster-GCN style batches):

    python examples/cog/train.py --nodes 200000 --epochs 5
    python examples/cog/train.py --nodes 20000 --batch 2000 --max-comm-size 1000 --epochs 4
    python examples/cog/train.py --nodes 20000 --batch 2000 --method leiden      # every community connected
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from dgll_amd import community, ops, synth  # noqa: E402
from dgll_amd.nn import gcnConv  # noqa: E402
from dgll_amd.sampling import CommunityBatchLoader  # noqa: E402


class Model(torch.nn.Module):
    def __init__(self, in_feats, h_feats, num_classes):
        super().__init__()
        self.conv1 = gcnConv(in_feats, h_feats)
        self.conv2 = gcnConv(h_feats, num_classes)

    def forward(self, g, x):
        return self.conv2(torch.relu(self.conv1(x, g)), g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--avg-degree", type=int, default=50)
    ap.add_argument("--feats", type=int, default=100)
    ap.add_argument("--classes", type=int, default=47)
    ap.add_argument("--batch", type=int, default=20_000)
    ap.add_argument("--max-comm-size", type=int, default=None, help="community size cap (default: the batch size)")
    ap.add_argument("--method", choices=("louvain", "leiden"), default="louvain", help="leiden: refined, connected communities")
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this example runs the HIP kernels: a GPU is required")
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)
    g = synth.products_like_graph(dev, seed=0, n=args.nodes, n_undirected=args.nodes * args.avg_degree // 2, locality=0.9)
    n = g.n_rows
    labels = ((torch.arange(n) * 64 // n) % args.classes).to(dev)                 # the planted community
    feats = torch.randn(n, args.feats, device=dev) + torch.nn.functional.one_hot(labels % args.feats, args.feats) * 2.0
    cap = args.batch if args.max_comm_size is None else args.max_comm_size
    t0 = time.time()
    loader = CommunityBatchLoader(g, feats, labels, args.batch, shuffle=True, seed=args.seed, max_comm_size=cap, method=args.method)
    torch.cuda.synchronize()
    book = loader.book
    sizes = book.community_ranges[:, 1] - book.community_ranges[:, 0]
    print("cog (%s): %d communities (largest %d, cap %d) in %d groups, modularity %.4f, %.2f s"
          % (args.method, sizes.numel(), int(sizes.max()), cap, len(loader), community.modularity(loader.graph, book.community), time.time() - t0))
    train = torch.rand(n, device=dev) < 0.5                                       # in the book's id space, as the batches are
    model = Model(args.feats, 128, args.classes).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    for epoch in range(args.epochs):
        t0, total, seen, correct, held = time.time(), 0.0, 0, 0, 0
        for (start, end), sub, x, y in loader:
            m = train[start:end]
            logits = model(sub, x)
            loss = ops.cross_entropy(logits[m], y[m])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            total += float(loss) * int(m.sum())
            seen += int(m.sum())
            correct += int((logits[~m].argmax(1) == y[~m]).sum())
            held += int((~m).sum())
        torch.cuda.synchronize()
        print("epoch %d  loss %.4f  held-out acc %.3f  %.2f s" % (epoch, total / max(seen, 1), correct / max(held, 1), time.time() - t0))


if __name__ == "__main__":
    main()
