#!/usr/bin/env python3
"""Mini-batch GraphSAGE-mean on device-sampled message-flow-graph blocks -- the loop of the reference's MQGraphSAGE.py / MQGCN.py
(`NeighborSampler([4, 4])`, line 114; DataLoader; Queue) on a synthetic products-shaped graph: NeighborSampler draws every hop on
the GPU, each block's sources are unique with the destinations first, so a layer is
    h_dst = W_self h[:n_dst] + W_neigh mean_{u in N(v)} h_u        (the mean is ops.spmm on the block's 1 / count values)

    python examples/neighbor/train.py --nodes 200000 --fanouts 10,25 --batch 1024 --epochs 3
    python examples/neighbor/train.py --weighted       # edge-weighted sampling: NeighborSampler(prob=...), weight 1 / in-degree of the source
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from dgll_amd import ops, synth  # noqa: E402
from dgll_amd.cache import GraphCacheServer  # noqa: E402
from dgll_amd.data import DGraph  # noqa: E402
from dgll_amd.dataloader import DataLoader  # noqa: E402
from dgll_amd.pipeline import MiniBatchPipeline  # noqa: E402
from dgll_amd.sampling import NeighborSampler, layerwise  # noqa: E402


class SageMean(torch.nn.Module):
    """GraphSAGE with the mean aggregator on blocks: one (self, neighbour) pair of weights per block, ReLU between layers."""

    def __init__(self, in_feats, h_feats, num_classes, layers=2):
        super().__init__()
        dims = [in_feats] + [h_feats] * (layers - 1) + [num_classes]
        self.w_self = torch.nn.ModuleList(torch.nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))
        self.w_neigh = torch.nn.ModuleList(torch.nn.Linear(a, b, bias=False) for a, b in zip(dims[:-1], dims[1:]))

    def forward(self, blocks, x):
        h = x
        for i, blk in enumerate(blocks):
            h = self.w_self[i](h[:blk.n_rows]) + self.w_neigh[i](ops.spmm(blk, h))
            if i + 1 < len(blocks):
                h = torch.relu(h)
        return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--avg-degree", type=int, default=50)
    ap.add_argument("--feats", type=int, default=100)
    ap.add_argument("--classes", type=int, default=47)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--fanouts", default="10,25", help="DGL's order: the last entry is applied to the seeds first; -1 = every neighbour")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weighted", action="store_true",
                    help="sample neighbours in proportion to an edge weight (1 / in-degree of the source: hubs are drawn less often)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this example runs the HIP kernels: a GPU is required")
    dev = torch.device("cuda:0")
    np.random.seed(args.seed)                    # sample() draws its per-batch seed from numpy's global generator
    torch.manual_seed(args.seed)
    g = synth.products_like_graph(dev, seed=0, n=args.nodes, n_undirected=args.nodes * args.avg_degree // 2, locality=0.9)
    n = g.n_rows
    labels = (torch.arange(n) * 64 // n) % args.classes                          # the planted community
    feats = torch.randn(n, args.feats) + torch.nn.functional.one_hot(labels % args.feats, args.feats) * 2.0
    dg = DGraph.from_csr(g.rowptr.cpu().numpy(), g.col.cpu().numpy().astype(np.int64), labels=labels, features=feats)
    fanouts = [int(f) for f in args.fanouts.split(",")]
    prob = None
    if args.weighted:                            # one weight per entry of g, in entry order; a source without in-neighbours counts as degree 1
        prob = 1.0 / g.degrees().clamp(min=1).to(torch.float32)[g.col.long()]
    sampler = NeighborSampler(fanouts, g, prob=prob)
    cache = GraphCacheServer(feats, gpuid=0)
    cache.auto_cache(g.degrees().cpu(), capacity=n // 2)
    model = SageMean(args.feats, 128, args.classes, layers=len(fanouts)).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    train = torch.nonzero(torch.rand(n) < 0.5).flatten()
    cur = torch.cuda.current_stream(dev)
    for epoch in range(args.epochs):
        loader = DataLoader(dg, train[torch.randperm(len(train))], sampler, batch_size=args.batch)
        pipe = MiniBatchPipeline(loader, cache=cache, labels=labels, queue_size=4, device=dev)
        t0, total, correct, seen = time.time(), 0.0, 0, 0
        for b in pipe:
            # the blocks and input ids come from the sampler's stream: tell the allocator they are used on this one
            layerwise.record_stream(b.subgraphs, b.input_nodes, cur)
            logits = model(b.subgraphs, b.features[0].contiguous())
            loss = ops.cross_entropy(logits, b.labels)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            k = b.labels.numel()
            total += float(loss) * k
            correct += int((logits.argmax(1) == b.labels).sum())
            seen += k
        torch.cuda.synchronize()
        print("epoch %d  loss %.4f  train acc %.3f  %.2f s" % (epoch, total / max(seen, 1), correct / max(seen, 1), time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
