#!/usr/bin/env python3
"""Mini-batch GCN on layer-wise importance samplers -- the reference's MQLadies.py / MQFastGCN.py training loop (Model: two GCN
layers, hidden 128, ReLU between them, MQLadies.py:48-60; Adam; cross-entropy) on a synthetic products-shaped graph, through
DataLoader + MiniBatchPipeline with a partly cached GraphCacheServer:

    python examples/layerwise/train.py --sampler ladies --nodes 200000 --epochs 2
    python examples/layerwise/train.py --sampler fastgcn
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
from dgll_amd.nn import gcnConv  # noqa: E402
from dgll_amd.pipeline import MiniBatchPipeline  # noqa: E402
from dgll_amd.sampling import layerwise  # noqa: E402

SAMPLERS = {"ladies": layerwise.Ladies, "ladies-flat": lambda f, g: layerwise.Ladies(f, g, flat=True),
            "fastgcn": layerwise.FastGCNSampler, "fastgcn-flat": lambda f, g: layerwise.FastGCNSamplerFlat(f, g, flat=True),
            "fastgcn-flat-wrs": lambda f, g: layerwise.FastGCNSamplerFlat(f, g, flat=True, wrs=True)}


class Model(torch.nn.Module):
    def __init__(self, in_feats, h_feats, num_classes):
        super().__init__()
        self.conv1 = gcnConv(in_feats, h_feats)
        self.conv2 = gcnConv(h_feats, num_classes)

    def forward(self, blocks, x):
        h = torch.relu(self.conv1(x, blocks[0]))
        return self.conv2(h, blocks[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sampler", choices=sorted(SAMPLERS), default="ladies")
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--avg-degree", type=int, default=50)
    ap.add_argument("--feats", type=int, default=100)
    ap.add_argument("--classes", type=int, default=47)
    ap.add_argument("--batch", type=int, default=1023)
    ap.add_argument("--fanouts", default="512,1024")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
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
    sampler = SAMPLERS[args.sampler]([int(f) for f in args.fanouts.split(",")], g)
    cache = GraphCacheServer(feats, gpuid=0)
    cache.auto_cache(g.degrees().cpu(), capacity=n // 2)
    model = Model(args.feats, 128, args.classes).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    train = torch.nonzero(torch.rand(n) < 0.1).flatten()
    cur = torch.cuda.current_stream(dev)
    for epoch in range(args.epochs):
        loader = DataLoader(dg, train[torch.randperm(len(train))], sampler, batch_size=args.batch)
        pipe = MiniBatchPipeline(loader, cache=cache, labels=labels, queue_size=4, device=dev)
        t0, correct, seen = time.time(), 0, 0
        for b in pipe:
            # the blocks and input ids come from the sampler's stream: tell the allocator they are used on this one
            layerwise.record_stream(b.subgraphs, b.input_nodes, cur)
            logits = model(b.subgraphs, b.features[0])
            loss = ops.cross_entropy(logits, b.labels)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            correct += int((logits.argmax(1) == b.labels).sum())
            seen += b.labels.numel()
        torch.cuda.synchronize()
        print("epoch %d  loss %.4f  train acc %.3f  %.2f s" % (epoch, loss.item(), correct / max(seen, 1), time.time() - t0))


if __name__ == "__main__":
    main()
