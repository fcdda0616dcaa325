#!/usr/bin/env python3
"""Two-layer R-GCN (DGL's entity-classification example: basis layers, ReLU between them) on the fused typed-edge gather:

    python examples/rgcn/train.py --synthetic [--bf16] [--num-rels 16 --num-bases 4] [--scale 14]

--synthetic: synth.typed_graph -- RMAT edges with Zipf-distributed types, reverse edges as types of their own, norm = 1 / c_{i, r};
a node's label says WHICH edge types reach it.  The features are noise plus one constant column, so the label cannot be read off a
node's own row.  Even nodes train, odd nodes test.  Adam; --bf16 keeps the activations in bf16 (fp32 parameters).

After the run the same model is trained the same way with every edge type set to 0 (same graph, same norms): a type-blind model.
Its test accuracy is printed next to the typed one -- a sanity line, not a test.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from dgll_amd import synth  # noqa: E402
from dgll_amd.nn.Convolution import RGCN  # noqa: E402
from dgll_amd.ops_typed import TypedEdges, typed_graph_from_coo  # noqa: E402


def run(args, graph, edges, x, labels, train, test, label):
    torch.manual_seed(0)
    model = RGCN(x.shape[1], args.hidden, int(labels.max()) + 1, edges.num_rels, args.num_bases).to(x.device)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    acc = 0.0
    for epoch in range(args.epochs):
        model.train()
        torch.cuda.synchronize()
        t0 = time.time()
        opt.zero_grad(set_to_none=True)
        logits = model(graph, x, edges).float()
        loss = torch.nn.functional.cross_entropy(logits[train], labels[train])
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        dt = time.time() - t0
        if epoch % 10 == 0 or epoch == args.epochs - 1:
            model.eval()
            with torch.no_grad():
                pred = model(graph, x, edges).argmax(1)
            acc = float((pred[test] == labels[test]).float().mean())
            print("%s epoch %3d  loss %.4f  train acc %.3f  test acc %.3f  %.1f ms" % (
                label, epoch, loss.item(), float((pred[train] == labels[train]).float().mean()), acc, dt * 1e3))
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--scale", type=int, default=14, help="2^scale nodes")
    ap.add_argument("--edge-factor", type=int, default=8)
    ap.add_argument("--num-rels", type=int, default=16, help="edge types before the reverse edges double them")
    ap.add_argument("--num-bases", type=int, default=4)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--in-feat", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--lr", type=float, default=2e-2)
    ap.add_argument("--weight-decay", type=float, default=0.0)
    ap.add_argument("--bf16", action="store_true")
    args = ap.parse_args()
    if not args.synthetic:
        raise SystemExit("pass --synthetic (no typed dataset loader is built)")
    if not torch.cuda.is_available():
        raise SystemExit("this example runs the HIP kernels: a GPU is required")
    dev = torch.device("cuda:0")
    d = synth.typed_graph(args.scale, edge_factor=args.edge_factor, num_rels=args.num_rels, n_classes=args.classes, seed=0, device=dev,
                          reverse=True)
    n = d["num_nodes"]
    graph, edges = typed_graph_from_coo(d["src"], d["dst"], d["etypes"], d["norm"], n, n, d["num_rels"])
    labels = d["labels"]
    x = torch.randn(n, args.in_feat, generator=torch.Generator().manual_seed(0))
    x[:, 0] = 1.0
    x = x.to(dev).to(torch.bfloat16 if args.bf16 else torch.float32)
    ids = torch.arange(n, device=dev)
    train, test = ids[ids % 2 == 0], ids[ids % 2 == 1]
    print("%d nodes, %d edges, %d edge types, %d bases, classes %s" % (n, graph.nnz, edges.num_rels, args.num_bases,
                                                                       torch.bincount(labels).tolist()))
    typed = run(args, graph, edges, x, labels, train, test, "typed")
    blind = run(args, graph, TypedEdges(graph, torch.zeros_like(edges.etypes), edges.num_rels, edges.norm), x, labels, train, test, "blind")
    print("test accuracy: typed %.3f, all edge types set to 0 %.3f" % (typed, blind))


if __name__ == "__main__":
    main()
