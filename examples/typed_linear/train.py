#!/usr/bin/env python3
"""A per-node-type input projection (TypedLinear) in front of two GraphSAGE layers:

    python examples/typed_linear/train.py --synthetic [--bf16] [--types 32] [--scale 14]

--synthetic: an RMAT graph whose nodes have one of --types types.  A node's raw features carry its label through a random matrix
that is DIFFERENT for every node type (x_i = onehot(label_i) . M[type_i] + noise), as the feature columns of the node types of a
heterogeneous graph mean different things.  With more (type, class) directions than feature columns no single matrix decodes
every type.  Even nodes train, odd nodes test.  Adam; --bf16 keeps the activations in bf16 (fp32 parameters).

The model is TypedLinear -> GraphSage (two layers, full graph).  After the run the same model is trained the same way with ONE
shared matrix in TypedLinear's place (num_types = 1, every node of type 0); its test accuracy is printed next to the typed one --
a sanity line, not a test.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from dgll_amd import synth  # noqa: E402
from dgll_amd.nn.Convolution import GraphSage, TypedLinear  # noqa: E402


class Model(torch.nn.Module):
    def __init__(self, in_feat, hidden, classes, num_types):
        super().__init__()
        self.proj = TypedLinear(in_feat, hidden, num_types)
        self.sage = GraphSage(hidden, [hidden, classes], None)

    def forward(self, graph, x, types):
        return self.sage.forward_graph(graph, torch.relu(self.proj(x, types)))


def run(args, graph, x, types, num_types, labels, train, test, label):
    torch.manual_seed(0)
    model = Model(x.shape[1], args.hidden, int(labels.max()) + 1, num_types).to(x.device)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    acc = 0.0
    for epoch in range(args.epochs):
        model.train()
        torch.cuda.synchronize()
        t0 = time.time()
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(graph, x, types).float()[train], labels[train])
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        dt = time.time() - t0
        if epoch % 10 == 0 or epoch == args.epochs - 1:
            model.eval()
            with torch.no_grad():
                pred = model(graph, x, types).argmax(1)
            acc = float((pred[test] == labels[test]).float().mean())
            print("%s epoch %3d  loss %.4f  test acc %.3f  %.1f ms" % (label, epoch, loss.item(), acc, dt * 1e3))
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--scale", type=int, default=14, help="2^scale nodes")
    ap.add_argument("--edge-factor", type=int, default=8)
    ap.add_argument("--types", type=int, default=32)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--in-feat", type=int, default=16)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--noise", type=float, default=0.5)
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--bf16", action="store_true")
    args = ap.parse_args()
    if not args.synthetic:
        raise SystemExit("pass --synthetic (no node-typed dataset loader is built)")
    if not torch.cuda.is_available():
        raise SystemExit("this example runs the HIP kernels: a GPU is required")
    dev = torch.device("cuda:0")
    graph = synth.rmat_graph(args.scale, args.edge_factor, seed=0, device=dev, symmetric=True, weighted=False)
    n = graph.n_rows
    gen = torch.Generator().manual_seed(0)
    types = torch.randint(0, args.types, (n,), generator=gen)
    labels = torch.randint(0, args.classes, (n,), generator=gen)
    mats = torch.randn(args.types, args.classes, args.in_feat, generator=gen)
    x = mats[types, labels] + args.noise * torch.randn(n, args.in_feat, generator=gen)
    x = x.to(dev).to(torch.bfloat16 if args.bf16 else torch.float32)
    types, labels = types.to(dev), labels.to(dev)
    ids = torch.arange(n, device=dev)
    train, test = ids[ids % 2 == 0], ids[ids % 2 == 1]
    print("%d nodes, %d edges, %d node types, %d classes, %d feature columns" % (n, graph.nnz, args.types, args.classes, args.in_feat))
    typed = run(args, graph, x, types, args.types, labels, train, test, "typed ")
    shared = run(args, graph, x, torch.zeros_like(types), 1, labels, train, test, "shared")
    print("test accuracy: TypedLinear %.3f, one shared Linear %.3f" % (typed, shared))


if __name__ == "__main__":
    main()
