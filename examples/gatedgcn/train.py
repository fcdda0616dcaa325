#!/usr/bin/env python3
"""Node classification on a graph whose EDGES carry the signal, with nn.GatedGCN (GatedGCNConv layers: Bresson & Laurent's residual
gated graph convnet, which updates the edge features in every layer and gates the messages with them):

    python examples/gatedgcn/train.py --synthetic [--nodes 20000 --classes 8 --degree 10 --hidden 64 --layers 2 --bf16]

--synthetic: the graph of examples/gine/train.py -- a random directed graph; node features are noise about a constant and say nothing
about the label; every edge into node i carries a noisy one-hot code of i's label as its attribute row.  A model that reads the edge
attributes classifies almost perfectly, one that does not is at chance: the script prints the accuracy with the real attributes and
with them zeroed.  Adam; --bf16 keeps the activations in bf16 (fp32 parameters).

Every layer aggregates with ONE autograd node (ops_gated.gated_sum): the gate sigmoid(ehat) is formed in registers per edge, and per
edge only the projected attributes, ehat and their gradients exist.
"""
import argparse
import importlib.util
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from dgll_amd.nn.Convolution import GatedGCN  # noqa: E402

_spec = importlib.util.spec_from_file_location("gine_train", os.path.join(HERE, "..", "gine", "train.py"))
_gine = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gine)
edge_signal_graph = _gine.edge_signal_graph        # the same graph, labels, node features and edge attributes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--nodes", type=int, default=20_000)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--degree", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--bf16", action="store_true")
    args = ap.parse_args()
    if not args.synthetic:
        raise SystemExit("pass --synthetic (the edge-signal graph is the only data source of this example)")
    if not torch.cuda.is_available():
        raise SystemExit("this example runs the HIP kernels: a GPU is required")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    edge_width = max(8, args.classes)
    graph, labels, x, attr = edge_signal_graph(args.nodes, args.classes, args.degree, edge_width, 0, dev)
    if args.bf16:
        x, attr = x.to(torch.bfloat16), attr.to(torch.bfloat16)
    model = GatedGCN(x.shape[1], edge_width, args.hidden, args.classes, layers=args.layers).to(dev)
    graph.transpose()
    print("gatedgcn on %d nodes, %d entries: the edge features are %.1f MB per layer, no gate or message tensor is formed" %
          (graph.n_rows, graph.nnz, 1e-6 * graph.nnz * args.hidden * x.element_size()))
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    for epoch in range(args.epochs):
        model.train()
        torch.cuda.synchronize()
        t0 = time.time()
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(graph, x, attr).float(), labels)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        dt = time.time() - t0
        model.eval()
        with torch.no_grad():
            pred = model(graph, x, attr).argmax(1)
        print("epoch %3d  loss %.4f  acc %.3f  %.1f ms" % (epoch, loss.item(), (pred == labels).float().mean().item(), dt * 1e3))
    model.eval()
    with torch.no_grad():
        real = (model(graph, x, attr).argmax(1) == labels).float().mean().item()
        zeroed = (model(graph, x, torch.zeros_like(attr)).argmax(1) == labels).float().mean().item()
    print("accuracy with the edge attributes %.3f, with them zeroed %.3f (chance %.3f)" % (real, zeroed, 1.0 / args.classes))


if __name__ == "__main__":
    main()
