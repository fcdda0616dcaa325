#!/usr/bin/env python3
"""Node classification on a graph whose EDGES carry the signal, with nn.GINE (GINEConv layers, each with its own encoder of the edge
attributes) or nn.CFConv (SchNet's continuous-filter convolution):

    python examples/gine/train.py --synthetic [--layer gine|cfconv --nodes 20000 --classes 8 --degree 10 --hidden 64 --bf16]

--synthetic: a random directed graph; node features are noise about a constant and say nothing about the label; every edge into
node i carries a noisy one-hot code of i's label as its attribute row.  A model that reads the edge attributes classifies almost
perfectly, one that does not is at chance: the script prints the accuracy with the real attributes and with them zeroed.  Adam;
--bf16 keeps the activations in bf16 (fp32 parameters).

Every layer aggregates with ONE autograd node (ops_ef.u_op_e_sum): relu(h_j + e_ij), or h_j * w_ij, is formed in registers per edge
and no [nnz, F] message tensor exists; the projected edge features themselves are a real [nnz, F] array.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from dgll_amd import ops_ef  # noqa: E402
from dgll_amd.nn.Convolution import GINE, CFConv  # noqa: E402


def edge_signal_graph(n, k, degree, edge_width, seed, device):
    """(graph, labels, node features, edge attributes in the graph's entry order)"""
    gen = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, k, (n,), generator=gen)
    src, dst = torch.randint(0, n, (n * degree,), generator=gen), torch.randint(0, n, (n * degree,), generator=gen)
    attr = torch.nn.functional.one_hot(labels[dst], edge_width).float() + 0.7 * torch.randn(n * degree, edge_width, generator=gen)
    graph, attr, _ = ops_ef.edge_graph_from_coo(src, dst, attr, n_dst=n, n_src=n)
    x = 1.0 + 0.5 * torch.randn(n, 16, generator=gen)
    return graph.to(device), labels.to(device), x.to(device), attr.to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--layer", choices=("gine", "cfconv"), default="gine")
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
    if args.layer == "gine":
        model = GINE(x.shape[1], edge_width, args.hidden, args.classes, n_layers=args.layers).to(dev)
    else:
        model = CFConv(x.shape[1], edge_width, args.hidden, args.classes).to(dev)       # its outputs are the logits
    graph.transpose()
    print("%s on %d nodes, %d entries: the projected edge features are %.1f MB per layer, no message tensor is formed" %
          (args.layer, graph.n_rows, graph.nnz, 1e-6 * graph.nnz * args.hidden * x.element_size()))
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
        if epoch % 10 == 0 or epoch == args.epochs - 1:
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
