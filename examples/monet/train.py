#!/usr/bin/env python3
"""Node classification on a graph whose PSEUDO-COORDINATES carry the signal, with nn.MoNet (GMMConv layers, each with its own
Linear(2, dim) + Tanh over the raw coordinates):

    python examples/monet/train.py --synthetic [--nodes 20000 --classes 6 --degree 10 --hidden 64 --kernels 6 --dim 2 --bf16]

--synthetic: a random directed graph; node features are noise about a constant and say nothing about the label; every edge into
node i carries a 2-d coordinate drawn about the point of i's class on a circle.  A model whose Gaussian kernels learn where the
classes sit classifies well, one that sees the same coordinate on every edge is at chance: the script prints the accuracy with the
real coordinates and with them held constant.  Adam; --bf16 keeps the activations in bf16 (fp32 parameters and coordinates).

Every layer aggregates with ONE autograd node (ops_gmm.gmm_expand): the K Gaussian weights of an edge are computed in registers from
its coordinates and no [nnz, K, out] message tensor exists; the backward's one per-edge scratch is the fp32 [nnz, K] dot products.
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from dgll_amd import ops_ef  # noqa: E402
from dgll_amd.nn.Convolution import MoNet  # noqa: E402


def pseudo_signal_graph(n, k, degree, seed, device):
    """(graph, labels, node features, pseudo-coordinates [nnz, 2] in the graph's entry order)"""
    gen = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, k, (n,), generator=gen)
    src, dst = torch.randint(0, n, (n * degree,), generator=gen), torch.randint(0, n, (n * degree,), generator=gen)
    angle = labels[dst].float() * (2.0 * math.pi / k)
    pseudo = 0.8 * torch.stack([torch.cos(angle), torch.sin(angle)], 1) + 0.25 * torch.randn(n * degree, 2, generator=gen)
    graph, pseudo, _ = ops_ef.edge_graph_from_coo(src, dst, pseudo, n_dst=n, n_src=n)
    x = 1.0 + 0.5 * torch.randn(n, 16, generator=gen)
    return graph.to(device), labels.to(device), x.to(device), pseudo.to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--nodes", type=int, default=20_000)
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--degree", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--kernels", type=int, default=6)
    ap.add_argument("--dim", type=int, default=2)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--bf16", action="store_true")
    args = ap.parse_args()
    if not args.synthetic:
        raise SystemExit("pass --synthetic (the pseudo-coordinate graph is the only data source of this example)")
    if not torch.cuda.is_available():
        raise SystemExit("this example runs the HIP kernels: a GPU is required")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    graph, labels, x, pseudo = pseudo_signal_graph(args.nodes, args.classes, args.degree, 0, dev)
    if args.bf16:
        x = x.to(torch.bfloat16)
    model = MoNet(x.shape[1], args.hidden, args.classes, dim=args.dim, n_kernels=args.kernels, n_layers=args.layers,
                  aggregator_type="mean")
    for layer in model.layers:      # the kernels start spread over the range of tanh, not at DGL's N(0, 0.1) about the origin: from there
        torch.nn.init.uniform_(layer.mu, -1.0, 1.0)     # all K weights of an edge are alike and the first steps see almost no signal
        torch.nn.init.constant_(layer.inv_sigma, 2.0)
    model = model.to(dev)
    graph.transpose()
    print("MoNet on %d nodes, %d entries, %d kernels: the backward's per-edge scratch is %.1f MB per layer; a message tensor would be %.1f MB" %
          (graph.n_rows, graph.nnz, args.kernels, 1e-6 * graph.nnz * 4 * ((args.kernels + 3) // 4 * 4),
           1e-6 * graph.nnz * args.kernels * args.hidden * x.element_size()))
    constant = torch.zeros_like(pseudo)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    for epoch in range(args.epochs):
        model.train()
        torch.cuda.synchronize()
        t0 = time.time()
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(graph, x, pseudo).float(), labels)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        dt = time.time() - t0
        if epoch % 10 == 0 or epoch == args.epochs - 1:
            model.eval()
            with torch.no_grad():
                pred = model(graph, x, pseudo).argmax(1)
            print("epoch %3d  loss %.4f  acc %.3f  %.1f ms" % (epoch, loss.item(), (pred == labels).float().mean().item(), dt * 1e3))
    model.eval()
    with torch.no_grad():
        real = (model(graph, x, pseudo).argmax(1) == labels).float().mean().item()
        held = (model(graph, x, constant).argmax(1) == labels).float().mean().item()
    print("accuracy with the pseudo-coordinates %.3f, with them held constant %.3f (chance %.3f)" % (real, held, 1.0 / args.classes))


if __name__ == "__main__":
    main()
