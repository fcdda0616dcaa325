#!/usr/bin/env python3
"""Node classification on a graph where a node's label is the class of its STRONGEST neighbour, with nn.DeeperGCN (GENConv layers in
res+ blocks: Li et al., "DeeperGCN: All You Need to Train Deeper GCNs"):

    python examples/deepergcn/train.py --synthetic [--aggr softmax|power --nodes 20000 --classes 8 --degree 10 --hidden 64 --layers 3
                                                    --epochs 100 --bf16]

--synthetic: every node j has a random class c_j and a random strength s_j in [0.2, 3]; its feature row is s_j times the one-hot code
of c_j, plus a little noise.  The label of node i is the class of the neighbour with the LARGEST feature norm -- something a mean of
the neighbours cannot read (it sees which class has the most mass, not which node is the strongest), and a softmax with a large
inverse temperature t, or a power mean with a large p, can.  The script trains the model with a learned t (or p), prints the loss per
epoch, and at the end the accuracy next to that of the same model with t frozen at 0 (p frozen at 1), which is the mean, and the
learned values.  Adam; --bf16 keeps the activations in bf16 (fp32 parameters).

Every layer aggregates with ONE autograd node (ops_softagg): per column an online softmax (or a power sum) over the row's messages,
nothing of the size of the edge list stored, and t / p read by the kernels through a pointer, never by the host.
"""
import argparse
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from dgll_amd import CSRGraph  # noqa: E402
from dgll_amd.nn.Convolution import DeeperGCN  # noqa: E402


def strongest_neighbour_graph(n, classes, degree, seed, device):
    """(graph, labels, node features): 2 to 2 * degree - 1 random entries a row; the label is the class of the row's strongest source"""
    gen = torch.Generator().manual_seed(seed)
    cls = torch.randint(0, classes, (n,), generator=gen)
    strength = 0.2 + 2.8 * torch.rand(n, generator=gen)
    deg = torch.randint(2, 2 * degree, (n,), generator=gen)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    torch.cumsum(deg, 0, out=rowptr[1:])
    col = torch.randint(0, n, (int(rowptr[-1]),), generator=gen)
    row = torch.repeat_interleave(torch.arange(n), deg)
    top = torch.zeros(n).scatter_reduce(0, row, strength[col], "amax", include_self=False)
    winner = torch.zeros(n, dtype=torch.int64).scatter_reduce(0, row, torch.where(strength[col] == top[row], col, -1), "amax",
                                                               include_self=False)
    x = strength.unsqueeze(1) * torch.nn.functional.one_hot(cls, classes).float() + 0.05 * torch.randn(n, classes, generator=gen)
    return CSRGraph(rowptr, col.to(torch.int32), None, n, n).to(device), cls[winner].to(device), x.to(device)


def train(model, graph, x, labels, epochs, lr, quiet=False):
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    for epoch in range(epochs):
        model.train()
        torch.cuda.synchronize()
        t0 = time.time()
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(graph, x).float(), labels)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        if not quiet:
            print("epoch %3d  loss %.4f  %.1f ms" % (epoch, loss.item(), (time.time() - t0) * 1e3))
    model.eval()
    with torch.no_grad():
        return (model(graph, x).argmax(1) == labels).float().mean().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--nodes", type=int, default=20_000)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--degree", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--aggr", choices=("softmax", "power"), default="softmax")
    ap.add_argument("--bf16", action="store_true")
    args = ap.parse_args()
    if not args.synthetic:
        raise SystemExit("pass --synthetic (the strongest-neighbour graph is the only data source of this example)")
    if not torch.cuda.is_available():
        raise SystemExit("this example runs the HIP kernels: a GPU is required")
    dev = torch.device("cuda:0")
    graph, labels, x = strongest_neighbour_graph(args.nodes, args.classes, args.degree, 0, dev)
    if args.bf16:
        x = x.to(torch.bfloat16)
    graph.transpose()
    name, start, mean_at = ("t", 1.0, 0.0) if args.aggr == "softmax" else ("p", 2.0, 1.0)
    print("deepergcn (%s) on %d nodes, %d entries: one [nnz, hidden] array would be %.1f MB, and none is formed" %
          (args.aggr, graph.n_rows, graph.nnz, 1e-6 * graph.nnz * args.hidden * x.element_size()))

    def make(value, learn):
        torch.manual_seed(0)
        return DeeperGCN(x.shape[1], args.hidden, args.classes, args.layers, aggr=args.aggr, t=value, learn_t=learn, p=value,
                         learn_p=learn).to(dev)

    model = make(start, True)
    learned = train(model, graph, x, labels, args.epochs, args.lr)
    frozen = train(make(mean_at, False), graph, x, labels, args.epochs, args.lr, quiet=True)
    values = " ".join("%.4f" % getattr(conv.aggr_module, name).item() for conv in model.convs)
    print("accuracy with the learned %s %.3f, with %s frozen at %g (the mean) %.3f (chance %.3f)" %
          (name, learned, name, mean_at, frozen, 1.0 / args.classes))
    print("learned %s per layer, from %.4f: %s" % (name, start, values))


if __name__ == "__main__":
    main()
