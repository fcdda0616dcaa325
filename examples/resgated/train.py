#!/usr/bin/env python3
"""Node classification on a graph where a node's label is written in its NEIGHBOURS' features, with nn.ResGatedGCN
(ResGatedGraphConv layers: Bresson & Laurent's residual gated graph convnet in PyG's form, without edge features):

    python examples/resgated/train.py --synthetic [--nodes 20000 --classes 8 --degree 10 --hidden 64 --layers 2 --epochs 100 --bf16]

--synthetic: every node j has a random type t_j, and its feature row is a noisy one-hot code of t_j; every node i has a random label
y_i that its own features say nothing about.  Four in five of the edges into i come from nodes of type y_i, the others from anywhere:
the label is the type most of the neighbours have.  A model that aggregates recovers the label of most nodes (0.88 after 60 epochs
at the defaults, still rising); the script also prints the accuracy on the same nodes with every edge removed, which is at chance.
Adam; --bf16 keeps the activations in bf16 (fp32 parameters).

Every layer aggregates with ONE autograd node (ops_res_gated.res_gated_sum): the gate sigmoid(k_i + q_j) is recomputed from two node
rows in every pass, so nothing of the size of the edge list is stored, in the forward or in the backward.
"""
import argparse
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from dgll_amd import CSRGraph  # noqa: E402
from dgll_amd.nn.Convolution import ResGatedGCN  # noqa: E402


def neighbour_signal_graph(n, classes, degree, width, seed, device):
    """(graph, labels, node features): 1 to 2 * degree - 1 entries a row, 80 % of them from sources whose type is the row's label"""
    gen = torch.Generator().manual_seed(seed)
    labels, types = torch.randint(0, classes, (n,), generator=gen), torch.randint(0, classes, (n,), generator=gen)
    deg = torch.randint(1, 2 * degree, (n,), generator=gen)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    torch.cumsum(deg, 0, out=rowptr[1:])
    want = labels.repeat_interleave(deg)                                    # per entry: the type its source should have
    order, counts = torch.argsort(types, stable=True), torch.bincount(types, minlength=classes)
    start = torch.cumsum(counts, 0) - counts
    pick = (start[want] + (torch.rand(len(want), generator=gen) * counts[want]).long()).clamp(max=n - 1)
    anywhere = torch.randint(0, n, (len(want),), generator=gen)
    col = torch.where((torch.rand(len(want), generator=gen) < 0.8) & (counts[want] > 0), order[pick], anywhere)
    x = torch.nn.functional.one_hot(types, width).float() + 0.7 * torch.randn(n, width, generator=gen)
    return CSRGraph(rowptr, col.to(torch.int32), None, n, n).to(device), labels.to(device), x.to(device)


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
    ap.add_argument("--aggr", choices=("mean", "add"), default="mean")
    ap.add_argument("--bf16", action="store_true")
    args = ap.parse_args()
    if not args.synthetic:
        raise SystemExit("pass --synthetic (the neighbour-signal graph is the only data source of this example)")
    if not torch.cuda.is_available():
        raise SystemExit("this example runs the HIP kernels: a GPU is required")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    graph, labels, x = neighbour_signal_graph(args.nodes, args.classes, args.degree, max(8, args.classes), 0, dev)
    if args.bf16:
        x = x.to(torch.bfloat16)
    model = ResGatedGCN(x.shape[1], args.hidden, args.classes, layers=args.layers, aggr=args.aggr).to(dev)
    graph.transpose()
    graph.inv_degrees()
    print("resgated on %d nodes, %d entries: one [nnz, hidden] array would be %.1f MB, and none is formed" %
          (graph.n_rows, graph.nnz, 1e-6 * graph.nnz * args.hidden * x.element_size()))
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    for epoch in range(args.epochs):
        model.train()
        torch.cuda.synchronize()
        t0 = time.time()
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(graph, x).float(), labels)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        dt = time.time() - t0
        model.eval()
        with torch.no_grad():
            pred = model(graph, x).argmax(1)
        print("epoch %3d  loss %.4f  acc %.3f  %.1f ms" % (epoch, loss.item(), (pred == labels).float().mean().item(), dt * 1e3))
    model.eval()
    no_edges = CSRGraph(torch.zeros(graph.n_rows + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None, graph.n_rows,
                        graph.n_cols).to(dev)
    with torch.no_grad():
        real = (model(graph, x).argmax(1) == labels).float().mean().item()
        alone = (model(no_edges, x).argmax(1) == labels).float().mean().item()
    print("accuracy with the neighbours %.3f, with every edge removed %.3f (chance %.3f)" % (real, alone, 1.0 / args.classes))


if __name__ == "__main__":
    main()
