#!/usr/bin/env python3
"""Node classification with Principal Neighbourhood Aggregation (nn.PNA: a linear embedding, PNAConv layers, a linear classifier):

    python examples/pna/train.py --synthetic [--nodes 20000 --communities 8 --hidden 64 --towers 4 --layers 2 --bf16]

--synthetic: the planted-community graph of examples/message_passing/train.py with noisy one-hot-ish features; every node trains.
delta, the normaliser of the degree scalers, is ops_agg.pna_delta(graph): the mean of log(degree + 1) over the training graph.  Adam;
--bf16 keeps the activations BETWEEN the layers in bf16 (fp32 parameters; a PNAConv works in fp32 inside and rounds its output once).

Every layer aggregates with ONE autograd node (ops_agg.multi_aggregate): the four aggregators and three scalers come from a single
gather of the source term per edge, and no per-edge message tensor exists.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from dgll_amd import ops_agg, synth  # noqa: E402
from dgll_amd.nn.Convolution import PNA  # noqa: E402


def planted(n, k, avg_in, avg_out, seed, device):
    """Symmetric planted-community graph with self-loops and (labels, features): node v belongs to community v % k."""
    gen = torch.Generator().manual_seed(seed)
    labels = torch.arange(n) % k
    m_in, m_out = n * avg_in // 2, n * avg_out // 2
    src_in = torch.randint(0, n, (m_in,), generator=gen)
    dst_in = (torch.randint(0, n // k, (m_in,), generator=gen) * k + src_in % k).clamp(max=n - 1)       # same community
    src_out, dst_out = torch.randint(0, n, (m_out,), generator=gen), torch.randint(0, n, (m_out,), generator=gen)
    graph = synth.build_graph(torch.cat([src_in, src_out]), torch.cat([dst_in, dst_out]), n, symmetric=True, self_loops=True, weighted=False)
    width = max(16, k)
    x = torch.nn.functional.one_hot(labels, width).float() + torch.randn(n, width, generator=gen)
    return graph.to(device), labels.to(device), x.to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--nodes", type=int, default=20_000)
    ap.add_argument("--communities", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--towers", type=int, default=4)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--dropout", type=float, default=0.0)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--weight-decay", type=float, default=5e-4)
    ap.add_argument("--bf16", action="store_true")
    args = ap.parse_args()
    if not args.synthetic:
        raise SystemExit("pass --synthetic (the planted-community graph is the only data source of this example)")
    if not torch.cuda.is_available():
        raise SystemExit("this example runs the HIP kernels: a GPU is required")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    graph, labels, x = planted(args.nodes, args.communities, 12, 3, 0, dev)
    if args.bf16:
        x = x.to(torch.bfloat16)
    nclass = int(labels.max()) + 1
    delta = ops_agg.pna_delta(graph)
    model = PNA(x.shape[1], args.hidden, nclass, n_layers=args.layers, delta=delta, dropout=args.dropout, num_towers=args.towers).to(dev)
    graph.transpose()
    print("PNA on %d nodes, %d entries, delta %.4f: a per-edge message tensor would be %.1f MB per tower, none is formed" %
          (graph.n_rows, graph.nnz, delta, 4e-6 * graph.nnz * args.hidden / args.towers))
    opt = torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
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
        if epoch % 10 == 0 or epoch == args.epochs - 1:
            model.eval()
            with torch.no_grad():
                pred = model(graph, x).argmax(1)
            print("epoch %3d  loss %.4f  acc %.3f  %.1f ms" % (epoch, loss.item(), (pred == labels).float().mean().item(), dt * 1e3))


if __name__ == "__main__":
    main()
