#!/usr/bin/env python3
"""examples/gine/train.py's task with the edge projection fused into the aggregation: nn.GINE(fused_edge=True).

    python examples/gine/train_fused.py --synthetic [--nodes 20000 --classes 8 --degree 10 --hidden 64 --bf16 --unfused]

--synthetic: the edge-signal graph of train.py (node features say nothing about the label, every edge into node i carries a noisy
one-hot code of i's label): a model that reads the edge attributes classifies almost perfectly, one that does not is at chance.

Every layer hands the RAW edge attributes [nnz, 8] and its encoder's weight and bias to ONE autograd node
(ops_efp.u_op_proj_e_sum): e_ij = enc(a_ij) is formed per entry in registers, in the forward and again in the backward, so neither the
projected edge features nor their gradient exist as [nnz, hidden] arrays.  The script prints the peak memory of a training step
above the model and the data; --unfused runs the same model (same parameters, same state dict) with a Linear per layer instead, for
comparison.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from dgll_amd.nn.Convolution import GINE  # noqa: E402
from train import edge_signal_graph  # noqa: E402


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
    ap.add_argument("--unfused", action="store_true")
    args = ap.parse_args()
    if not args.synthetic:
        raise SystemExit("pass --synthetic (the edge-signal graph is the only data source of this example)")
    if not torch.cuda.is_available():
        raise SystemExit("this example runs the HIP kernels: a GPU is required")
    if args.classes > 16:
        raise SystemExit("the fused projection takes edge attributes of at most 16 columns (one per class here)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    edge_width = max(8, args.classes)
    graph, labels, x, attr = edge_signal_graph(args.nodes, args.classes, args.degree, edge_width, 0, dev)
    if args.bf16:
        x, attr = x.to(torch.bfloat16), attr.to(torch.bfloat16)
    model = GINE(x.shape[1], edge_width, args.hidden, args.classes, n_layers=args.layers, fused_edge=not args.unfused).to(dev)
    graph.transpose()
    print("gine (%s) on %d nodes, %d entries: the edge attributes are %.2f MB, one [nnz, hidden] array would be %.1f MB" %
          ("unfused" if args.unfused else "fused edge projection", graph.n_rows, graph.nnz, 1e-6 * attr.numel() * attr.element_size(),
           1e-6 * graph.nnz * args.hidden * x.element_size()))
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    peak = 0
    for epoch in range(args.epochs):
        model.train()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t0 = time.time()
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(graph, x, attr).float(), labels)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        dt = time.time() - t0
        if epoch:                                   # the first step also allocates Adam's state
            peak = max(peak, torch.cuda.max_memory_allocated() - before)
        if epoch % 10 == 0 or epoch == args.epochs - 1:
            model.eval()
            with torch.no_grad():
                pred = model(graph, x, attr).argmax(1)
            print("epoch %3d  loss %.4f  acc %.3f  %.1f ms" % (epoch, loss.item(), (pred == labels).float().mean().item(), dt * 1e3))
    model.eval()
    with torch.no_grad():
        real = (model(graph, x, attr).argmax(1) == labels).float().mean().item()
        zeroed = (model(graph, x, torch.zeros_like(attr)).argmax(1) == labels).float().mean().item()
    print("peak memory of a training step above the model and the data: %.2f MB" % (1e-6 * peak))
    print("accuracy with the edge attributes %.3f, with them zeroed %.3f (chance %.3f)" % (real, zeroed, 1.0 / args.classes))


if __name__ == "__main__":
    main()
