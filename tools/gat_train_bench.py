#!/usr/bin/env python3
"""BASELINE config 4 shape on one GPU: 2-layer SpGAT (8 heads x 32 -> 47 classes) full-graph training step on the
products-shaped graph, bf16 activations.  Prints the step time (median over --reps repetitions of --steps steps, with the
repetitions' spread) and the per-pass times of the GAT gather kernels from the launch timer.

    python tools/gat_train_bench.py [locality] [reorder] [--dropout P] [--reps R] [--steps S] [--nodes N --edges E]

--dropout P: SpGAT(dropout=P) in training mode -- input dropout plus attention dropout, drawn inside the gather kernels
(DGLL_GAT_DROPOUT=mask in the environment: the materialised [nnz, heads] mask on the first-generation kernels)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dgll_amd import nn as dnn  # noqa: E402
from dgll_amd import ops, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("locality", nargs="?", type=float, default=0.9)
ap.add_argument("reorder", nargs="?", default="lpa")
ap.add_argument("--dropout", type=float, default=0.0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--nodes", type=int, default=synth.PRODUCTS_NODES)
ap.add_argument("--edges", type=int, default=synth.PRODUCTS_UNDIRECTED_EDGES, help="undirected edges before symmetrisation")
args = ap.parse_args()

dev = torch.device("cuda:0")
loc, reorder = args.locality, args.reorder
g = synth.products_like_graph(dev, seed=0, n=args.nodes, n_undirected=args.edges, locality=loc, self_loops=True, exact=True,
                              permute_ids=True)   # bench.py's graph + I
if reorder != "none":
    g = g.reorder(method=reorder, seed=0)[0]
n = g.n_rows
torch.manual_seed(0)
model = dnn.SpGAT(100, 32, 47, dropout=args.dropout, alpha=0.2, nheads=8).to(dev)
x = ops.alloc_features(n, 100, torch.bfloat16, dev, pad_to=64)
x.copy_(torch.randn(n, 100, device=dev))
labels = torch.randint(0, 47, (n,), device=dev)
opt = torch.optim.Adam(model.parameters(), lr=1e-3)


def step():
    opt.zero_grad(set_to_none=True)
    out = model(x, g)                       # log_softmax output
    loss = -out.float().gather(1, labels.unsqueeze(1)).sum() / n
    loss.backward()
    opt.step()
    return loss


for _ in range(3):
    step()
torch.cuda.synchronize()
times = []
for _ in range(args.reps):
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    times.append((time.perf_counter() - t0) / args.steps * 1e3)
torch.cuda.reset_peak_memory_stats()
step()
torch.cuda.synchronize()
peak = torch.cuda.max_memory_allocated() / 2 ** 30
mode = os.environ.get("DGLL_GAT_DROPOUT", "kernel") if args.dropout > 0 else "-"
print("SpGAT 100 -> 8x32 -> 47, products-shaped (locality %.1f, nnz %d), dropout %.2f (%s): median %.2f ms/step (fwd+bwd+Adam), "
      "min %.2f max %.2f over %d x %d steps, peak %.2f GiB, loss %.3f"
      % (loc, g.nnz, args.dropout, mode, statistics.median(times), min(times), max(times), args.reps, args.steps, peak,
         float(loss.detach())))
with ops.LaunchTimer() as timer:
    for _ in range(3):
        step()
for tag, (count, ms) in sorted(timer.summary().items(), key=lambda kv: str(kv[0])):
    if tag[0] == "gat":
        print("  %-10s heads %d x %d  %-18s %.3f ms (%d launches)" % (tag[1], tag[2], tag[3], tag[-1] or "strided", ms, count))
