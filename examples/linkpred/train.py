#!/usr/bin/env python3
"""Link prediction with GraphSAGE-mean on device-sampled blocks -- DGL's
`as_edge_prediction_sampler(NeighborSampler(fanouts), negative_sampler=GlobalUniform(5), exclude="reverse_id")` loop with a
dot-product predictor, on the synthetic products-shaped graph of examples/neighbor/train.py (same model, same generator).

10 % of the undirected edges are held out: both directions are removed from the training graph.  A training batch is a set of
edge ids of the training graph; EdgePredictionSampler turns it into positive pairs, 5 uniform negatives each (candidates that are
real edges are redrawn), the unique endpoint list and its blocks with the batch's own edges and their reverses taken out, all on
the GPU.  The model embeds the endpoints, ops.pair_dot scores the pairs, the loss is binary cross-entropy with logits.  After
every epoch: the mean loss and the AUC of held-out edges against as many uniform non-edges (rank statistic).

    python examples/linkpred/train.py --nodes 200000 --fanouts 10,25 --batch 1024 --epochs 3
"""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from dgll_amd import ops, synth  # noqa: E402
from dgll_amd.cache import gather_rows  # noqa: E402
from dgll_amd.graph import CSRGraph  # noqa: E402
from dgll_amd.sampling import EdgePredictionSampler, NeighborSampler, layerwise  # noqa: E402


def neighbor_example():
    """examples/neighbor/train.py as a module: its SageMean model is this example's encoder."""
    spec = importlib.util.spec_from_file_location("neighbor_example_train", os.path.join(ROOT, "examples", "neighbor", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SageMean = neighbor_example().SageMean


def hold_out(g, fraction, seed):
    """(training graph, held-out pairs int64[H, 2]): a seeded `fraction` of the undirected edges u < v leaves the graph in BOTH
    directions.  g: symmetric CSR with sorted rows, on the device."""
    n = g.n_rows
    row = g.row_index()
    col = g.col.to(torch.int64)
    upper = torch.nonzero(col < row).flatten()                                   # every undirected edge once (col -> row, col < row)
    gen = torch.Generator(device=g.device)
    gen.manual_seed(seed)
    pick = upper[torch.randperm(upper.numel(), generator=gen, device=g.device)[:int(upper.numel() * fraction)]]
    held = torch.stack([col[pick], row[pick]], 1)
    gone = torch.cat([held[:, 1] * n + held[:, 0], held[:, 0] * n + held[:, 1]])
    keep = ~torch.isin(row * n + col, gone)
    below = torch.zeros(g.nnz + 1, dtype=torch.int64, device=g.device)
    below[1:] = torch.cumsum(keep, 0)
    return CSRGraph(below[g.rowptr], g.col[keep].contiguous(), None, n, n), held


def auc(pos, neg):
    """P(score of a positive > score of a negative) + P(equal) / 2, by ranks (Mann-Whitney U), in torch."""
    s = torch.cat([pos, neg]).double()
    order = torch.argsort(s)
    rank = torch.empty_like(s)
    rank[order] = torch.arange(1, s.numel() + 1, dtype=torch.float64, device=s.device)
    uniq, inv, cnt = torch.unique(s, return_inverse=True, return_counts=True)    # ties share their mean rank
    mean_rank = torch.zeros(uniq.numel(), dtype=torch.float64, device=s.device).index_add_(0, inv, rank) / cnt
    rank = mean_rank[inv]
    n_pos, n_neg = pos.numel(), neg.numel()
    return float((rank[:n_pos].sum() - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg))


@torch.no_grad()
def evaluate(model, sampler, feats, held, n, batch, seed):
    """AUC of the held-out edges against as many pairs (u, uniform node); embeddings from blocks of the training graph."""
    gen = torch.Generator(device=held.device)
    gen.manual_seed(seed)
    pos_s, neg_s = [], []
    for i in range(0, held.shape[0], batch):
        pos = held[i:i + batch]
        neg = torch.stack([pos[:, 0], torch.randint(0, n, (pos.shape[0],), generator=gen, device=held.device)], 1)
        nodes, local = torch.unique(torch.cat([pos, neg]).reshape(-1), return_inverse=True)
        inp, _, blocks = sampler.sample_seeded(None, nodes, seed + i)
        h = model(blocks, gather_rows(feats, inp))
        score = ops.pair_dot(h, local.reshape(-1, 2).to(torch.int32))
        pos_s.append(score[:pos.shape[0]])
        neg_s.append(score[pos.shape[0]:])
    return auc(torch.cat(pos_s), torch.cat(neg_s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200_000)
    ap.add_argument("--avg-degree", type=int, default=50)
    ap.add_argument("--feats", type=int, default=100)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--embed", type=int, default=64)
    ap.add_argument("--batch", type=int, default=1024, help="positive edges per batch")
    ap.add_argument("--batches", type=int, default=200, help="batches per epoch (a seeded sample of the training edges)")
    ap.add_argument("--negatives", type=int, default=5)
    ap.add_argument("--fanouts", default="10,25", help="DGL's order: the last entry is applied to the seeds first; -1 = every neighbour")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--eval-edges", type=int, default=20_000)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this example runs the HIP kernels: a GPU is required")
    dev = torch.device("cuda:0")
    np.random.seed(args.seed)                    # sample() draws its per-batch seed from numpy's global generator
    torch.manual_seed(args.seed)
    full = synth.products_like_graph(dev, seed=0, n=args.nodes, n_undirected=args.nodes * args.avg_degree // 2, locality=0.9)
    n = full.n_rows
    g, held = hold_out(full, 0.1, args.seed)
    held = held[:args.eval_edges]
    community = torch.arange(n) * 64 // n
    feats = (torch.randn(n, args.feats) + torch.nn.functional.one_hot(community % args.feats, args.feats) * 2.0).to(dev)
    fanouts = [int(f) for f in args.fanouts.split(",")]
    blocks_of = NeighborSampler(fanouts, g)
    sampler = EdgePredictionSampler(blocks_of, negatives=args.negatives, filter_existing=True, exclude="reverse")
    model = SageMean(args.feats, args.hidden, args.embed, layers=len(fanouts)).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    cur = torch.cuda.current_stream(dev)
    print("graph: %d nodes, %d training entries, %d held-out edges (%d evaluated)" % (n, g.nnz, int(full.nnz - g.nnz) // 2, held.shape[0]),
          flush=True)
    for epoch in range(args.epochs):
        edges = torch.randint(0, g.nnz, (args.batches * args.batch,), device=dev)
        t0, total, capped, drawn, seen = time.time(), 0.0, 0, 0, 0
        for i in range(0, edges.numel(), args.batch):
            inp, batch, blocks = sampler.sample(None, edges[i:i + args.batch])
            # the blocks, the pairs and the input ids come from the sampler's stream: tell the allocator they are used on this one
            batch.record_stream(cur)
            layerwise.record_stream(blocks, inp, cur)
            h = model(blocks, gather_rows(feats, inp))
            loss = torch.nn.functional.binary_cross_entropy_with_logits(ops.pair_dot(h, batch), batch.labels())
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            total += float(loss) * len(batch)
            seen += len(batch)
            capped += batch.capped
            drawn += batch.n_neg
        torch.cuda.synchronize()
        score = evaluate(model, blocks_of, feats, held, n, 4096, args.seed + 1)
        print("epoch %d  loss %.4f  held-out auc %.4f  capped negatives %d of %d  %.2f s"
              % (epoch, total / max(seen, 1), score, capped, drawn, time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
