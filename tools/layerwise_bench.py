#!/usr/bin/env python3
"""Layer-wise sampler benchmark: prints ONE JSON line.

    python tools/layerwise_bench.py --sampler ladies --graph products [--batch 1023 --fanouts 512,1024 --hidden 128]

Reports, on a synthetic graph (products-shaped: synth.products_like_graph defaults; reddit-shaped: the configuration-2 graph,
232 965 nodes, 57.3 M undirected edges):
  sampler_ms_device   device time of one sample() on the sampler's stream (events), median over --batches
  sampler_ms_host     host wall time of one sample() (it returns after its stream finished), median
  e2e_batches_per_s   DataLoader + MiniBatchPipeline (GraphCacheServer, half the rows cached) + the reference's 2-layer GCN
                      (hidden --hidden, Adam, cross-entropy): batches per second over --batches
  cpu_scipy_ms        the reference's host algorithm restated with scipy / numpy (tests/layerwise_ref.py does the same) on the
                      same normalised adjacency, median over --cpu-batches
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dgll_amd import ops, synth  # noqa: E402
from dgll_amd.cache import GraphCacheServer  # noqa: E402
from dgll_amd.data import DGraph  # noqa: E402
from dgll_amd.dataloader import DataLoader  # noqa: E402
from dgll_amd.nn import gcnConv  # noqa: E402
from dgll_amd.pipeline import MiniBatchPipeline  # noqa: E402
from dgll_amd.sampling import layerwise as lw  # noqa: E402

GRAPHS = {"products": dict(n=synth.PRODUCTS_NODES, n_undirected=synth.PRODUCTS_UNDIRECTED_EDGES, feats=100, classes=47),
          "reddit": dict(n=232_965, n_undirected=57_300_000, feats=602, classes=41)}


class Model(torch.nn.Module):
    def __init__(self, fin, hid, ncls):
        super().__init__()
        self.conv1, self.conv2 = gcnConv(fin, hid), gcnConv(hid, ncls)

    def forward(self, blocks, x):
        return self.conv2(torch.relu(self.conv1(x, blocks[0])), blocks[1])


def cpu_restatement(L, batch, fanouts, ladies, rng):
    """The reference's sample() (MQLadies.py:73-89 / MQFastGCN.py:68-88, fix (b) applied) with scipy on the host."""
    n = L.shape[0]
    rows = batch
    p_global = None
    if not ladies:
        p_global = np.asarray(L.multiply(L).sum(0)).flatten()
        p_global /= p_global.sum()
    t0 = time.perf_counter()
    for f in fanouts:
        Q = L[rows, :]
        if ladies:
            p = np.asarray(Q.multiply(Q).sum(0)).flatten()
            p /= p.sum()
        else:
            p = p_global
        s = int(min(np.sum(p > 0), f))
        draw = rng.choice(n, s, replace=False, p=p)
        if ladies:
            w = np.zeros(s)
            psum = 0.0
            for i in range(s):
                alpha = n / (i + 1) / (n - i)
                w[i] = (1 - psum) / p[draw[i]] * alpha
                w[:i] = w[:i] * (1 - alpha) + alpha
                psum += p[draw[i]]
            cols = draw
        else:
            cols = np.unique(np.concatenate((draw, batch)))
            w = 1 / p[cols] / s
        Q[:, cols].multiply(w).tocsr()
        rows = cols
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sampler", choices=["ladies", "fastgcn"], default="ladies")
    ap.add_argument("--graph", choices=sorted(GRAPHS), default="products")
    ap.add_argument("--batch", type=int, default=1023)
    ap.add_argument("--fanouts", default="512,1024")
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-batches", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    spec = GRAPHS[args.graph]
    fanouts = [int(f) for f in args.fanouts.split(",")]
    g = synth.products_like_graph(dev, seed=1, n=spec["n"], n_undirected=spec["n_undirected"], locality=0.0)
    n = g.n_rows
    t0 = time.perf_counter()
    s = (lw.Ladies if args.sampler == "ladies" else lw.FastGCNSampler)(fanouts, g)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    rng = np.random.default_rng(0)
    dev_ms, host_ms = [], []
    for i in range(args.warmup + args.batches):
        batch = rng.choice(n, args.batch, replace=False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        h0 = time.perf_counter()
        e0.record(s.stream)
        s.sample_seeded(None, batch, i)
        e1.record(s.stream)
        h1 = time.perf_counter()
        e1.synchronize()
        if i >= args.warmup:
            dev_ms.append(e0.elapsed_time(e1))
            host_ms.append((h1 - h0) * 1e3)
    # end to end through the pipeline
    torch.manual_seed(0)
    feats = torch.randn(n, spec["feats"])
    labels = torch.randint(0, spec["classes"], (n,))
    indptr, indices = g.rowptr.cpu().numpy(), g.col.cpu().numpy().astype(np.int64)
    dg = DGraph.from_csr(indptr, indices, labels=labels, features=feats)
    srv = GraphCacheServer(feats, gpuid=0)
    srv.auto_cache(g.degrees().cpu(), capacity=n // 2)
    model = Model(spec["feats"], args.hidden, spec["classes"]).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    train = torch.randperm(n)[:args.batch * (args.warmup + args.batches)]
    loader = DataLoader(dg, train, s, batch_size=args.batch)
    pipe = MiniBatchPipeline(loader, cache=srv, labels=labels, queue_size=4, device=dev)
    cur = torch.cuda.current_stream(dev)
    t_start, done = None, 0
    for k, b in enumerate(pipe):
        if k == args.warmup:
            torch.cuda.synchronize()
            t_start = time.perf_counter()
        lw.record_stream(b.subgraphs, b.input_nodes, cur)
        loss = ops.cross_entropy(model(b.subgraphs, b.features[0]), b.labels)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        if k >= args.warmup:
            done += 1
    torch.cuda.synchronize()
    e2e = done / (time.perf_counter() - t_start) if done else 0.0
    # host restatement on the same normalised adjacency
    L = s.lap
    Lc = sp.csr_matrix((L.val.double().cpu().numpy(), L.col.cpu().numpy(), L.rowptr.cpu().numpy()), shape=(n, n))
    cpu_ms = [cpu_restatement(Lc, rng.choice(n, args.batch, replace=False), fanouts, args.sampler == "ladies", rng)
              for _ in range(args.cpu_batches)]
    print(json.dumps({"tool": "layerwise_bench", "sampler": args.sampler, "graph": args.graph, "nodes": n, "nnz_with_self_loops": L.nnz,
                      "batch": args.batch, "fanouts": fanouts, "hidden": args.hidden, "setup_s": round(setup_s, 3),
                      "sampler_ms_device": round(float(np.median(dev_ms)), 3), "sampler_ms_host": round(float(np.median(host_ms)), 3),
                      "sampler_ms_host_p90": round(float(np.percentile(host_ms, 90)), 3), "e2e_batches_per_s": round(e2e, 1),
                      "cpu_scipy_ms": round(float(np.median(cpu_ms)), 1), "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
