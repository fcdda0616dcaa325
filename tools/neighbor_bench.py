#!/usr/bin/env python3
"""Neighbour-sampler benchmark: prints ONE JSON line.

    python tools/neighbor_bench.py --graph reddit   [--batch 1024 --fanouts 25,10,10 --batches 20]
    python tools/neighbor_bench.py --graph products
    python tools/neighbor_bench.py --graph reddit --prob      # also times NeighborSampler(prob=...) on the same batches

On a synthetic graph (reddit-shaped: the graph of `bench.py --workload minibatch`, 232 965 nodes, 57.3 M undirected edges;
products-shaped: synth.products_like_graph defaults), the same batches through both samplers, same process:
  device_ms_events   NeighborSampler.sample_seeded, device time on the sampler's stream (events), median over --batches
  device_ms_host     its host wall time (it returns after its stream has finished), median
  host_ms            FastNeighborSampler.sample_seeded (host threads, duplicates kept, arrays left on the host), wall, median
  weighted_ms_events, weighted_ms_host (--prob)   the same two figures for the edge-weighted sampler (prob = uniform random weights in
                     (0, 1], none of them 0, so it samples on the same graph), same batches and seeds, next to the uniform one
  *_sources          rows of the outermost source list (what the feature fetch and the first layer's product are proportional to):
                     the device sampler's are distinct; the host sampler's are counted with and without duplicates
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dgll_amd import synth  # noqa: E402
from dgll_amd.data import DGraph  # noqa: E402
from dgll_amd.sampling import FastNeighborSampler, NeighborSampler  # noqa: E402

GRAPHS = {"products": dict(n=synth.PRODUCTS_NODES, n_undirected=synth.PRODUCTS_UNDIRECTED_EDGES),
          "reddit": dict(n=232_965, n_undirected=57_300_000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=sorted(GRAPHS), default="reddit")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--fanouts", default="25,10,10")
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=1)
    ap.add_argument("--prob", action="store_true", help="also time the edge-weighted sampler (prob=) on the same batches")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    spec = GRAPHS[args.graph]
    fanouts = [int(f) for f in args.fanouts.split(",")]
    g = synth.products_like_graph(dev, seed=1, n=spec["n"], n_undirected=spec["n_undirected"], locality=0.0)
    n = g.n_rows
    dg = DGraph.from_csr(g.rowptr.cpu().numpy(), g.col.cpu().numpy().astype(np.int64))
    dsm = NeighborSampler(fanouts, g)
    wsm = None
    if args.prob:
        weights = 1.0 - torch.rand(g.nnz, device=dev, generator=torch.Generator(dev).manual_seed(2))      # (0, 1]
        wsm = NeighborSampler(fanouts, g, prob=weights)
    hsm = FastNeighborSampler(fanouts)
    hsm.prepare(dg)
    rng = np.random.default_rng(0)
    dev_ms, dev_host_ms, host_ms, dev_src, host_src, host_src_distinct = [], [], [], [], [], []
    w_ms, w_host_ms, w_src = [], [], []
    for i in range(args.warmup + args.batches):
        batch = rng.choice(n, args.batch, replace=False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        h0 = time.perf_counter()
        e0.record(dsm.stream)
        inp, _, blocks = dsm.sample_seeded(None, batch, i)
        e1.record(dsm.stream)
        h1 = time.perf_counter()
        e1.synchronize()
        if wsm is not None:
            w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            g0 = time.perf_counter()
            w0.record(wsm.stream)
            winp, _, _ = wsm.sample_seeded(None, batch, i)
            w1.record(wsm.stream)
            g1 = time.perf_counter()
            w1.synchronize()
            if i >= args.warmup:
                w_ms.append(w0.elapsed_time(w1))
                w_host_ms.append((g1 - g0) * 1e3)
                w_src.append(int(winp.numel()))
        t0 = time.perf_counter()
        hinp, _, hsub = hsm.sample_seeded(dg, batch, i, max_threads=args.host_threads)
        t1 = time.perf_counter()
        if i >= args.warmup:
            dev_ms.append(e0.elapsed_time(e1))
            dev_host_ms.append((h1 - h0) * 1e3)
            host_ms.append((t1 - t0) * 1e3)
            dev_src.append(int(inp.numel()))
            outer = np.asarray(hsub[0].src_nodes())
            host_src.append(int(outer.size))
            host_src_distinct.append(int(np.unique(outer).size))
    med = lambda v: round(float(np.median(v)), 3)      # noqa: E731
    out = {"tool": "neighbor_bench", "graph": args.graph, "nodes": n, "nnz": g.nnz, "batch": args.batch, "fanouts": fanouts,
           "batches": args.batches, "device_ms_events": med(dev_ms), "device_ms_host": med(dev_host_ms),
           "device_ms_host_p90": round(float(np.percentile(dev_host_ms, 90)), 3), "host_ms": med(host_ms),
           "host_threads": args.host_threads, "device_sources": med(dev_src), "host_sources": med(host_src),
           "host_sources_distinct": med(host_src_distinct), "device": torch.cuda.get_device_name(0)}
    if wsm is not None:
        out.update({"weighted_ms_events": med(w_ms), "weighted_ms_host": med(w_host_ms), "weighted_sources": med(w_src)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
