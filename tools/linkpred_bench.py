#!/usr/bin/env python3
"""Link-prediction benchmark: prints ONE JSON line.

    python tools/linkpred_bench.py --graph reddit   [--batch 1024 --negatives 5 --fanouts 25,10,10 --batches 20]
    python tools/linkpred_bench.py --graph products

On the synthetic graphs of tools/neighbor_bench.py (reddit-shaped: 232 965 nodes, 57.3 M undirected edges; products-shaped:
synth.products_like_graph defaults), batches of uniform random edge ids:
  edge_ms_events / edge_ms_host      EdgePredictionSampler.sample_seeded (filter_existing=True, exclude="reverse"): device time on the
                                     sampler's stream (events) and host wall time (it returns after its stream has finished), medians
  blocks_ms_events / blocks_ms_host  NeighborSampler.sample_seeded alone on the SAME output_nodes and seed: what the edge front end adds
                                     is the difference
  capped_rate                        capped negatives / negatives drawn, over all timed batches
  output_nodes, sources              medians of M and of the outermost source list
  pair_dot_fwd_ms / pair_dot_bwd_ms  ops.pair_dot on the last batch's pairs and a random [M, 256] bf16 matrix: kernel time by events,
                                     median of --reps launches each; *_gbs: bytes the algorithm needs (forward: two rows read per
                                     pair, the pairs, the scores; backward: one row read per incidence entry, the incidence, g, the
                                     gradient written) over that time
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dgll_amd import ops, ops_pair, synth  # noqa: E402
from dgll_amd.sampling import EdgePredictionSampler, NeighborSampler  # noqa: E402

GRAPHS = {"products": dict(n=synth.PRODUCTS_NODES, n_undirected=synth.PRODUCTS_UNDIRECTED_EDGES),
          "reddit": dict(n=232_965, n_undirected=57_300_000)}


def timed(fn, reps, warmup=3):
    """Median device milliseconds of fn() on the current stream."""
    out = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=sorted(GRAPHS), default="reddit")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--negatives", type=int, default=5)
    ap.add_argument("--fanouts", default="25,10,10")
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--feat", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    spec = GRAPHS[args.graph]
    fanouts = [int(f) for f in args.fanouts.split(",")]
    g = synth.products_like_graph(dev, seed=1, n=spec["n"], n_undirected=spec["n_undirected"], locality=0.0)
    nbs = NeighborSampler(fanouts, g)
    eps = EdgePredictionSampler(nbs, negatives=args.negatives, filter_existing=True, exclude="reverse")
    rng = np.random.default_rng(0)
    e_ms, e_host, b_ms, b_host, m_nodes, sources, capped, drawn = [], [], [], [], [], [], 0, 0
    batch = None
    for i in range(args.warmup + args.batches):
        eids = rng.integers(0, g.nnz, args.batch)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        h0 = time.perf_counter()
        e0.record(eps.stream)
        inp, batch, _ = eps.sample_seeded(None, eids, i)
        e1.record(eps.stream)
        h1 = time.perf_counter()
        e1.synchronize()
        n0, n1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        g0 = time.perf_counter()
        n0.record(nbs.stream)
        nbs.sample_seeded(None, batch.output_nodes, i)
        n1.record(nbs.stream)
        g1 = time.perf_counter()
        n1.synchronize()
        if i >= args.warmup:
            e_ms.append(e0.elapsed_time(e1))
            e_host.append((h1 - h0) * 1e3)
            b_ms.append(n0.elapsed_time(n1))
            b_host.append((g1 - g0) * 1e3)
            m_nodes.append(int(batch.output_nodes.numel()))
            sources.append(int(inp.numel()))
            capped += batch.capped
            drawn += batch.n_neg
    # pair scores at F = --feat, bf16, on the last batch
    m, p, f = int(batch.output_nodes.numel()), len(batch), args.feat
    h = ops.as_rows16(torch.randn(m, f, device=dev).to(torch.bfloat16))
    grad = torch.randn(p, device=dev)
    inc = batch.incidence()
    fwd = timed(lambda: ops_pair.pair_dot_raw(h, batch.pairs), args.reps)
    bwd = timed(lambda: ops_pair.pair_dot_bwd_raw(h, inc, p, grad), args.reps)
    row = f * h.element_size()
    fwd_bytes = p * (2 * row + 8 + 4)
    bwd_bytes = 2 * p * (row + 4 + 4 + 4) + (m + 1) * 8 + m * row
    med = lambda v: round(float(np.median(v)), 3)      # noqa: E731
    print(json.dumps({
        "tool": "linkpred_bench", "graph": args.graph, "nodes": g.n_rows, "nnz": g.nnz, "batch": args.batch, "negatives": args.negatives,
        "fanouts": fanouts, "batches": args.batches, "edge_ms_events": med(e_ms), "edge_ms_host": med(e_host),
        "blocks_ms_events": med(b_ms), "blocks_ms_host": med(b_host), "added_ms_events": round(med(e_ms) - med(b_ms), 3),
        "added_ms_host": round(med(e_host) - med(b_host), 3), "capped_rate": round(capped / max(drawn, 1), 6),
        "output_nodes": med(m_nodes), "sources": med(sources), "pairs": p, "feat": f, "dtype": "bf16",
        "pair_dot_fwd_ms": round(fwd, 4), "pair_dot_fwd_gbs": round(fwd_bytes / fwd / 1e6, 1),
        "pair_dot_bwd_ms": round(bwd, 4), "pair_dot_bwd_gbs": round(bwd_bytes / bwd / 1e6, 1),
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
