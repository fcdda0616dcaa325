#!/usr/bin/env python3
"""Subgraph-sampler benchmark: prints ONE JSON line, every time in ms per batch (median over --batches).

    python tools/subgraph_bench.py --graph reddit   [--nodes-per-batch 10000 --batches 20]
    python tools/subgraph_bench.py --graph products

On a synthetic graph (reddit-shaped: 232 965 nodes, 57.3 M undirected edges; products-shaped: synth.products_like_graph defaults):
  node_subgraph_ms_events / _ms_host   node_subgraph(graph, M random nodes, normalize="row") on a persistent workspace: device time
                       (events on the current stream) and host wall time (it returns after its one blocking read and the fill launch;
                       the wall time includes a final synchronize)
  torch_ms_events / _ms_host           the BASELINE: the same result in torch -- sampling.community.induced_range's mask, cumsum and
                       boolean index, generalised to a node list through a lookup table (local id per node, -1 elsewhere) and a
                       flat entry index of the selected rows; checked against the kernel's result once (structure equal, values to 1e-6)
  shadow_ms_host, neighbor_ms_host     ShaDowKHopSampler.sample_seeded next to the NeighborSampler.sample_seeded call it wraps
                       (same seeds, same batches), host wall; shadow_nodes: rows of the batch subgraph
  saint_{node,edge,walk}_ms_host       SAINTSampler.sample_seeded per mode, host wall; saint_*_nodes: rows of the batch subgraph;
                       saint_node_longest_row: entries of the longest parent row among a node-mode batch's rows (one workgroup walks it)
  transpose_ms_host                    the lazy CSRGraph.transpose() (a torch sort) of one node_subgraph batch graph, host wall
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
from dgll_amd.graph import CSRGraph  # noqa: E402
from dgll_amd.sampling import NeighborSampler, SAINTSampler, ShaDowKHopSampler, SubgraphWorkspace, node_subgraph  # noqa: E402
from dgll_amd.sampling.subgraph import LONG_ROW  # noqa: E402

GRAPHS = {"products": dict(n=synth.PRODUCTS_NODES, n_undirected=synth.PRODUCTS_UNDIRECTED_EDGES),
          "reddit": dict(n=232_965, n_undirected=57_300_000)}


def torch_node_subgraph(graph, nodes, table):
    """The torch formulation (normalize="row").  table: int64[N] of -1, restored before returning."""
    m = nodes.numel()
    table[nodes] = torch.arange(m, device=nodes.device)
    b = graph.rowptr[nodes]
    deg = graph.rowptr[nodes + 1] - b
    ends = torch.cumsum(deg, 0)
    total = int(ends[-1]) if m else 0
    e = torch.repeat_interleave(b - (ends - deg), deg) + torch.arange(total, device=nodes.device)      # entry index of every selected entry
    local = table[graph.col[e].long()]
    keep = local >= 0
    kept = torch.zeros(total + 1, dtype=torch.int64, device=nodes.device)
    torch.cumsum(keep, 0, out=kept[1:])
    rowptr = torch.cat([kept[:1], kept[ends]])
    col = local[keep].to(torch.int32)
    out_deg = rowptr[1:] - rowptr[:-1]
    val = torch.repeat_interleave(1.0 / out_deg.clamp(min=1).to(torch.float32), out_deg)
    table[nodes] = -1
    return CSRGraph(rowptr, col, val, m, m, check=False)


def timed(fn, stream):
    """(result, device ms by events on `stream`, host wall ms including a synchronize of it)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(stream)
    out = fn()
    e1.record(stream)
    e1.synchronize()
    t1 = time.perf_counter()
    return out, e0.elapsed_time(e1), (t1 - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=sorted(GRAPHS), default="reddit")
    ap.add_argument("--nodes-per-batch", type=int, default=10_000)
    ap.add_argument("--batch", type=int, default=1024, help="ShaDow: seeds per batch")
    ap.add_argument("--fanouts", default="10,5")
    ap.add_argument("--node-budget", type=int, default=6000)
    ap.add_argument("--edge-budget", type=int, default=4000)
    ap.add_argument("--roots", type=int, default=2000)
    ap.add_argument("--length", type=int, default=4)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    spec = GRAPHS[args.graph]
    fanouts = [int(f) for f in args.fanouts.split(",")]
    g = synth.products_like_graph(dev, seed=1, n=spec["n"], n_undirected=spec["n_undirected"], locality=0.0)
    n = g.n_rows
    cur = torch.cuda.current_stream(dev)
    ws = SubgraphWorkspace(n, dev)
    table = torch.full((n,), -1, dtype=torch.int64, device=dev)
    shadow, nbr = ShaDowKHopSampler(fanouts, g), NeighborSampler(fanouts, g, norm=None)
    saint = {"node": SAINTSampler("node", args.node_budget, g), "edge": SAINTSampler("edge", args.edge_budget, g),
             "walk": SAINTSampler("walk", (args.roots, args.length), g)}
    rng = np.random.default_rng(0)
    deg = g.degrees()
    t = {k: [] for k in ("sg_ev", "sg_host", "torch_ev", "torch_host", "shadow", "nbr", "shadow_nodes", "sg_nnz", "transpose",
                         "node", "edge", "walk", "node_nodes", "edge_nodes", "walk_nodes", "longest")}
    for i in range(args.warmup + args.batches):
        nodes = torch.as_tensor(rng.choice(n, args.nodes_per_batch, replace=False), device=dev)
        sub, ev, host = timed(lambda: node_subgraph(g, nodes, normalize="row", workspace=ws), cur)
        want, tev, thost = timed(lambda: torch_node_subgraph(g, nodes, table), cur)
        if i == 0 and not (torch.equal(sub.rowptr, want.rowptr) and torch.equal(sub.col, want.col) and torch.allclose(sub.val, want.val, rtol=1e-6, atol=0)):
            raise SystemExit("the torch baseline and the kernel disagree")
        _, _, tr = timed(lambda: sub.transpose(), cur)
        seeds = rng.choice(n, args.batch, replace=False)
        (inp, _, _), _, sh = timed(lambda: shadow.sample_seeded(None, seeds, i), cur)
        _, _, nb = timed(lambda: nbr.sample_seeded(None, seeds, i), cur)
        modes = {k: timed(lambda s=s: s.sample_seeded(None, i), cur) for k, s in saint.items()}
        if i >= args.warmup:
            for k, v in (("sg_ev", ev), ("sg_host", host), ("torch_ev", tev), ("torch_host", thost), ("transpose", tr), ("shadow", sh),
                         ("nbr", nb), ("shadow_nodes", inp.numel()), ("sg_nnz", sub.nnz)):
                t[k].append(v)
            for k, ((nd, _), _, ms) in modes.items():
                t[k].append(ms)
                t[k + "_nodes"].append(nd.numel())
            t["longest"].append(int(deg[modes["node"][0][0]].max()))
    med = lambda v: round(float(np.median(v)), 3)      # noqa: E731
    print(json.dumps({"tool": "subgraph_bench", "graph": args.graph, "nodes": n, "nnz": g.nnz, "nodes_per_batch": args.nodes_per_batch,
                      "batches": args.batches, "subgraph_nnz": med(t["sg_nnz"]),
                      "node_subgraph_ms_events": med(t["sg_ev"]), "node_subgraph_ms_host": med(t["sg_host"]),
                      "torch_ms_events": med(t["torch_ev"]), "torch_ms_host": med(t["torch_host"]),
                      "transpose_ms_host": med(t["transpose"]),
                      "shadow_batch": args.batch, "fanouts": fanouts, "shadow_ms_host": med(t["shadow"]), "neighbor_ms_host": med(t["nbr"]),
                      "shadow_nodes": med(t["shadow_nodes"]),
                      "saint_node_budget": args.node_budget, "saint_node_ms_host": med(t["node"]), "saint_node_nodes": med(t["node_nodes"]),
                      "saint_node_longest_row": med(t["longest"]),
                      "saint_edge_budget": args.edge_budget, "saint_edge_ms_host": med(t["edge"]), "saint_edge_nodes": med(t["edge_nodes"]),
                      "saint_walk_budget": [args.roots, args.length], "saint_walk_ms_host": med(t["walk"]),
                      "saint_walk_nodes": med(t["walk_nodes"]), "long_row": LONG_ROW,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
