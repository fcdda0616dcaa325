#!/usr/bin/env python3
"""Size-capped Louvain and Leiden (dgll_amd/community.py, csrc/louvain.hip) on the products-shaped graph, next to label propagation:

  * seconds per level-0 sweep (one dgll_hip_louvain_move call with its scratch allocation and info read) and edges/s;
  * the levels: nodes, sweeps, seconds;
  * total seconds and modularity of `louvain` and of `reorder.label_propagation` on the same graph;
  * `leiden` on the same graph: seconds per level-0 refinement sweep (one dgll_hip_leiden_refine call), the levels with their
    refinement sweeps and seconds, total seconds, modularity;
  * the number of disconnected communities of both (`disconnected`: label propagation of component ids inside the communities);
  * the time of bench.py's SpMM shapes (bf16, mean, F = 100 / 256 / 47) on the graph ordered each way.

    python tools/cog_bench.py [--nodes N] [--max-comm-size C]

Prints one JSON line.  DESIGN.md section 6.3 says "Measured: not yet" until a run of this is recorded there.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dgll_amd import community, ops, reorder, synth  # noqa: E402


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) / reps


def sweep_seconds(g, cap, reps=5):
    """Level 0, sweep 0 (every node a singleton, the densest sweep): one move_targets call between two events."""
    n, dev = g.n_rows, g.device
    k, size = g.degrees().contiguous(), torch.ones(n, dtype=torch.int64, device=dev)
    comm = torch.arange(n, dtype=torch.int32, device=dev)
    tot, csize, cnt = community.community_state(k, size, comm, n)
    args = (g.rowptr, g.col, None, k, size, comm, tot, csize, cnt, g.nnz, 1.0, cap, 0, 0, 0, False)
    community.move_targets(*args)
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        community.move_targets(*args)                 # includes its scratch allocation and the blocking info read
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / 1e3)
    return sorted(times)[len(times) // 2]


def refine_sweep_seconds(g, cap, reps=5):
    """Level 0, refinement sweep 0 inside one bound community (every entry counts, every node decides): one refine_targets call."""
    n, dev = g.n_rows, g.device
    k, size = g.degrees().contiguous(), torch.ones(n, dtype=torch.int64, device=dev)
    sub = torch.arange(n, dtype=torch.int32, device=dev)
    bound = torch.zeros(n, dtype=torch.int32, device=dev)
    tot, csize, cnt = community.community_state(k, size, sub, n)
    totP = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, bound.long(), k)
    args = (g.rowptr, g.col, None, k, size, sub, bound, tot, csize, cnt, totP, g.nnz, 1.0, cap)
    community.refine_targets(*args)
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        community.refine_targets(*args)               # includes its allocations and the blocking info read
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / 1e3)
    return sorted(times)[len(times) // 2]


def disconnected(g, labels):
    """Communities that fall into pieces: connected components of the entries inside a community (minimum-id propagation with
    pointer jumping, on the device) minus the number of communities.  The graph must be symmetric."""
    n = g.n_rows
    row, col = g.row_index(), g.col.long()
    keep = labels[row] == labels[col]
    row, col = row[keep], col[keep]
    comp = torch.arange(n, device=g.device)
    while True:
        new = comp.clone().scatter_reduce_(0, row, comp[col], reduce="amin")
        new = new[new]
        if torch.equal(new, comp):
            break
        comp = new
    return int(torch.unique(comp).numel()) - int(torch.unique(labels).numel())


def spmm_ms(g, widths=(100, 256, 47), reps=10):
    out = {}
    for f in widths:
        x = ops.alloc_features(g.n_rows, f, torch.bfloat16, g.device, pad_to=64)
        x.normal_()
        ops.spmm(g, x, reduce="mean")
        _, sec = timed(lambda: ops.spmm(g, x, reduce="mean"), reps)
        out["F%d" % f] = round(sec * 1e3, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=synth.PRODUCTS_NODES)
    ap.add_argument("--avg-degree", type=float, default=50.5)
    ap.add_argument("--max-comm-size", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cog_bench runs the HIP kernels: a GPU is required")
    dev = torch.device("cuda:0")
    g = synth.products_like_graph(dev, seed=0, n=args.nodes, n_undirected=int(args.nodes * args.avg_degree / 2), locality=0.9,
                                  permute_ids=True)
    cap = g.n_rows if args.max_comm_size is None else args.max_comm_size
    rec = {"nodes": g.n_rows, "entries": g.nnz, "max_comm_size": cap, "max_degree": int(g.degrees().max())}
    sec = sweep_seconds(g, cap)
    rec["level0_sweep_s"], rec["level0_edges_per_s"] = round(sec, 6), round(g.nnz / sec)
    levels, clock = [], [time.perf_counter()]

    def on_sweep(level, sweep, comm, size):
        if level == len(levels):
            levels.append({"nodes": int(comm.numel()), "sweeps": 0, "s": 0.0})
        torch.cuda.synchronize()
        now = time.perf_counter()
        levels[level]["sweeps"] += 1
        levels[level]["s"] = round(levels[level]["s"] + now - clock[0], 4)       # includes the aggregation that built the level
        clock[0] = now

    labels, rec["louvain_s"] = timed(lambda: community.louvain(g, max_comm_size=args.max_comm_size, seed=args.seed, on_sweep=on_sweep))
    rec["levels"] = levels
    rec["louvain_communities"], rec["louvain_largest"] = int(labels.max()) + 1, int(torch.bincount(labels).max())
    rec["louvain_modularity"] = round(community.modularity(g, labels), 5)
    rec["louvain_disconnected"] = disconnected(g, labels)
    sec = refine_sweep_seconds(g, cap)
    rec["level0_refine_sweep_s"], rec["level0_refine_edges_per_s"] = round(sec, 6), round(g.nnz / sec)
    rlevels, clock[0] = [], time.perf_counter()

    def on_refine(level, sweep, sub, bound, size):
        while level >= len(rlevels):
            rlevels.append({"nodes": int(sub.numel()), "refine_sweeps": 0, "refine_s": 0.0})
        torch.cuda.synchronize()
        now = time.perf_counter()
        rlevels[level]["refine_sweeps"] += 1
        rlevels[level]["refine_s"] = round(rlevels[level]["refine_s"] + now - clock[0], 4)
        clock[0] = now

    def on_move(level, sweep, comm, size):
        torch.cuda.synchronize()
        clock[0] = time.perf_counter()               # the refinement's clock starts where the local moving ends

    labels, rec["leiden_s"] = timed(lambda: community.leiden(g, max_comm_size=args.max_comm_size, seed=args.seed, on_sweep=on_move,
                                                             on_refine=on_refine))
    rec["leiden_levels"] = rlevels
    rec["leiden_refine_s"] = round(sum(lv["refine_s"] for lv in rlevels), 4)
    rec["leiden_communities"], rec["leiden_largest"] = int(labels.max()) + 1, int(torch.bincount(labels).max())
    rec["leiden_modularity"] = round(community.modularity(g, labels), 5)
    rec["leiden_disconnected"] = disconnected(g, labels)
    lpa, rec["lpa_s"] = timed(lambda: reorder.label_propagation(g.rowptr, g.col, g.n_rows, seed=args.seed))
    dense = torch.unique(lpa, return_inverse=True)[1]
    rec["lpa_communities"], rec["lpa_largest"] = int(dense.max()) + 1, int(torch.bincount(dense).max())
    rec["lpa_modularity"] = round(community.modularity(g, dense), 5)
    rec["spmm_ms"] = {"given_order": spmm_ms(g)}
    for method in ("lpa", "louvain"):
        g2, _ = g.reorder(method=method, seed=args.seed, max_comm_size=args.max_comm_size)
        rec["spmm_ms"][method] = spmm_ms(g2)
        del g2
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
