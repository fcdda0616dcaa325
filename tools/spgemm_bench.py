#!/usr/bin/env python3
"""Device-event timing and peak memory of the sparse x sparse products (csrc/spgemm.hip through dgll_amd.ops_spgemm) on an
ogbn-products-shaped synthetic graph (synth.products_like_graph, scaled down by --nodes / --edges: A . A of the full graph has
more than 2^31 entries):

    A . A        the two-hop graph, with values
    S^T A S      coarsening by --clusters contiguous clusters (two products)

next to torch.sparse.mm on the same operands plus the sort of its COO result back into a CSRGraph, on the same card.

    python tools/spgemm_bench.py [--nodes 131072 --edges 1048576 --clusters 4096 --reps 10 --rounds 3]

HIP events round `reps` calls after two warm-up calls, the implementations alternating inside every round, the median of `rounds`
reported; the symbolic / numeric / backward entry points alone from a LaunchTimer inside the whole call.  Prints a table and one
JSON line.  Run by no test.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dgll_amd import CSRGraph, _lib, ops_spgemm, synth  # noqa: E402


def timeit(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def to_torch(g):
    val = g.val if g.val is not None else torch.ones(g.nnz, device=g.device)
    return torch.sparse_coo_tensor(torch.stack([g.row_index(), g.col.long()]), val, g.shape).coalesce()


def torch_product(ts):
    """torch.sparse.mm down the chain `ts`, then the sort back into CSR that a CSRGraph needs"""
    out = ts[0]
    for t in ts[1:]:
        out = torch.sparse.mm(out, t)
    out = out.coalesce()
    return CSRGraph.from_coo(out.indices()[0], out.indices()[1], out.values(), out.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 17)
    ap.add_argument("--edges", type=int, default=1 << 20, help="undirected edges drawn")
    ap.add_argument("--clusters", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = synth.products_like_graph(dev, seed=0, n=args.nodes, n_undirected=args.edges, weighted=True, locality=0.9)
    if g.val is None:
        g = g.with_values(torch.rand(g.nnz, device=dev))
    cluster = (torch.arange(args.nodes, device=dev) * args.clusters) // args.nodes
    s = CSRGraph(torch.arange(args.nodes + 1, device=dev), cluster.to(torch.int32), None, args.nodes, args.clusters, check=False)
    tg, ts = to_torch(g), to_torch(s)
    tst = ts.t().coalesce()
    cases = {"A.A hip ms": lambda: ops_spgemm.spgemm(g, g, check=False),
             "A.A torch.sparse.mm + sort ms": lambda: torch_product([tg, tg]),
             "StAS hip ms": lambda: ops_spgemm.coarsen(g, cluster, args.clusters),
             "StAS torch.sparse.mm + sort ms": lambda: torch_product([tst, tg, ts])}
    rounds = {key: [] for key in cases}
    for _ in range(args.rounds):                               # alternating: the same round sees the same neighbours on the card
        for key, fn in cases.items():
            rounds[key].append(timeit(fn, args.reps))
    row = {key: statistics.median(v) for key, v in rounds.items()}
    for key, fn in cases.items():
        row[key.replace(" ms", " peak MiB")] = peak_mib(fn)
    for label, fn in (("A.A", cases["A.A hip ms"]), ("StAS", cases["StAS hip ms"])):
        with _lib.LaunchTimer() as timer:                       # events round the entry points alone, inside the whole call
            for _ in range(args.reps):
                fn()
        for tag, (count, avg) in timer.summary().items():
            row["  %s of which %s ms (x%d per call)" % (label, tag[0], count // args.reps)] = avg
    weights = g.val.clone().requires_grad_(True)
    gw = g.with_values(weights)

    def backward():
        ops_spgemm.spgemm(gw, gw, check=False).val.sum().backward()
        weights.grad = None

    row["A.A hip forward + backward ms"] = timeit(backward, args.reps)
    c, ref = cases["A.A hip ms"](), cases["A.A torch.sparse.mm + sort ms"]()
    same = torch.equal(c.rowptr, ref.rowptr) and torch.equal(c.col, ref.col)
    print("n = %d, nnz(A) = %d, nnz(A.A) = %d, same structure as torch: %s, max |value difference| %.3g" % (
        args.nodes, g.nnz, c.nnz, same, float((c.val - ref.val).abs().max()) if same and c.nnz else float("nan")), flush=True)
    for key, v in row.items():
        print("  %-60s %10.4f" % (key, v), flush=True)
    print(json.dumps({key.strip(): round(v, 4) for key, v in row.items()}))


if __name__ == "__main__":
    main()
