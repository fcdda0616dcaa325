#!/usr/bin/env python3
"""A/B of the row-group SpMM kernel (dgll_hip_debug_tune(15, v): 1 = never, 2 / 4 = wherever instantiated, with that many slots
per row) on the bench graph, forward and transposed, and on thinned / thickened copies of it (the band's edges); also the idle
share of the kernel's lane groups on the bench graph: the rows of a wavefront advance until its longest row is done."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dgll_amd  # noqa: E402
from dgll_amd import _lib, ops, synth  # noqa: E402

dev = torch.device("cuda:0")
g = synth.products_like_graph(dev, seed=0, locality=0.9, exact=True, permute_ids=True).reorder(seed=0)[0]
gt = g.transpose()[0]


def idle_share(graph, rows, round_edges, threshold=256):
    """Share of the gather positions issued by groups of `rows` consecutive rows (rounds of `round_edges` edges per row, all rows
    of a group running until the longest is done) that carry no edge."""
    n = torch.diff(graph.rowptr)
    n = torch.where(n > threshold, torch.zeros_like(n), n)          # long rows run as chunk items
    pad = (-n.numel()) % rows
    n = torch.cat([n, n.new_zeros(pad)]).view(-1, rows)
    rounds = (n.max(dim=1).values + round_edges - 1) // round_edges
    issued = int(rounds.sum()) * rows * round_edges
    return 1.0 - float(n.sum()) / max(issued, 1)


def timed(graph, x, weighted, reps=6):
    val = torch.rand(graph.nnz, device=dev) if weighted else None
    fn = lambda: ops.spmm_raw(graph, x, val=val, reduce="sum" if weighted else "mean")   # noqa: E731
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def thinned(graph, keep_frac):
    keep = torch.rand(graph.nnz, device=dev) < keep_frac
    return dgll_amd.CSRGraph.from_coo(graph.row_index()[keep], graph.col[keep].long(), None, (graph.n_rows, graph.n_cols), coalesce=False)


def doubled(graph):
    """Every row twice as long: the row's edges followed by the edges of the row half the graph away."""
    n = graph.n_rows
    row = graph.row_index()
    row2 = torch.cat([row, (row + n // 2) % n])
    col2 = torch.cat([graph.col.long(), graph.col.long()])
    return dgll_amd.CSRGraph.from_coo(row2, col2, None, (n, graph.n_cols), coalesce=False)


for name, graph in (("forward", g), ("transposed", gt)):
    for rows, spr in ((4, 2), (2, 4)):
        print("idle share, %s bench graph, LPR = 8, %d rows per wavefront (SPR = %d, rounds of %d edges): %.3f; wave-per-row rounds of 32: %.3f"
              % (name, rows, spr, 4 * spr, idle_share(graph, rows, 4 * spr), idle_share(graph, 1, 32)), flush=True)

cases = [("bench graph (avg %.0f edges/row)" % (g.nnz / g.n_rows), g), ("bench graph transposed", gt)]
if "--band" in sys.argv:
    for frac in (0.5, 0.75):
        t = thinned(g, frac)
        cases.append(("thinned (avg %.0f edges/row)" % (t.nnz / t.n_rows), t))
    d = doubled(g)
    cases.append(("doubled (avg %.0f edges/row)" % (d.nnz / d.n_rows), d))
    t = thinned(d, 0.75)
    cases.append(("doubled, thinned (avg %.0f edges/row)" % (t.nnz / t.n_rows), t))
for name, graph in cases:
    for feat in (47, 64, 100):
        x = ops.alloc_features(graph.n_cols, feat, torch.bfloat16, dev, pad_to=64 if feat < 64 else 8)
        x.copy_(torch.randn(graph.n_cols, feat, device=dev))
        for weighted in (False, True):
            res = {}
            modes = (1, 2, 4) if feat <= 64 else (1, 2)
            for rnd in range(2):
                for mode in modes:
                    _lib.lib.dgll_hip_debug_tune(15, mode)
                    gg = dgll_amd.CSRGraph(graph.rowptr, graph.col, None, graph.n_rows, graph.n_cols, check=False)
                    res.setdefault(mode, []).append(timed(gg, x, weighted))
            old = min(res[1])
            print("%-36s F=%-3d %-10s old choice %.3f ms" % (name, feat, "weighted" if weighted else "unweighted", old) +
                  "".join("   SPR = %d: %.3f ms (%+.0f %%)" % (m, min(res[m]), 100.0 * (min(res[m]) / old - 1)) for m in modes[1:]), flush=True)
_lib.lib.dgll_hip_debug_tune(15, 0)
