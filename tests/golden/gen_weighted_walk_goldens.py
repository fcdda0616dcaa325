#!/usr/bin/env python3
"""Generate tests/golden/node2vec_probs_weighted.npz by RUNNING the reference's `Node2vec.computeProbabilities` on a weighted graph.

Same method as gen_embedding_goldens.py (whose graph, extraction and layout are imported, not copied): the method is taken out of
`node2vec.py` with `ast` and called with a stub `self` on the 128-node directed graph of node2vec_probs.npz -- same hub, sink and
isolated node -- with a `weight` on every edge.  Runs only where the reference tree exists.

Weights (seeded, every one a float32 value): 2^u with u uniform in [-1, 1], so a row spans a ratio of at most 4; the hub row is
drawn from [1, 2) instead and one of its edges, into a node that has out-edges itself, is 1 500: about 10^3 times the rest; four
edges of core rows with at least three entries are exactly 0, at most one per row, so no row is all zeros.

Starts: the first step is weighted, so edge (t, v) is walked by about start_reps[t] w_tv / sum_x w_tx walks.  start_reps[t] is
the smallest count that gives every positive edge of row t an expectation of EXPECT walks; with the 500 that
`transition_check` asks of a cell, a cell is short only by (EXPECT - 500) / sqrt(EXPECT) = 5.9 standard deviations.  The cells
behind the four zero-weight edges are never reached: they are the share of cells that the rule's 90 % allows to fail.
Only data is written: no reference source text is stored in the fixture.

Usage:  python tests/golden/gen_weighted_walk_goldens.py            (writes next to this file)
"""
import json
import os
import sys
from collections import defaultdict
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_embedding_goldens import CORE, HUB, N, OUT, PQ, REF, SEED, SINK, extract_method, fake_graph  # noqa: E402

WEIGHT_SEED, EXPECT, N_ZERO, DOMINANT = 23, 650, 4, 1500.0


def weights(edges, deg):
    rng = np.random.default_rng(WEIGHT_SEED)
    w = np.exp2(rng.uniform(-1.0, 1.0, len(edges))).astype(np.float32)
    hub = np.nonzero(edges[:, 0] == HUB)[0]
    w[hub] = rng.uniform(1.0, 2.0, len(hub)).astype(np.float32)
    live = hub[deg[edges[hub, 1]] > 0]                             # the dominant edge leads somewhere: its walks go on
    w[live[len(live) // 2]] = DOMINANT
    rows = rng.permutation([t for t in range(CORE) if t != HUB and deg[t] >= 3])[:N_ZERO]
    for t in rows:
        w[rng.choice(np.nonzero(edges[:, 0] == t)[0])] = 0.0
    return w


def main():
    assert os.path.isdir(REF), "reference not mounted; goldens can only be regenerated in the build container"
    g, edges = fake_graph()
    deg = np.bincount(edges[:, 0], minlength=N)
    val = weights(edges, deg)
    for (a, b), w in zip(edges.tolist(), val.tolist()):
        g[a][b]["weight"] = w                                      # a Python float that holds the float32 value exactly
    ns = {"np": np, "defaultdict": defaultdict}
    exec(compile(extract_method(os.path.join(REF, "node2vec.py"), "Node2vec", "computeProbabilities"), "node2vec.py", "exec"), ns)
    compute = ns["computeProbabilities"]
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = edges[:, 1].astype(np.int32)
    assert deg[HUB] >= 100 and deg[SINK] == 0 and deg[N - 1] == 0 and (col == SINK).any() and not (col == N - 1).any()
    row_sum = np.bincount(edges[:, 0], weights=val.astype(np.float64), minlength=N)
    assert (row_sum[deg > 0] > 0).all() and (val == 0).sum() == N_ZERO
    prob_ptr = np.zeros(len(edges) + 1, dtype=np.int64)
    np.cumsum(deg[col], out=prob_ptr[1:])
    out = {"rowptr": rowptr, "col": col, "val": val, "prob_ptr": prob_ptr}
    for i, (p, q) in enumerate(PQ):
        stub = SimpleNamespace(graph=g, p=p, q=q)
        flat = np.zeros(prob_ptr[-1], dtype=np.float64)
        for t in range(N):
            if deg[t] == 0:
                continue
            probs = compute(stub, t)[t]["probabilities"]
            for e in range(rowptr[t], rowptr[t + 1]):
                v = int(col[e])
                assert list(g.neighbors(v)) == sorted(g.neighbors(v))
                flat[prob_ptr[e]:prob_ptr[e + 1]] = np.asarray(probs[v], dtype=np.float64)
        assert np.isfinite(flat).all()
        out["probs_%d" % i] = flat
    reps = np.zeros(N, dtype=np.int64)
    for t in np.nonzero(deg)[0]:
        w = val[rowptr[t]:rowptr[t + 1]].astype(np.float64)
        reps[t] = int(np.ceil(EXPECT * w.sum() / w[w > 0].min()))
    out["start_reps"] = reps
    hub_w = val[rowptr[HUB]:rowptr[HUB + 1]]
    meta = {"pq": PQ, "seed": SEED, "n_walks": int(reps.sum()), "hub": HUB, "sink": SINK, "isolated": N - 1,
            "dominant_ratio": float(hub_w.max() / np.median(hub_w)), "zero_weights": N_ZERO}
    path = os.path.join(OUT, "node2vec_probs_weighted.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **out)
    print({k: v.shape for k, v in out.items()}, meta, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
