#!/usr/bin/env python3
"""Generate tests/golden/node2vec_probs.npz by RUNNING the reference's `Node2vec.computeProbabilities`.

Runs only where the reference tree exists (the build container); the GPU box only sees the .npz file this script wrote.
The package cannot be imported (`utils.py` needs fastdtw), so the method is extracted from `node2vec.py` with `ast` at generation
time and called with a stub `self` (graph, p, q) on a small directed networkx graph: a core of 40 nodes with random edges (so
triangles exist and every one of the three weight classes occurs), node 3 a hub pointing to 100 nodes, leaves that point back
into the core, node 7 with in-edges only and node N - 1 isolated.

The fixture holds the graph as a CSR with ascending rows, and for every edge (t, v) in CSR order the transition probabilities
from v given the previous node t, one per out-neighbour of v in ascending order, for (p, q) = (0.5, 2) and (4, 0.25); and the
number of walks to start at every node (proportional to its out-degree, 200 000 in all, so every (t, v) is visited about
equally often).  Only data is written: no reference source text is stored in the fixture.

Usage:  python tests/golden/gen_embedding_goldens.py            (writes next to this file)
"""
import ast
import json
import os
from collections import defaultdict
from types import SimpleNamespace

import networkx as nx
import numpy as np

REF = os.path.join("/root/reference", "dgll", "Graph Embedding", "src", "ge")
OUT = os.path.dirname(os.path.abspath(__file__))
N, CORE, HUB, SINK, SEED, N_WALKS = 128, 40, 3, 7, 11, 200_000
PQ = [(0.5, 2.0), (4.0, 0.25)]


def fake_graph():
    rng = np.random.default_rng(5)
    edges = set()
    while len(edges) < 120:                                        # the core: dense enough for common neighbours
        a, b = rng.integers(0, CORE, 2)
        if a != b and a != SINK:
            edges.add((int(a), int(b)))
    for b in rng.choice(np.setdiff1d(np.arange(N - 1), [HUB]), 100, replace=False):
        edges.add((HUB, int(b)))                                   # the hub
    for a in rng.choice(np.arange(CORE, N - 1), 40, replace=False):
        edges.add((int(a), int(rng.integers(0, CORE))))            # leaves point back into the core
    edges.add((5, SINK)); edges.add((11, SINK)); edges.add((20, HUB)); edges.add((21, HUB))
    edges = sorted(e for e in edges if e[0] != SINK)               # sorted: networkx then lists neighbours in ascending order
    g = nx.DiGraph()
    g.add_nodes_from(range(N))
    g.add_edges_from(edges)
    return g, np.array(edges, dtype=np.int64)


def extract_method(path, cls, name):
    tree = ast.parse(open(path).read(), filename=path)
    klass = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls]
    fn = [n for n in klass[0].body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(fn) == 1, (path, cls, name)
    return ast.Module(body=fn, type_ignores=[])


def main():
    assert os.path.isdir(REF), "reference not mounted; goldens can only be regenerated in the build container"
    g, edges = fake_graph()
    ns = {"np": np, "defaultdict": defaultdict}
    exec(compile(extract_method(os.path.join(REF, "node2vec.py"), "Node2vec", "computeProbabilities"), "node2vec.py", "exec"), ns)
    compute = ns["computeProbabilities"]
    deg = np.bincount(edges[:, 0], minlength=N)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = edges[:, 1].astype(np.int32)
    assert deg[HUB] >= 100 and deg[SINK] == 0 and deg[N - 1] == 0 and (col == SINK).any() and not (col == N - 1).any()
    prob_ptr = np.zeros(len(edges) + 1, dtype=np.int64)
    np.cumsum(deg[col], out=prob_ptr[1:])
    out = {"rowptr": rowptr, "col": col, "prob_ptr": prob_ptr}
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
        out["probs_%d" % i] = flat
    reps = np.floor(deg / deg.sum() * N_WALKS).astype(np.int64)
    reps[HUB] += N_WALKS - reps.sum()
    out["start_reps"] = reps
    meta = {"pq": PQ, "seed": SEED, "n_walks": N_WALKS, "hub": HUB, "sink": SINK, "isolated": N - 1}
    np.savez_compressed(os.path.join(OUT, "node2vec_probs.npz"), meta=json.dumps(meta), **out)
    print({k: v.shape for k, v in out.items()}, "edges", len(edges), os.path.getsize(os.path.join(OUT, "node2vec_probs.npz")), "bytes")


if __name__ == "__main__":
    main()
