#!/usr/bin/env python3
"""Generate tests/golden/cog_groups.npz: the reference's CoG group forming, RUN on fixed community lists, and two seeded test graphs
with the modularity networkx's Louvain reaches on them.

Runs only where the reference tree exists (the build container); the GPU box only sees the .npz file this script wrote.  The
reference's `GPU Accelerator/cog.py` cannot be imported (igraph and leidenalg are not installed), so `merge_groups` and
`relabel_groups` are extracted with `ast` at generation time, as gen_struc2vec_goldens.py does, and called.  Only data is written:
no reference source text is stored in the fixture.

Cases (communities as ragged lists, in the order given): empty communities, one community larger than the batch, a remainder
group, a batch of 1, a batch larger than everything.  Recorded per case: the merged groups (ragged), the new id of every node in the
order the groups list them, and the groups' [start, end) ranges (what the reference keeps in `groups_id_map_list`).

Graphs (undirected, no self-loops, no duplicates; written as symmetric CSR):
  A: eight planted communities of 40, 60, 80, 100, 120, 150, 200, 250 nodes, about 12 edges per node, 85 % of the edges inside a
     community, and node 0 a hub with 300 extra edges;
  B: 24 communities of 100 nodes, degree 16, 70 % of the edges inside.
For each, `nx.community.modularity` of `nx.community.louvain_communities(G, seed=s)`, s = 0..4: the yardstick of the Louvain tests
(Leiden cannot be run here; both maximise the same objective).

Usage:  python tests/golden/gen_cog_goldens.py            (writes next to this file)
"""
import ast
import json
import os

import networkx as nx
import numpy as np

REF = os.path.join("/root/reference", "dgll", "GPU Accelerator", "cog.py")
OUT = os.path.dirname(os.path.abspath(__file__))

CASES = [
    ([[3, 1, 4], [], [9, 2], [6], [], [5, 8, 7, 0]], 4),
    ([[0, 1, 2, 3, 4, 5, 6, 7, 8], [9], [10, 11], [12]], 3),              # one community larger than the batch; remainder [12]
    ([[2], [0], [1], [4], [3]], 1),
    ([[5, 4], [3], [], [2, 1, 0]], 100),                                    # everything is the remainder
    ([[7, 3], [1, 0, 5], [2], [6, 4], [8]], 5),
]


def extract(path, names):
    tree = ast.parse(open(path).read(), filename=path)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(f.name for f in fns) == sorted(names), (path, names)
    return ast.Module(body=fns, type_ignores=[])


def planted_graph(sizes, undirected_edges, inside, seed, hub_edges=0):
    rng = np.random.RandomState(seed)
    n = int(sum(sizes))
    start = np.concatenate(([0], np.cumsum(sizes)))
    comm = np.repeat(np.arange(len(sizes)), sizes)
    edges = set()
    p = np.asarray(sizes, dtype=np.float64) / n
    while len(edges) < undirected_edges:
        if rng.rand() < inside:
            c = rng.choice(len(sizes), p=p)
            a, b = rng.randint(start[c], start[c + 1], size=2)
        else:
            a, b = rng.randint(0, n, size=2)
            if comm[a] == comm[b]:
                continue
        if a != b:
            edges.add((min(a, b), max(a, b)))
    extra = 0
    while extra < hub_edges:
        b = int(rng.randint(1, n))
        if (0, b) not in edges:
            edges.add((0, b))
            extra += 1
    e = np.array(sorted(edges), dtype=np.int64)
    both = np.concatenate([e, e[:, ::-1]])
    both = both[np.lexsort((both[:, 1], both[:, 0]))]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(both[:, 0], minlength=n), out=rowptr[1:])
    return rowptr, both[:, 1].astype(np.int32), comm.astype(np.int32), e


def ragged(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    return ptr, np.array([v for x in lists for v in x], dtype=np.int64)


def main():
    assert os.path.isfile(REF), "reference not mounted; goldens can only be regenerated in the build container"
    ns = {}
    exec(compile(extract(REF, ["merge_groups", "relabel_groups"]), "cog.py", "exec"), ns)
    out = {}
    for i, (comms, batch) in enumerate(CASES):
        merged = ns["merge_groups"]([list(c) for c in comms], batch)
        relabelled, mapping = ns["relabel_groups"](merged, None, None, None)
        out["comm_ptr_%d" % i], out["comm_nodes_%d" % i] = ragged(comms)
        out["group_ptr_%d" % i], out["group_nodes_%d" % i] = ragged(merged)
        nodes = out["group_nodes_%d" % i]
        out["new_id_%d" % i] = np.array([mapping[int(v)] for v in nodes], dtype=np.int64)
        out["ranges_%d" % i] = np.array([[g[0], g[-1] + 1] for g in relabelled], dtype=np.int64).reshape(-1, 2)
    graphs = {"A": planted_graph([40, 60, 80, 100, 120, 150, 200, 250], 6000, 0.85, 11, hub_edges=300),
              "B": planted_graph([100] * 24, 2400 * 8, 0.70, 12)}
    for name, (rowptr, col, planted, e) in graphs.items():
        g = nx.Graph()
        g.add_nodes_from(range(len(rowptr) - 1))
        g.add_edges_from(e.tolist())
        q = [nx.community.modularity(g, nx.community.louvain_communities(g, seed=s)) for s in range(5)]
        out["rowptr_" + name], out["col_" + name], out["planted_" + name] = rowptr, col, planted
        out["nx_modularity_" + name] = np.array(q, dtype=np.float64)
        print(name, "n", len(rowptr) - 1, "entries", len(col), "max degree", int(np.diff(rowptr).max()), "networkx Q", q)
    meta = {"batch": [b for _, b in CASES], "graphs": sorted(graphs), "nx_seeds": list(range(5)), "networkx": nx.__version__}
    path = os.path.join(OUT, "cog_groups.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **out)
    assert os.path.getsize(path) < 512 * 1024
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
