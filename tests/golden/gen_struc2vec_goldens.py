#!/usr/bin/env python3
"""Generate tests/golden/struc2vec_context.npz by RUNNING the reference's struc2vec functions.

Runs only where the reference tree exists (the build container); the GPU box only sees the .npz file this script wrote.  The
package cannot be imported (`utils.py` needs fastdtw, `struc2vec.py` gensim), so the functions are extracted with `ast` at
generation time, as gen_embedding_goldens.py does, and called with a stub `self`: from struc2vec.py `_get_order_degreelist_node`,
`_create_vectors`, `_get_layer_rep`, `_get_transition_probs` and `prepare_biased_walk`; from utils.py `get_vertices`,
`verifyDegrees`, `compute_dtw_dist`, `cost`, `cost_max`, `convert_dtw_struc_dist` and `create_alias_table`.  Two things are
injected: an exact dynamic-time-warping function under the name `fastdtw` (same signature, returns (dist, None)) -- fastdtw is not
installed, and the package computes the exact DTW (documented difference (h)) -- and an in-memory dict behind `pd.to_pickle` /
`pd.read_pickle` / `os.path.exists`.  Only data is written: no reference source text is stored in the fixture.

The graph: 57 nodes, undirected.  Two disjoint isomorphic copies of a 24-node motif -- a hub joined to every member of a 6-clique,
a 5-clique and a 4-clique, to 4 leaves and to a pendant path of 4 nodes (hub degree 20) -- as nodes 0..23 and 24..47 (node v mirrors
v + 24), and a third component of another shape: a 7-cycle with one chord and a tail of 2 nodes.  (No degree class is as large
as the 2 log2 N partners a node takes, and no layer is so small or so regular that a row of equal weights sits exactly on the
layer's average weight: the generator asserts the latter.)

Recorded for (opt1_reduce_len, opt2_reduce_sim_calc, opt3_num_layers) in {(T, T, 3), (F, T, 3), (T, F, None)}: the degree lists
(ragged), the pair list in the reference's order, the cumulative distance of every (pair, layer) (-1 where the layer is invalid),
per (layer, v) the neighbour list with the normalised weights, gamma and the layer averages.

Usage:  python tests/golden/gen_struc2vec_goldens.py            (writes next to this file)
"""
import ast
import json
import math
import os
from collections import deque
from types import SimpleNamespace

import networkx as nx
import numpy as np

REF = os.path.join("/root/reference", "dgll", "Graph Embedding", "src", "ge")
OUT = os.path.dirname(os.path.abspath(__file__))
SETTINGS = [(True, True, 3), (False, True, 3), (True, False, None)]
MOTIF, N = 24, 57


def motif_edges(o):
    hub, a, b, c = o, list(range(o + 1, o + 7)), list(range(o + 7, o + 12)), list(range(o + 12, o + 16))
    leaves, path = list(range(o + 16, o + 20)), list(range(o + 20, o + 24))
    e = [(hub, x) for x in a + b + c + leaves + path[:1]]
    e += [(x, y) for k in (a, b, c) for i, x in enumerate(k) for y in k[i + 1:]]
    e += list(zip(path[:-1], path[1:]))
    return e


def fake_graph():
    edges = motif_edges(0) + motif_edges(MOTIF)
    ring = list(range(2 * MOTIF, N))
    edges += [(ring[i], ring[(i + 1) % 7]) for i in range(7)] + [(ring[0], ring[3]), (ring[5], ring[7]), (ring[7], ring[8])]
    g = nx.Graph()
    g.add_nodes_from(range(N))
    g.add_edges_from(sorted((min(a, b), max(a, b)) for a, b in edges))
    return g


def extract(path, names, cls=None):
    tree = ast.parse(open(path).read(), filename=path)
    body = tree.body if cls is None else [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls][0].body
    fns = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(f.name for f in fns) == sorted(names), (path, names)
    return ast.Module(body=fns, type_ignores=[])


def exact_dtw(x, y, radius=1, dist=None):
    m, n = len(x), len(y)
    D = [[math.inf] * (n + 1) for _ in range(m + 1)]
    D[0][0] = 0.0
    for i in range(m):
        for j in range(n):
            D[i + 1][j + 1] = dist(x[i], y[j]) + min(D[i][j + 1], D[i + 1][j], D[i][j])
    return D[m][n], None


def run_setting(g, ns, opt1, opt2, opt3):
    store = {}
    ns["pd"] = SimpleNamespace(to_pickle=lambda obj, path: store.__setitem__(path, obj), read_pickle=lambda path: store[path])
    ns["os"] = SimpleNamespace(path=SimpleNamespace(exists=lambda path: path in store))
    identity = SimpleNamespace(transform=lambda x: np.asarray(x), inverse_transform=lambda x: np.asarray(x))
    stub = SimpleNamespace(graph=g, nodeEncoder=identity, idx=list(range(N)), opt1_reduce_len=opt1, temp_path="mem/")
    lists = {v: ns["_get_order_degreelist_node"](stub, v, opt3) for v in stub.idx}
    if opt2:
        degrees = ns["_create_vectors"](stub)
        vertices = {v: ns["get_vertices"](v, len(g[v]), degrees, N) for v in stub.idx}
    else:
        vertices = {v: [u for u in lists if u > v] for v in lists}
    dtw = ns["compute_dtw_dist"](list(vertices.items()), lists, ns["cost_max"] if opt1 else ns["cost"])
    pairs = list(dtw.keys())
    assert pairs == [(v, u) for v in stub.idx for u in vertices[v]]
    dist = ns["convert_dtw_struc_dist"](dtw)
    adj, layer_dist = ns["_get_layer_rep"](stub, dist)
    ns["_get_transition_probs"](stub, adj, layer_dist)
    ns["prepare_biased_walk"](stub)
    gamma, average = store["mem/gamma.pkl"], store["mem/average_weight"]
    n_layers = max(len(x) for x in lists.values())
    assert sorted(adj) == list(range(n_layers)) and sorted(gamma) == list(range(n_layers))
    # ragged degree lists
    ptr, deg, cnt = [0], [], []
    for v in range(N):
        for l in range(n_layers):
            for item in lists[v].get(l, []):
                d, c = item if opt1 else (item, 1)
                deg.append(d)
                cnt.append(c)
            ptr.append(len(deg))
    d_out = np.full((len(pairs), n_layers), -1.0)
    for p, key in enumerate(pairs):
        for l, x in dist[key].items():
            d_out[p, l] = x
    nb_ptr, nb_col, nb_w = [0], [], []
    g_out = np.zeros(n_layers * N, dtype=np.int64)
    for l in range(n_layers):
        weights = store["mem/norm_weights_distance-layer-%d.pkl" % l]
        for v in range(N):
            if v in adj[l]:
                assert len(adj[l][v]) == len(weights[v]) and np.isfinite(weights[v]).all()
                nb_col += adj[l][v]
                nb_w += weights[v]
                g_out[l * N + v] = gamma[l][v]
            nb_ptr.append(len(nb_col))
    avg = np.array([average[l] for l in range(n_layers)], dtype=np.float64)
    nb_w = np.array(nb_w, dtype=np.float64)
    layer_of = np.repeat(np.arange(n_layers * N) // N, np.diff(nb_ptr))
    gap = np.abs(nb_w - avg[layer_of]) / avg[layer_of]
    assert gap.min() > 1e-9, "a normalised weight sits on its layer's average: gamma would depend on rounding"
    assert sum(1 for l in range(n_layers) if adj[l]) >= 3
    return dict(lists_ptr=np.array(ptr, np.int64), lists_deg=np.array(deg, np.int32), lists_cnt=np.array(cnt, np.int32),
                pairs=np.array(pairs, np.int32).reshape(-1, 2), dist=d_out, nb_ptr=np.array(nb_ptr, np.int64),
                nb_col=np.array(nb_col, np.int32), nb_w=nb_w, gamma=g_out, average=avg), n_layers


def main():
    assert os.path.isdir(REF), "reference not mounted; goldens can only be regenerated in the build container"
    g = fake_graph()
    ns = {"np": np, "math": math, "deque": deque, "fastdtw": exact_dtw}
    exec(compile(extract(os.path.join(REF, "utils.py"), ["get_vertices", "verifyDegrees", "compute_dtw_dist", "cost", "cost_max",
                                                          "convert_dtw_struc_dist", "create_alias_table"]), "utils.py", "exec"), ns)
    exec(compile(extract(os.path.join(REF, "struc2vec.py"), ["_get_order_degreelist_node", "_create_vectors", "_get_layer_rep",
                                                              "_get_transition_probs", "prepare_biased_walk"], "Struc2Vec"),
                 "struc2vec.py", "exec"), ns)
    rows = np.array([(v, u) for v in range(N) for u in sorted(g[v])], dtype=np.int64)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[:, 0], minlength=N), out=rowptr[1:])
    out = {"rowptr": rowptr, "col": rows[:, 1].astype(np.int32)}
    deg = np.diff(rowptr)
    assert deg.min() == 1 and deg.max() >= 20 and nx.number_connected_components(g) == 3
    layers = []
    for i, (opt1, opt2, opt3) in enumerate(SETTINGS):
        res, n_layers = run_setting(g, ns, opt1, opt2, opt3)
        layers.append(n_layers)
        for k, v in res.items():
            out["%s_%d" % (k, i)] = v
    seen = set(map(tuple, out["pairs_0"].tolist()))
    assert any((b, a) in seen for a, b in seen), "no pair in both orders"
    meta = {"settings": SETTINGS, "n_nodes": N, "motif": MOTIF, "n_layers": layers}
    path = os.path.join(OUT, "struc2vec_context.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **out)
    assert os.path.getsize(path) < 512 * 1024
    print({k: v.shape for k, v in out.items()}, "layers", layers, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
