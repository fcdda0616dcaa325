#!/usr/bin/env python3
"""Generate tests/golden/layerwise_*.npz by RUNNING the reference's layer-wise samplers.

Runs only where the reference tree exists (the build container); the GPU box only sees the .npz files this script wrote.
The MQ*.py scripts cannot be imported (their top levels load ogb datasets and need DGL), so the sampler classes and the
`utils.py` functions they use are extracted from the files with `ast` at generation time and executed against stubs:
`dgll.create_block` (records what the reference passes it), `dgll.dataloading.Sampler` and a small fake graph (directed,
two hubs, one isolated node).  Each class runs under `np.random.seed` on a fixed batch; for every layer the fixture holds the
rows R the reference sliced, the ids drawn (draw order), the columns of the block, p, the weights, `indptr` / `indices` as
passed to `create_block` and the values `lap_matrix[R][:, cols].multiply(w)` -- which the reference computes and then drops.

Only data is written: no reference source text is stored in the fixtures.

Usage:  python tests/golden/gen_layerwise_goldens.py            (writes next to this file)
"""
import ast
import json
import os
import types

import numpy as np
import scipy.sparse as sp
import torch

REF = os.path.join("/root/reference", "dgll", "GPU Accelerator")
OUT = os.path.dirname(os.path.abspath(__file__))
N, SEED, FANOUTS = 300, 11, [40, 80]
# (fixture name, script, class, constructor keyword arguments)
CASES = [("ladies", "MQLadies.py", "Ladies", {}),
         ("ladies_flat", "MQLadies.py", "Ladies", {"flat": True}),
         ("ladies_wrs", "MQLadiesWrs.py", "LadiesWrs", {}),
         ("ladies_flat_wrs", "MQLadiesFlatWrs.py", "LadiesFlatWrs", {"flat": True}),
         ("fastgcn", "MQFastGCN.py", "FastGCNSampler", {}),
         ("fastgcn_flat", "MQFastGCNFlat.py", "FastGCNSamplerFlat", {"flat": True}),
         ("fastgcn_flat_wrs", "MQFastGCNFlat.py", "FastGCNSamplerFlat", {"flat": True, "wrs": True}),
         ("fastgcn_flat_plain", "MQFastGCNFlat.py", "FastGCNSamplerFlat", {})]


def fake_graph():
    """Directed graph on N nodes: random edges, two hubs (node 3 points to many, many point to node 7), node N-1 isolated."""
    rng = np.random.default_rng(5)
    src = rng.integers(0, N - 1, 1200)
    dst = rng.integers(0, N - 1, 1200)
    hub_out = np.stack([np.full(90, 3), rng.choice(N - 1, 90, replace=False)])
    hub_in = np.stack([rng.choice(N - 1, 120, replace=False), np.full(120, 7)])
    row = np.concatenate([src, hub_out[0], hub_in[0]])
    col = np.concatenate([dst, hub_out[1], hub_in[1]])
    keep = row != col
    A = sp.csr_matrix((np.ones(keep.sum()), (row[keep], col[keep])), shape=(N, N))
    A.data[:] = 1.0                                   # duplicates collapse to one unweighted edge
    A.eliminate_zeros()
    A.sort_indices()
    return A


def extract(path, names):
    """The top-level function / class definitions `names` of one reference file, as an executable module AST."""
    tree = ast.parse(open(path).read(), filename=path)
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert {n.name for n in body} == set(names), (path, names)
    return ast.Module(body=body, type_ignores=[])


class Recorder:
    def __init__(self):
        self.layers = []

    def new(self):
        self.layers.append({})
        return self.layers[-1]


class RecLap:
    """Wraps the sampler's lap_matrix: records the rows it is sliced with."""

    def __init__(self, m, rec):
        self.m, self.rec = m, rec

    def __getitem__(self, key):
        rows = np.asarray(key[0]).astype(np.int64)      # the reference passes torch tensors, which this scipy no longer accepts
        self.rec.new()["rows"] = rows.copy()
        return self.m[rows, key[1]]

    def multiply(self, other):
        return self.m.multiply(other.m if isinstance(other, RecLap) else other)


def run_case(name, script, cls_name, kw, A):
    rec = Recorder()
    ns = {"np": np, "sp": sp, "torch": torch}
    exec(compile(extract(os.path.join(REF, "utils.py"), ["matrix_row_normalize", "estWRS_weights", "normalize_lap"]), "utils", "exec"), ns)
    orig_wrs = ns["estWRS_weights"]

    def est_wrs(p, m):
        idx, w = orig_wrs(p, m)
        rec.layers[-1].update(p=np.asarray(p, dtype=np.float64).copy(), draw=np.asarray(idx, np.int64).copy(), w=np.asarray(w).copy())
        return idx, w

    ns["estWRS_weights"] = est_wrs

    class FakeBlock:
        def __init__(self, indptr, indices):
            self.n_src = int(indices.max()) + 1 if len(indices) else 0      # DGL infers the source count from the indices
            self.srcdata, self.dstdata = {}, {}

        def srcnodes(self):
            return torch.arange(self.n_src)

    def create_block(spec):
        fmt, (indptr, indices, _eids) = spec
        assert fmt == "csc"
        rec.layers[-1].update(indptr=np.asarray(indptr, np.int64).copy(), indices=np.asarray(indices, np.int64).copy())
        return FakeBlock(indptr, indices)

    class Sampler:
        def __init__(self):
            pass

    dgll = types.SimpleNamespace(create_block=create_block, dataloading=types.SimpleNamespace(Sampler=Sampler))
    ns["dgll"] = dgll
    np_shim = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    real_choice = np.random.choice

    def choice(n, s, replace=True, p=None):
        idx = real_choice(n, s, replace=replace, p=p)
        lay = rec.layers[-1]
        if "draw" not in lay:
            lay.update(p=np.asarray(p, np.float64).copy(), draw=np.asarray(idx, np.int64).copy())
        return idx

    np_shim.random = types.SimpleNamespace(choice=choice)
    ns["np"] = np_shim
    exec(compile(extract(os.path.join(REF, script), [cls_name]), script, "exec"), ns)

    class FakeGraph:
        ndata = {"feat": torch.zeros(N, 1), "label": torch.zeros(N, dtype=torch.int64)}

        def adj_external(self, scipy_fmt):
            assert scipy_fmt == "csr"
            return A.copy()

        def num_nodes(self):
            return N

    g = FakeGraph()
    sampler = ns[cls_name](FANOUTS, g, **kw)
    lap = sp.csr_matrix(sampler.lap_matrix)
    lap.sort_indices()
    sampler.lap_matrix = RecLap(sampler.lap_matrix, rec)
    batch = np.array([N - 1, 0, 3, 7, 42, 99, 150, 151, 200, 250, 298, 17, 64], dtype=np.int64)
    np.random.seed(SEED)
    inp, _, subgs = sampler.sample(g, torch.as_tensor(batch))
    out = {"n": np.int64(N), "a_indptr": A.indptr.astype(np.int64), "a_indices": A.indices.astype(np.int64),
           "lap_indptr": lap.indptr.astype(np.int64), "lap_indices": lap.indices.astype(np.int64), "lap_data": lap.data.astype(np.float64),
           "batch": batch, "fanouts": np.array(FANOUTS, np.int64), "input_nodes": np.asarray(inp, np.int64)}
    union = cls_name == "FastGCNSampler"
    for l, lay in enumerate(rec.layers):
        p, draw = lay["p"], lay["draw"]
        s_num = int(min(np.sum(p > 0), FANOUTS[l]))
        if union:
            cols = np.unique(np.concatenate((draw, batch)))
        else:
            cols = draw
        if "w" in lay:
            w = lay["w"]
        else:
            w = 1 / p[cols] / s_num
        R = lay["rows"]
        blk = lap[R][:, cols].multiply(w).tocsr()
        assert np.array_equal(blk.indptr, lay["indptr"]) and np.array_equal(blk.indices, lay["indices"])
        for k, v in (("rows", R), ("draw", draw), ("cols", np.asarray(cols, np.int64)), ("p", p), ("w", np.asarray(w, np.float64)),
                     ("indptr", lay["indptr"]), ("indices", lay["indices"]), ("values", blk.data.astype(np.float64)), ("s", np.int64(s_num))):
            out["l%d_%s" % (l, k)] = v
    meta = {"class": cls_name, "script": script, "kwargs": kw, "seed": SEED, "layers": len(rec.layers), "union": union}
    np.savez_compressed(os.path.join(OUT, "layerwise_%s.npz" % name), meta=json.dumps(meta), **out)
    print(name, {k: v.shape for k, v in out.items() if isinstance(v, np.ndarray) and v.ndim})


def main():
    assert os.path.isdir(REF), "reference not mounted; goldens can only be regenerated in the build container"
    A = fake_graph()
    for case in CASES:
        run_case(*case, A)


if __name__ == "__main__":
    main()
