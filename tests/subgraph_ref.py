"""Numpy restatement of the subgraph samplers (dgll_amd/csrc/subgraph.hip, dgll_amd/sampling/subgraph.py) -- a helper, not a test.
DGL's contract restated: every decision is an integer compare, and the one value (1 / kept entries of a row) is formed as the
device forms it (a float64 quotient rounded to fp32), so device output is compared bit for bit, `val` included."""
import numpy as np

import embedding_ref
import neighbor_ref
import neighbor_weighted_ref

MODES = {"node": 1, "edge": 2, "walk": 3}


def node_subgraph(rowptr, col, val, nodes, normalize=None):
    """(rowptr int64[M + 1], col int32, val fp32 or None, eid int64): row i = row nodes[i] of the parent, the entries whose column is
    in `nodes` in the parent's order, columns as positions in `nodes`.  normalize None: the parent's values (None without);
    "row": 1 / kept entries of the row."""
    assert normalize in ("row", None)
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col)
    nodes = np.asarray(nodes, np.int64).reshape(-1)
    n = len(rowptr) - 1
    assert len(set(nodes.tolist())) == len(nodes) and (len(nodes) == 0 or (nodes.min() >= 0 and nodes.max() < n))
    local = np.full(n, -1, np.int64)
    local[nodes] = np.arange(len(nodes))
    out_rowptr, out_col, out_val, out_eid = [0], [], [], []
    for v in nodes:
        kept = [e for e in range(int(rowptr[v]), int(rowptr[v + 1])) if local[col[e]] >= 0]
        out_eid += kept
        out_col += [int(local[col[e]]) for e in kept]
        if normalize == "row" and kept:
            out_val += [np.float32(1.0 / len(kept))] * len(kept)
        elif val is not None:
            out_val += [val[e] for e in kept]
        out_rowptr.append(len(out_col))
    has_val = normalize == "row" or val is not None
    return (np.asarray(out_rowptr, np.int64), np.asarray(out_col, np.int32), np.asarray(out_val, np.float32) if has_val else None,
            np.asarray(out_eid, np.int64))


def draw_words(mode, budget, seed):
    """uint64[budget]: w = x0 << 32 | x1 of Philox4x32-10 with key = seed and counter {i lo, i hi, 0, mode}."""
    i = np.arange(budget, dtype=np.uint64)
    ctr = np.stack([i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), np.zeros(budget, np.uint64), np.full(budget, MODES[mode], np.uint64)], axis=-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = embedding_ref.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    return [(int(a) << 32) | int(b) for a, b in zip(x[:, 0], x[:, 1])]


def saint_draws(rowptr, col, mode, budget, seed):
    """The raw draws: mode "node": the drawn node per draw; "edge": the drawn entry per draw; "walk": the walk matrix
    int32[num_roots, length + 1] (budget = (num_roots, length))."""
    rowptr = np.asarray(rowptr, np.int64)
    n, nnz = len(rowptr) - 1, int(rowptr[-1])
    if mode == "walk":
        roots, length = budget
        starts = np.asarray([(w * n) >> 64 for w in draw_words(mode, roots, seed)], np.int64)
        return embedding_ref.walks(rowptr, col, starts, length + 1, seed=seed, first_walk_index=0)
    entries = np.asarray([(w * nnz) >> 64 for w in draw_words(mode, budget, seed)], np.int64)
    if mode == "edge":
        return entries
    return np.searchsorted(rowptr, entries, side="right") - 1          # the largest v with rowptr[v] <= e


def saint_nodes(rowptr, col, mode, budget, seed):
    """The node set of one SAINT batch: ascending unique int64 ids."""
    d = saint_draws(rowptr, col, mode, budget, seed)
    if mode == "node":
        ids = d
    elif mode == "edge":
        ids = np.concatenate([np.searchsorted(np.asarray(rowptr, np.int64), d, side="right") - 1, np.asarray(col, np.int64)[d]])
    else:
        ids = d.reshape(-1)
        ids = ids[ids >= 0]
    return np.unique(ids.astype(np.int64))


def saint(rowptr, col, val, mode, budget, seed, normalize="row"):
    """(nodes, (rowptr, col, val, eid)) of SAINTSampler.sample_seeded."""
    nodes = saint_nodes(rowptr, col, mode, budget, seed)
    return nodes, node_subgraph(rowptr, col, val, nodes, normalize)


def shadow(rowptr, col, seeds, fanouts, seed, normalize="row", weights=None):
    """(input_nodes, (rowptr, col, val, eid)) of ShaDowKHopSampler.sample_seeded.  weights: the prob= weights per entry; the subgraph
    is then induced on the graph without its zero-weight entries, with the weights as its values."""
    if weights is None:
        inp, _ = neighbor_ref.sample_blocks(rowptr, col, seeds, fanouts, seed, norm=None)
        return inp, node_subgraph(rowptr, col, None, inp, normalize)
    inp, _, gap, (frp, fcol, fw) = neighbor_weighted_ref.sample_blocks(rowptr, col, weights, seeds, fanouts, seed, norm=None)
    assert gap > neighbor_weighted_ref.MIN_GAP
    return inp, node_subgraph(frp, fcol, fw, inp, normalize)
