"""Pure numpy / Python restatement of the edge-prediction sampler (dgll_amd/csrc/edge_pred.hip, dgll_amd/sampling/edge.py) on top of
neighbor_ref -- a helper, not a test.  The only native call is the host Philox; every decision is an integer compare and the one
float is np.float32(1) / np.float32(kept), so the device output is bit-equal."""
import numpy as np

import neighbor_ref as nref

NEG_DOMAIN = 0x40000000


def row_of(rowptr, e):
    """upper_bound(rowptr, e) - 1: runs of empty rows in front of and behind the entry's row are stepped over."""
    return int(np.searchsorted(np.asarray(rowptr), e, side="right")) - 1


def has_edge(rowptr, col, u, c):
    """Is u a source of row c?"""
    return bool(np.any(col[int(rowptr[c]):int(rowptr[c + 1])] == u))


def negative(rowptr, col, n, e, k, seed, filter_existing=False, max_attempts=16):
    """(candidate, capped) of negative k of entry e."""
    e, seed = int(e), int(seed) & (2 ** 64 - 1)
    key = [seed & 0xFFFFFFFF, seed >> 32]
    u, c = int(col[e]), 0
    for a in range(max_attempts):
        x = nref.philox([e & 0xFFFFFFFF, e >> 32, k | NEG_DOMAIN, a], key)
        c = (x[0] * n) >> 32
        if not filter_existing or not has_edge(rowptr, col, u, c):
            return c, False
    return c, True


def pairs_and_negatives(rowptr, col, n, edge_ids, negatives, seed, filter_existing=False, max_attempts=16):
    """(global pairs int64[B * (1 + K), 2], capped flags bool[B * (1 + K)]): the positives in batch order, then negative k of
    positive i in row B + i * K + k."""
    edge_ids = [int(e) for e in np.asarray(edge_ids).reshape(-1)]
    nnz = int(rowptr[-1])
    assert all(0 <= e < nnz for e in edge_ids), "edge id outside [0, nnz)"
    pos = [(int(col[e]), row_of(rowptr, e)) for e in edge_ids]
    neg, capped = [], [False] * len(pos)
    for e in edge_ids:
        for k in range(negatives):
            c, cap = negative(rowptr, col, n, e, k, seed, filter_existing, max_attempts)
            neg.append((int(col[e]), c))
            capped.append(cap)
    return np.asarray(pos + neg, np.int64).reshape(-1, 2), np.asarray(capped, bool)


def compact(gpairs):
    """(output_nodes int64[M] ascending, local pairs int32[P, 2])."""
    out, inv = np.unique(np.asarray(gpairs, np.int64).reshape(-1), return_inverse=True)
    return out.astype(np.int64), inv.reshape(-1, 2).astype(np.int32)


def exclude(block, positives, mode, norm="mean"):
    """The block (a neighbor_ref dict with src / dst) without the entries a -> b with (a, b) in positives (mode "self") or (a, b) or
    (b, a) in positives ("reverse"); None: the block itself.  Kept entries in order, val = 1 / kept, shapes and sources unchanged."""
    if mode is None:
        return block
    gone = {(int(a), int(b)) for a, b in positives}
    if mode == "reverse":
        gone |= {(b, a) for a, b in gone}
    src, rp, cl = block["src"], block["rowptr"], block["col"]
    rowptr, col, val = [0], [], []
    for r in range(block["n_rows"]):
        b = int(src[r])
        keep = [int(c) for c in cl[rp[r]:rp[r + 1]] if (int(src[c]), b) not in gone]
        col += keep
        if keep:
            val += [np.float32(1) / np.float32(len(keep))] * len(keep)
        rowptr.append(len(col))
    out = dict(block)
    out.update(rowptr=np.asarray(rowptr, np.int64), col=np.asarray(col, np.int32),
               val=np.asarray(val, np.float32) if norm == "mean" else None)
    return out


def incidence(pairs, m):
    """(rowptr int64[m + 1], pair int32[2P], other int32[2P]): row i lists (pair, other endpoint) of every slot holding i, ascending by
    (pair, slot)."""
    rows = [[] for _ in range(m)]
    for p, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        rows[int(a)].append((p, int(b)))
        rows[int(b)].append((p, int(a)))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    flat = [x for r in rows for x in r]
    return rowptr, np.asarray([p for p, _ in flat], np.int32), np.asarray([o for _, o in flat], np.int32)


def sample(rowptr, col, n, edge_ids, fanouts, seed, negatives=1, filter_existing=False, exclude_mode=None, max_attempts=16, norm="mean"):
    """The whole front end: a dict {output_nodes, pairs, gpairs, capped, capped_flags, n_pos, n_neg, input_nodes, blocks}."""
    gpairs, flags = pairs_and_negatives(rowptr, col, n, edge_ids, negatives, seed, filter_existing, max_attempts)
    out, pairs = compact(gpairs)
    n_pos = len(np.asarray(edge_ids).reshape(-1))
    inp, blocks = nref.sample_blocks(rowptr, col, out, fanouts, seed, norm)
    blocks = [exclude(b, gpairs[:n_pos], exclude_mode, norm) for b in blocks]
    return {"output_nodes": out, "pairs": pairs, "gpairs": gpairs, "capped": int(flags.sum()), "capped_flags": flags, "n_pos": n_pos,
            "n_neg": len(gpairs) - n_pos, "input_nodes": inp, "blocks": blocks}


def check_invariants(rowptr, col, n, output_nodes, pairs, n_pos, blocks, filter_existing=False, exclude_mode=None, capped_flags=None):
    """The structural contract of one batch: blocks as neighbor_ref dicts (src / dst global ids), pairs local."""
    output_nodes, pairs = np.asarray(output_nodes), np.asarray(pairs).reshape(-1, 2)
    m = len(output_nodes)
    assert np.all(np.diff(output_nodes) > 0)                                        # strictly ascending
    assert m == 0 or (output_nodes[0] >= 0 and output_nodes[-1] < n)
    assert pairs.size == 0 or (pairs.min() >= 0 and pairs.max() < m)                # locals in range
    used = np.zeros(m, bool)
    used[pairs.reshape(-1)] = True
    assert used.all()                                                               # every output node is somebody's endpoint
    g = output_nodes[pairs]
    for u, v in g[:n_pos]:
        assert has_edge(rowptr, col, int(u), int(v))                                # a positive is an entry of the graph
    if filter_existing:
        flags = np.zeros(len(g), bool) if capped_flags is None else np.asarray(capped_flags)
        for (u, c), cap in zip(g[n_pos:], flags[n_pos:]):
            assert cap or not has_edge(rowptr, col, int(u), int(c))                 # no uncapped negative is an edge
    if exclude_mode is not None:
        gone = {(int(a), int(b)) for a, b in g[:n_pos]}
        if exclude_mode == "reverse":
            gone |= {(b, a) for a, b in gone}
        for blk in blocks:
            src, rp, cl = blk["src"], blk["rowptr"], blk["col"]
            assert len(rp) == blk["n_rows"] + 1 and rp[0] == 0 and rp[-1] == len(cl) and np.all(np.diff(rp) >= 0)
            assert len(cl) == 0 or (cl.min() >= 0 and cl.max() < blk["n_cols"])
            for r in range(blk["n_rows"]):
                for c in cl[rp[r]:rp[r + 1]]:
                    assert (int(src[c]), int(src[r])) not in gone                   # no entry is a positive pair (or its reverse)
    if blocks:
        assert np.array_equal(blocks[-1]["dst"], output_nodes)


DEGREES = [0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 24, 25, 26, 63, 64, 65]


def build_graph(n, hub, hub_degree, seed):
    """The recipe of test_neighbor_gpu.build_graph: in-neighbour CSR with sorted, unique columns; node v has degree
    DEGREES[v % 16], `hub` has hub_degree; every 7th node with a neighbour has a self-loop; node n - 1 is a source of every row of
    degree >= 3 (13 rows in 16)."""
    rng = np.random.default_rng(seed)
    rows = []
    for v in range(n):
        d = hub_degree if v == hub else DEGREES[v % len(DEGREES)]
        forced = []
        if d >= 1 and v % 7 == 0:
            forced.append(v)
        if d >= 3 and v != n - 1:
            forced.append(n - 1)
        pool = np.setdiff1d(np.arange(n), forced)
        rows.append(np.sort(np.concatenate([np.asarray(forced, np.int64), rng.choice(pool, d - len(forced), replace=False)])))
        assert len(rows[-1]) == d
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rowptr, np.concatenate(rows).astype(np.int32), n
