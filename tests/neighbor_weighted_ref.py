"""Numpy restatement of the edge-weighted neighbour draw (dgll_hip_nb_sample_weighted, dgll_amd/csrc/neighbor.hip) -- a helper, not a
test.  The random words come from the host Philox (dgll_host_philox4x32_10); device and host agree on every integer decision, and the
only floating-point steps are log, a conversion and a division (three roundings of at most 2^-52 relative each), so a kept set can
differ from the device's only where the relative gap between the last kept key and the first rejected key is below about 1e-15.
sample_blocks returns the smallest such gap over the rows it sampled: a test asserts it is above MIN_GAP and then demands bit
equality."""
import ctypes
import functools
import itertools

import numpy as np

import neighbor_ref as ref

MIN_GAP = 1e-9
_KEYS = {}          # (v, layer, seed, weights of the row) -> keys: a node's keys do not depend on the batch or the fan-out


def build_graph(n, special, seed, degrees=(0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 24, 25, 26, 63, 64, 65)):
    """In-neighbour CSR (sorted, unique columns) as test_neighbor_gpu.build_graph: node v has degree degrees[v % 16], the nodes
    of `special` ({node: degree}) theirs; self-loops at every 7th node, the last node a neighbour of every row of degree >= 3."""
    rng = np.random.default_rng(seed)
    rows = []
    for v in range(n):
        d = special.get(v, degrees[v % len(degrees)])
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


POSITIVE_COUNTS = (0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 24, 25, 26, 63, 64, 65)     # 0 and f - 1, f, f + 1 of every fan-out used


def build_weights(rowptr, seed, zero_every=3, keep_whole=()):
    """fp32 weights 2^x, x uniform in [-20, 31); every `zero_every`-th node, when its degree d is >= 2, keeps k positive weights and
    0 elsewhere, k cycling per degree through the POSITIVE_COUNTS below d: rows of weight 0 throughout, rows with fewer positive
    weights than a fan-out, exactly as many, one more.  The nodes of `keep_whole` keep every weight."""
    rng = np.random.default_rng(seed)
    w = np.exp2(rng.uniform(-20.0, 31.0, int(rowptr[-1]))).astype(np.float32)
    turn = {}
    for v in range(0, len(rowptr) - 1, zero_every):
        b, d = int(rowptr[v]), int(rowptr[v + 1] - rowptr[v])
        if d < 2 or v in keep_whole:
            continue
        below = [k for k in POSITIVE_COUNTS if k < d]
        keep = below[turn.get(d, 0) % len(below)]
        turn[d] = turn.get(d, 0) + 1
        w[b + rng.choice(d, d - keep, replace=False)] = 0.0
    return w


def drop_zero_weights(rowptr, col, w):
    """The CSR without its zero-weight entries, order kept."""
    keep = np.asarray(w) > 0
    below = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    return below[np.asarray(rowptr)], np.asarray(col)[keep], np.asarray(w, np.float32)[keep]


def row_keys(v, layer, seed, w_row):
    """fp64 keys -log(u) / w of the positions of node v's row: one Philox call per position, counter (v lo, v hi, layer | 2^31, p)."""
    from dgll_amd import _lib

    v, seed = int(v), int(seed) & (2 ** 64 - 1)
    w_row = np.ascontiguousarray(w_row, np.float32)
    tag = (v, int(layer), seed, w_row.tobytes())
    if tag not in _KEYS:
        assert np.all(w_row > 0) and np.all(np.isfinite(w_row))
        fn = _lib.lib.dgll_host_philox4x32_10
        ctr = np.array([v & 0xFFFFFFFF, v >> 32, int(layer) | 0x80000000, 0], np.uint32)
        key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)
        out = np.zeros((len(w_row), 4), np.uint32)
        cp, kp, stride = ctypes.c_void_p(ctr.ctypes.data), ctypes.c_void_p(key.ctypes.data), out.strides[0]
        for p in range(len(w_row)):
            ctr[3] = p
            assert fn(cp, kp, ctypes.c_void_p(out.ctypes.data + p * stride)) == 0
        bits = ((out[:, 0].astype(np.uint64) << np.uint64(32)) | out[:, 1].astype(np.uint64)) >> np.uint64(11)
        u = (bits.astype(np.float64) + 0.5) * 2.0 ** -53
        _KEYS[tag] = -np.log(u) / w_row.astype(np.float64)
    return _KEYS[tag]


def positions(w_row, v, fanout, seed, layer):
    """(kept positions ascending, gap): the `fanout` smallest by (key bits as uint64, position); gap = (k[f] - k[f-1]) / k[f] of the
    sorted keys, None for a row that is copied."""
    d = len(w_row)
    if fanout < 0 or d <= fanout:
        return list(range(d)), None
    k = row_keys(v, layer, seed, w_row)
    order = np.lexsort((np.arange(d), k.view(np.uint64)))
    ks = k[order]
    return sorted(int(p) for p in order[:fanout]), float((ks[fanout] - ks[fanout - 1]) / ks[fanout])


def draw(rowptr, col, w, v, fanout, seed, layer):
    """(global ids of the kept in-neighbours of v in ascending position, gap) on a CSR WITHOUT zero weights."""
    b, e = int(rowptr[v]), int(rowptr[v + 1])
    pos, gap = positions(w[b:e], v, fanout, seed, layer)
    return [int(col[b + p]) for p in pos], gap


def sample_blocks(rowptr, col, w, seeds, fanouts, seed, norm="mean"):
    """(input_nodes, blocks, smallest gap, filtered CSR): neighbor_ref.sample_blocks with the weighted draw on the filtered graph."""
    frp, fcol, fw = drop_zero_weights(rowptr, col, w)
    rows = np.asarray(seeds, np.int64).reshape(-1)
    blocks, min_gap = [], np.inf
    for layer in range(len(fanouts) - 1, -1, -1):
        drawn = []
        for v in rows:
            ids, gap = draw(frp, fcol, fw, int(v), fanouts[layer], seed, layer)
            drawn.append(ids)
            min_gap = min_gap if gap is None else min(min_gap, gap)
        src, rp, cl, vl = ref.to_block(rows, drawn, norm)
        blocks.append({"rowptr": rp, "col": cl, "val": vl, "n_rows": len(rows), "n_cols": len(src), "dst": rows, "src": src})
        rows = src
    blocks.reverse()
    return rows, blocks, min_gap, (frp, fcol, fw)


# ---- the distribution case: 20 000 rows that list the same 7 neighbours, fan-out 3 ------------------------------------------------
DIST_WEIGHTS = (0.38, 0.24, 0.16, 0.11, 0.07, 0.04, 0.0)
DIST_ROWS, DIST_FANOUT, DIST_SEED = 20000, 3, 20241018


def dist_graph():
    """Rows 0 .. DIST_ROWS-1 each list the nodes DIST_ROWS .. DIST_ROWS+6 with DIST_WEIGHTS."""
    k = len(DIST_WEIGHTS)
    n = DIST_ROWS + k
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:DIST_ROWS + 1] = k
    return (np.cumsum(rowptr), np.tile(np.arange(DIST_ROWS, n, dtype=np.int32), DIST_ROWS),
            np.tile(np.asarray(DIST_WEIGHTS, np.float32), DIST_ROWS), n)


def set_probabilities(p, f):
    """Plackett-Luce probability of every f-subset of range(len(p)), summed over its orders."""
    p = np.asarray(p, np.float64) / np.sum(p)
    out = {}
    for t in itertools.permutations(range(len(p)), f):
        q, left = 1.0, 1.0
        for i in t:
            q *= p[i] / left
            left -= p[i]
        out[tuple(sorted(t))] = out.get(tuple(sorted(t)), 0.0) + q
    return out


def check_set_counts(kept_sets):
    """kept_sets: one sorted tuple of neighbour indices (0 .. 6) per row.  The zero-weight neighbour never appears and the counts of
    the 20 possible sets follow Plackett-Luce: Pearson's statistic below the chi-square 0.9999 quantile, bins whose expectation is
    under 5 pooled.  Returns the statistic."""
    from scipy import stats

    assert len(kept_sets) == DIST_ROWS
    counts = {}
    for t in kept_sets:
        assert len(t) == DIST_FANOUT and len(set(t)) == DIST_FANOUT and max(t) < 6, t
        counts[t] = counts.get(t, 0) + 1
    prob = set_probabilities(DIST_WEIGHTS[:6], DIST_FANOUT)
    assert len(prob) == 20 and abs(sum(prob.values()) - 1.0) < 1e-12 and set(counts) <= set(prob)
    exp = np.array([prob[t] * DIST_ROWS for t in sorted(prob)])
    obs = np.array([counts.get(t, 0) for t in sorted(prob)])
    big = exp >= 5
    e, o = exp[big], obs[big]
    if (~big).any():
        e, o = np.append(e, exp[~big].sum()), np.append(o, obs[~big].sum())
    chi2 = float(((o - e) ** 2 / e).sum())
    bound = float(stats.chi2.ppf(0.9999, len(e) - 1))
    print("pearson", chi2, "bound", bound, "bins", len(e))
    assert chi2 < bound, (chi2, bound)
    return chi2


@functools.lru_cache(maxsize=None)
def dist_reference():
    """(kept sets of the restatement per row, smallest gap) under DIST_SEED."""
    rowptr, col, w, n = dist_graph()
    frp, fcol, fw = drop_zero_weights(rowptr, col, w)
    sets, min_gap = [], np.inf
    for v in range(DIST_ROWS):
        ids, gap = draw(frp, fcol, fw, v, DIST_FANOUT, DIST_SEED, 0)
        sets.append(tuple(sorted(i - DIST_ROWS for i in ids)))
        min_gap = min(min_gap, gap)
    return sets, min_gap
