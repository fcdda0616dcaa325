"""Host restatement of struc2vec as dgll_amd.embedding builds it, in numpy float64: ordered degree lists, pair selection, the
exact DTW, the multilayer context graph with its normalised weights, gamma and up-move thresholds, and the layer-carrying walker
(built on embedding_ref.philox4x32_10 and weighted_walk_ref.alias_draw: every decision an integer compare, so it is bit-exact
against the device for the same tables)."""
import math
import os
from collections import deque

import numpy as np

import embedding_ref as ref
import weighted_walk_ref as wref

SETTINGS = [(True, True, 3), (False, True, 3), (True, False, None)]          # (opt1, opt2, opt3) of the golden's three cases


def degree_lists(rowptr, col, reduce_len=True, num_layers=None):
    """[v][level] -> ascending list of (degree, count) (count 1 per node when not reduce_len); levels 0..num_layers."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    out = []
    for root in range(n):
        seen = np.zeros(n, dtype=bool)
        seen[root] = True
        queue, levels = deque([root]), []
        while queue and (num_layers is None or len(levels) <= num_layers):
            ring = [queue.popleft() for _ in range(len(queue))]
            for v in ring:
                for u in col[rowptr[v]:rowptr[v + 1]]:
                    if not seen[u]:
                        seen[u] = True
                        queue.append(int(u))
            d = np.sort(deg[ring])
            if reduce_len:
                vals, cnt = np.unique(d, return_counts=True)
                levels.append(list(zip(vals.tolist(), cnt.tolist())))
            else:
                levels.append([(int(x), 1) for x in d])
        out.append(levels)
    return out


def select_pairs(deg, reduce_sim_calc=True):
    """Ordered list of (v, u): own degree first, then the nearest other degrees (a tie goes to the larger), until more than
    2 log2 N partners are taken; or all v < u."""
    deg = [int(d) for d in deg]
    n = len(deg)
    if not reduce_sim_calc:
        return [(v, u) for v in range(n) for u in range(v + 1, n)]
    by_degree = {}
    for v, d in enumerate(deg):
        by_degree.setdefault(d, []).append(v)
    ladder = sorted(by_degree)
    want = 2 * math.log(n, 2)
    pairs = []
    for v, d in enumerate(deg):
        taken = 0
        at = ladder.index(d)
        lo, hi = at - 1, at + 1
        cur = at
        while True:
            full = False
            for u in by_degree[ladder[cur]]:
                if u != v:
                    pairs.append((v, u))
                    taken += 1
                    if taken > want:
                        full = True
                        break
            if full:
                break
            if cur != at:
                if cur == lo:
                    lo -= 1
                else:
                    hi += 1
            has_lo, has_hi = lo >= 0, hi < len(ladder)
            if not has_lo and not has_hi:
                break
            if not has_lo:
                cur = hi
            elif not has_hi:
                cur = lo
            else:
                cur = lo if abs(ladder[lo] - d) < abs(ladder[hi] - d) else hi
    return pairs


def dtw(a, b):
    """Exact DTW distance of two lists of (degree, count) in float64, cell by cell as the kernel computes it (the anti-diagonals
    are evaluated as vectors; every cell is the same three operations)."""
    da, ca = np.array([x[0] for x in a], np.float64), np.array([x[1] for x in a], np.float64)
    db, cb = np.array([x[0] for x in b], np.float64), np.array([x[1] for x in b], np.float64)
    m, n = len(da), len(db)
    hi, lo = np.maximum(da[:, None], db[None, :]) + 0.5, np.minimum(da[:, None], db[None, :]) + 0.5
    c = (hi / lo - 1.0) * np.maximum(ca[:, None], cb[None, :])
    D = np.full((m + 1, n + 1), np.inf)
    D[0, 0] = 0.0
    for k in range(m + n - 1):
        i = np.arange(max(0, k - n + 1), min(m - 1, k) + 1)
        j = k - i
        D[i + 1, j + 1] = c[i, j] + np.minimum(np.minimum(D[i, j + 1], D[i + 1, j]), D[i, j])
    return float(D[m, n])


def pair_distances(lists, pairs):
    """float64 [P, Lmax]: cumulative DTW distance of every pair at every layer both nodes have, -1 elsewhere."""
    n_layers = max(len(x) for x in lists)
    out = np.full((len(pairs), n_layers), -1.0)
    for p, (v, u) in enumerate(pairs):
        total = 0.0
        for l in range(min(len(lists[v]), len(lists[u]))):
            step = dtw(lists[v][l], lists[u][l])
            total = step if l == 0 else total + step
            out[p, l] = total
    return out


def context(dist, pairs, n_nodes):
    """The stacked graph of the layers from the cumulative distances: dict with rowptr [L N + 1], col, d (the distance of every
    stacked edge), shifted (exp(-(d - row min))), norm (shifted / row sum), average [L], gamma [L N]."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n_layers = dist.shape[1]
    pi, li = np.nonzero(dist >= 0)
    rows = np.concatenate([li * n_nodes + pairs[pi, 0], li * n_nodes + pairs[pi, 1]])
    col = np.concatenate([pairs[pi, 1], pairs[pi, 0]])
    d = np.concatenate([dist[pi, li], dist[pi, li]])
    order = np.argsort(rows, kind="stable")
    rows, col, d = rows[order], col[order], d[order]
    n_rows = n_layers * n_nodes
    rowptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=rowptr[1:])
    d_min = np.full(n_rows, np.inf)
    np.minimum.at(d_min, rows, d)
    shifted = np.exp(-(d - d_min[rows]))
    norm = shifted / np.bincount(rows, weights=shifted, minlength=n_rows)[rows]
    layer = rows // n_nodes
    count = np.bincount(layer, minlength=n_layers)
    average = np.bincount(layer, weights=norm, minlength=n_layers) / np.maximum(count, 1)
    gamma = np.bincount(rows, weights=(norm > average[layer]).astype(np.float64), minlength=n_rows).astype(np.int64)
    return dict(rowptr=rowptr, col=col.astype(np.int32), d=d, shifted=shifted, norm=norm, average=average, gamma=gamma,
                n_layers=n_layers, n_nodes=n_nodes)


def up_thresholds(gamma):
    x = np.log(np.asarray(gamma, dtype=np.float64) + math.e)
    return np.rint(4294967296.0 * (x / (x + 1.0))).astype(np.uint64).astype(np.uint32)


def up_probability(gamma):
    x = np.log(np.asarray(gamma, dtype=np.float64) + math.e)
    return x / (x + 1.0)


def build(rowptr, col, opt1=True, opt2=True, opt3=None):
    """Sections 1-4 in one call: (lists, pairs, dist, context dict)."""
    lists = degree_lists(rowptr, col, opt1, opt3)
    pairs = select_pairs(np.diff(np.asarray(rowptr, np.int64)), opt2)
    dist = pair_distances(lists, pairs)
    return lists, pairs, dist, context(dist, pairs, len(rowptr) - 1)


def walks(rowptr, col, T, alias, t_up, n_nodes, n_layers, starts, length, stay_prob, seed=0, first_walk_index=0,
          max_attempts=ref.MAX_ATTEMPTS, moves=None):
    """(walks int32 [n, length], layers int32 [n, length], attempts that reached the cap): struc_walk_kernel restated.
    moves: optional int64 [2, n_layers * n_nodes] that receives, per row, the layer-move attempts and how many of them drew "up"."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    T, alias, t_up = np.asarray(T, np.uint32), np.asarray(alias, np.uint32), np.asarray(t_up, np.uint32).astype(np.uint64)
    starts = np.asarray(starts, np.int64)
    n = len(starts)
    t_stay = np.uint64(int(np.rint(4294967296.0 * float(stay_prob))))
    out = np.full((n, length), -1, dtype=np.int32)
    lay = np.full((n, length), -1, dtype=np.int32)
    out[:, 0], lay[:, 0] = starts, 0
    widx = np.uint64(first_walk_index) + np.arange(n, dtype=np.uint64)
    key = ref._key(seed)
    v, layer = starts.copy(), np.zeros(n, dtype=np.int64)
    capped = 0
    for s in range(1, length):
        nxt = np.full(n, -1, dtype=np.int64)
        pending = np.nonzero(v >= 0)[0]
        a = 0
        while pending.size and a < max_attempts:
            x = ref.philox4x32_10(ref._counters(widx[pending], s, a), key).astype(np.uint64)
            last = a == max_attempts - 1
            if last:
                capped += pending.size
            row = layer[pending] * n_nodes + v[pending]
            stay = (x[:, 0] < t_stay) | last
            sp, srow, sx = pending[stay], row[stay], x[stay]
            ok = rowptr[srow + 1] > rowptr[srow]                                  # an empty row ends the walk
            sp, srow, sx = sp[ok], srow[ok], sx[ok]
            e = wref.alias_draw(rowptr, T, alias, srow, sx[:, 1], sx[:, 2])
            live = e >= 0                                                         # a dead row ends it too
            nxt[sp[live]] = col[rowptr[srow[live]] + e[live]]
            mp, mrow, mx = pending[~stay], row[~stay], x[~stay, 3]
            up = mx < t_up[mrow]
            if moves is not None:
                np.add.at(moves[0], mrow, 1)
                np.add.at(moves[1], mrow[up], 1)
            above = np.minimum(mrow + n_nodes, len(rowptr) - 2)
            can = up & (layer[mp] + 1 < n_layers) & (rowptr[above + 1] > rowptr[above])
            down = ~up & (layer[mp] > 0)
            layer[mp[can]] += 1
            layer[mp[down]] -= 1
            pending = mp
            a += 1
        v = nxt
        out[:, s] = v
        lay[:, s] = np.where(v >= 0, layer, -1)
    return out, lay, capped


def frequency_excess(count, n, P, min_visits=500, share=0.9):
    """The rule of test_embedding_host.transition_check on plain arrays: per cell |count / n - P| against 5 sqrt(P (1 - P) / n) +
    1 / n, cells with n >= min_visits only, and at least `share` of the cells with mass must qualify.
    Returns (cells checked, cells with mass, worst excess over the cap)."""
    count, n, P = np.asarray(count, np.float64), np.asarray(n, np.float64), np.asarray(P, np.float64)
    mass = P > 0
    assert not count[~mass].any(), "a transition of probability 0 was taken"
    ok = mass & (n >= min_visits)
    assert ok.sum() >= share * mass.sum(), (int(ok.sum()), int(mass.sum()))
    p, m = P[ok], n[ok]
    excess = np.abs(count[ok] / m - p) - (5.0 * np.sqrt(p * (1.0 - p) / m) + 1.0 / m)
    return int(ok.sum()), int(mass.sum()), float(excess.max())


def stay_cells(rowptr, col, norm, n_nodes, layers=(0, 1)):
    """The (row, neighbour) cells of the given layers with their probability (duplicate neighbours merged):
    (cell key row * n_nodes + u ascending, P)."""
    rowptr = np.asarray(rowptr, np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    keep = np.isin(rows // n_nodes, layers)
    key = rows[keep] * n_nodes + np.asarray(col, np.int64)[keep]
    uniq, inverse = np.unique(key, return_inverse=True)
    return uniq, np.bincount(inverse, weights=np.asarray(norm, np.float64)[keep], minlength=len(uniq))


def stay_frequencies(walk_arr, layer_arr, cells, n_nodes):
    """(count per cell, stay steps of the cell's row): entry s was emitted from (layer_arr[s], walk_arr[s - 1])."""
    w, l = np.asarray(walk_arr, np.int64), np.asarray(layer_arr, np.int64)
    took = w[:, 1:] >= 0
    row = (l[:, 1:] * n_nodes + w[:, :-1])[took]
    key = row * n_nodes + w[:, 1:][took]
    inside = np.isin(row, cells // n_nodes)
    row, key = row[inside], key[inside]
    pos = np.searchsorted(cells, key)
    assert np.array_equal(cells[np.minimum(pos, len(cells) - 1)], key), "a step along an edge the layer does not have"
    count = np.bincount(pos, minlength=len(cells))
    rows_u, visits = np.unique(row, return_counts=True)
    at = np.searchsorted(rows_u, cells // n_nodes)
    hit = (at < len(rows_u)) & (rows_u[np.minimum(at, max(len(rows_u) - 1, 0))] == cells // n_nodes) if len(rows_u) else np.zeros(len(cells), bool)
    n = np.where(hit, visits[np.minimum(at, max(len(rows_u) - 1, 0))], 0) if len(rows_u) else np.zeros(len(cells), np.int64)
    return count, n


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "struc2vec_context.npz")
