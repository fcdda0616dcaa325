"""Host restatements of the edge-weighted walks of dgll_amd.embedding: the alias draw and the weighted walker in numpy, given a
table (T, alias) as input (every decision an integer compare, so they are bit-exact against the device for the same table); a
float64 Vose builder for tests that run without a GPU (it need not give the device's bits: any valid table implies the same
distribution); and the distribution a table implies, in exact integers."""
import numpy as np

import embedding_ref as ref

FULL = 0xFFFFFFFF            # the threshold of a slot that always keeps itself (it is its own alias)


def build_alias(rowptr, val):
    """Vose's construction per row in float64: (T uint32 [nnz], alias uint32 [nnz], alias local to the row).  A row whose weights
    sum to 0 holds {0, slot} in every slot."""
    rowptr = np.asarray(rowptr, np.int64)
    val = np.asarray(val, np.float64)
    if not (np.isfinite(val).all() and (val >= 0).all()):
        raise ValueError("weights must be finite and >= 0")
    T = np.zeros(len(val), dtype=np.uint32)
    alias = np.zeros(len(val), dtype=np.uint32)
    for r in range(len(rowptr) - 1):
        b, e = int(rowptr[r]), int(rowptr[r + 1])
        deg = e - b
        w = val[b:e]
        total = float(w.sum())
        if deg == 0:
            continue
        if not total > 0.0:
            alias[b:e] = np.arange(deg)
            continue
        q = (w * (deg / total)).tolist()
        small = [j for j in range(deg) if q[j] < 1.0]
        large = [j for j in range(deg) if q[j] >= 1.0]
        while small and large:
            l, g = small.pop(), large[-1]
            T[b + l] = min(int(np.rint(q[l] * 4294967296.0)), FULL)
            alias[b + l] = g
            q[g] = (q[g] + q[l]) - 1.0
            if q[g] < 1.0:
                small.append(large.pop())
        top = int(np.argmax(w))
        for j in small + large:
            T[b + j], alias[b + j] = (FULL, j) if w[j] > 0.0 else (0, top)
    return T, alias


def implied_probs(rowptr, T, alias):
    """float64 [nnz]: the probability with which a draw from the table returns every edge,
    [T_e + sum over slots l of the row with alias_l = e of (2^32 - T_l)] / (deg 2^32), a self-aliased slot counted as full (2^32)
    -- except the {0, slot} entries of a row whose weights sum to 0, which count as nothing.  The numerators are exact integers."""
    rowptr = np.asarray(rowptr, np.int64)
    T = np.asarray(T).astype(np.int64)
    alias = np.asarray(alias).astype(np.int64)
    deg = np.diff(rowptr)
    begin = np.repeat(rowptr[:-1], deg)
    slot = np.arange(len(T), dtype=np.int64) - begin
    own = alias == slot
    dead = own & (T == 0)
    num = np.where(own, np.where(dead, 0, 1 << 32), T)
    give = ~own
    np.add.at(num, begin[give] + alias[give], (1 << 32) - T[give])
    return num.astype(np.float64) / (np.repeat(deg, deg).astype(np.float64) * 4294967296.0)


def alias_draw(rowptr, T, alias, v, x0, x1):
    """Edge offset inside row v (int64, -1 for a row whose weights sum to 0) of the draw with words x0, x1 (uint64 arrays holding
    32-bit words); every v has deg > 0."""
    b = rowptr[v]
    deg = (rowptr[v + 1] - b).astype(np.uint64)
    slot = ((x0 * deg) >> np.uint64(32)).astype(np.int64)
    t, al = T[b + slot].astype(np.uint64), alias[b + slot].astype(np.int64)
    e = np.where(x1 < t, slot, al)
    return np.where((t == 0) & (al == slot), -1, e)


def walks(rowptr, col, T, alias, starts, length, p=1.0, q=1.0, seed=0, first_walk_index=0, max_attempts=ref.MAX_ATTEMPTS,
          return_capped=False):
    """int32 [n, length]: embedding_ref.walks with the candidate of every attempt drawn from the table and word 2 as the acceptance
    word; rows of the CSR ascend."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    T, alias = np.asarray(T, np.uint32), np.asarray(alias, np.uint32)
    n_nodes = len(rowptr) - 1
    deg = np.diff(rowptr)
    edge_key = np.repeat(np.arange(n_nodes, dtype=np.int64), deg) * n_nodes + col
    starts = np.asarray(starts, np.int64)
    n = len(starts)
    out = np.full((n, length), -1, dtype=np.int32)
    out[:, 0] = starts
    widx = np.uint64(first_walk_index) + np.arange(n, dtype=np.uint64)
    key = ref._key(seed)
    thr3 = ref.thresholds(p, q)
    biased = not (p == 1.0 and q == 1.0)
    v, t = starts.copy(), np.full(n, -1, dtype=np.int64)
    capped = 0
    for s in range(1, length):
        nxt = np.full(n, -1, dtype=np.int64)
        vs = np.where(v >= 0, v, 0)
        pending = np.nonzero((v >= 0) & (deg[vs] > 0))[0]
        a = 0
        while pending.size and a < max_attempts:
            x = ref.philox4x32_10(ref._counters(widx[pending], s, a), key).astype(np.uint64)
            vp = v[pending]
            e = alias_draw(rowptr, T, alias, vp, x[:, 0], x[:, 1])
            live = e >= 0
            pending, vp, e, x = pending[live], vp[live], e[live], x[live]          # a dead row: the walk ends, -1 stays
            cand = col[rowptr[vp] + e]
            nxt[pending] = cand
            if not biased or s == 1:
                break
            tp = t[pending]
            k = tp * n_nodes + cand
            pos = np.searchsorted(edge_key, k)
            common = (pos < len(edge_key)) & (edge_key[np.minimum(pos, len(edge_key) - 1)] == k)
            thr = np.where(cand == tp, thr3[0], np.where(common, thr3[1], thr3[2]))
            pending = pending[~(x[:, 2] < thr)]
            a += 1
            if a == max_attempts:
                capped += pending.size
        t, v = v, nxt
        out[:, s] = v
    return (out, capped) if return_capped else out


SHAPE_DEGREES = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129)
SHAPE_KINDS = ("equal", "dominant", "some_zero", "all_zero")
SHAPE_LONG = 4097


def shapes_graph(seed=3):
    """The CSR the table tests share: one row of every degree in SHAPE_DEGREES for every kind in SHAPE_KINDS -- equal weights, one
    weight 10^6 times the rest, about a third of the weights 0 (never all), all weights 0 -- then one row of 4 097 entries whose
    first weight is 10^6 times the rest with a few zeros among the rest, then nodes without out-edges: 6 425 edges in all.
    Returns (rowptr int64, col int32 ascending in every row, val float32, kind of every row with edges or None)."""
    rng = np.random.default_rng(seed)
    n_nodes = SHAPE_LONG + 103
    rows = [(d, k) for d in SHAPE_DEGREES for k in SHAPE_KINDS] + [(SHAPE_LONG, "dominant")]
    rowptr = np.zeros(n_nodes + 1, dtype=np.int64)
    col, val, kinds = [], [], [None] * n_nodes
    for r, (d, kind) in enumerate(rows):
        kinds[r] = kind
        col.append(np.sort(rng.choice(n_nodes, d, replace=False)).astype(np.int32))
        if kind == "equal":
            w = np.full(d, 0.75, dtype=np.float32)
        elif kind == "dominant":
            w = np.full(d, 0.75, dtype=np.float32)
            if d:
                w[0 if d == SHAPE_LONG else d // 2] = 750000.0
            if d == SHAPE_LONG:
                w[rng.choice(np.arange(1, d), 5, replace=False)] = 0.0
        elif kind == "some_zero":
            w = rng.uniform(0.5, 2.0, d).astype(np.float32)
            if d > 1:
                w[rng.choice(d, max(1, d // 3), replace=False)] = 0.0
        else:
            w = np.zeros(d, dtype=np.float32)
        val.append(w)
        rowptr[r + 1] = rowptr[r] + d
    rowptr[len(rows) + 1:] = rowptr[len(rows)]
    return rowptr, np.concatenate(col), np.concatenate(val), kinds
