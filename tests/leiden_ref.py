"""Host restatement of dgll_amd.community's Leiden in numpy, on top of louvain_ref (local moving, admission, aggregation): the
refinement sweep (what dgll_hip_leiden_refine writes), the refinement of a level and the level loop, with the same float64
expressions evaluated left to right, the same tie-breaks and the same admission, so targets, sums and labels are bit-equal to the
device's.  `disconnected` counts the communities that fall into pieces."""
import numpy as np

import louvain_ref as lref


def refine_targets(rowptr, col, w, k, size, sub, bound, tot, csize, cnt, totP, two_m, resolution, cap):
    """(target int32 [n], wS, wC, cut int64 [n]): what dgll_hip_leiden_refine writes.  Entries with a column outside [0, n) are
    skipped, as there."""
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    colv = np.asarray(col, dtype=np.int64)
    wt = np.ones(colv.size, np.int64) if w is None else np.asarray(w, dtype=np.int64)
    s, p = np.asarray(sub, dtype=np.int64), np.asarray(bound, dtype=np.int64)
    keep = (colv != row) & (colv >= 0) & (colv < n)                       # self-loop entries count in k only
    keep[keep] = p[colv[keep]] == p[row[keep]]                            # only entries inside the bound community count
    r, c, x = row[keep], colv[keep], wt[keep]
    wC, wS, cut = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    np.add.at(wC, r, x)
    own = s[c] == s[r]
    np.add.at(wS, r[own], x[own])
    np.add.at(cut, s, wC - wS)
    pair, W = lref.segment_sums(r * n + s[c], x)
    pr, pc = pair // n, pair % n
    kf, m2, res = k.astype(np.float64), np.float64(two_m), np.float64(resolution)
    tp = totP[p]                                                          # per node: the weight of its bound community
    node_ok = (cnt[s] == 1) & (wC.astype(np.float64) >= res * kf * (tp - k).astype(np.float64) / m2)
    sub_ok = cut[pc].astype(np.float64) >= res * tot[pc].astype(np.float64) * (tp[pr] - tot[pc]).astype(np.float64) / m2
    gain = W.astype(np.float64) - res * kf[pr] * tot[pc].astype(np.float64) / m2
    ok = (pc != s[pr]) & node_ok[pr] & sub_ok & (csize[pc] + size[pr] <= cap) & (gain > 0.0)
    ok &= ~((cnt[pc] == 1) & (pc > s[pr]))                                # two singletons: only the larger id moves
    idx = np.nonzero(ok)[0]
    idx = idx[np.lexsort((pc[idx], -gain[idx], pr[idx]))]                 # per row: largest gain, then smallest id
    first = np.concatenate(([True], pr[idx][1:] != pr[idx][:-1])) if idx.size else np.zeros(0, bool)
    target = np.asarray(sub, dtype=np.int32).copy()
    target[pr[idx[first]]] = pc[idx[first]]
    return target, wS, wC, cut


def settle(sub, target):
    """Targets stay: a would-be mover whose own sub-community is somebody's target keeps it."""
    want = target != sub
    aimed = np.zeros(len(sub), dtype=bool)
    aimed[target[want]] = True
    return np.where(want & ~aimed[sub], target, sub).astype(np.int32)


def refine(rowptr, col, w, k, size, bound, two_m, resolution, cap, max_sweeps=32, level=0, on_refine=None):
    """int32 [n]: the sub-communities of a level, every one inside one community of `bound` and connected."""
    n = len(rowptr) - 1
    sub = np.arange(n, dtype=np.int32)
    totP = np.zeros(n, np.int64)
    np.add.at(totP, bound, k)
    for sweep in range(max_sweeps):
        tot, csize, cnt = lref.community_state(k, size, sub, n)
        target = refine_targets(rowptr, col, w, k, size, sub, bound, tot, csize, cnt, totP, two_m, resolution, cap)[0]
        movers, t = lref.admit(sub, settle(sub, target), size, csize, cap)
        sub[movers] = t
        if on_refine is not None:
            on_refine(level, sweep, sub, bound, size)
        if movers.size == 0:
            break
    return sub


def local_moving(rowptr, col, w, k, size, comm, two_m, resolution, cap, seed, level, max_sweeps, on_sweep=None):
    """louvain_ref.louvain's sweeps of one level, from the communities given; `comm` is updated in place and returned."""
    n = len(rowptr) - 1
    for sweep in range(max_sweeps):
        tot, csize, cnt = lref.community_state(k, size, comm, n)
        target = lref.move_targets(rowptr, col, w, k, size, comm, tot, csize, cnt, two_m, resolution, cap, seed, level, sweep,
                                   sweep == max_sweeps - 1)
        movers, t = lref.admit(comm, target, size, csize, cap)
        comm[movers] = t
        if on_sweep is not None:
            on_sweep(level, sweep, comm, size)
        if sweep >= 2 and movers.size < max(n // 1000, 1):
            break
    return comm


def coarsen(rowptr, col, w, k, size, dense, nc):
    """The level's graph aggregated on the dense labels: (rowptr, col, w, k, size)."""
    rowptr, col, w = lref.aggregate(rowptr, col, w, dense, nc)
    k2, s2 = np.zeros(nc, np.int64), np.zeros(nc, np.int64)
    np.add.at(k2, dense, k)
    np.add.at(s2, dense, size)
    return rowptr, col, w, k2, s2


def leiden(rowptr, col, max_comm_size=None, resolution=1.0, seed=0, max_levels=20, max_sweeps=32, on_sweep=None, on_refine=None,
           stats=None):
    """int64 [n] dense labels.  stats: a list that receives one (nodes, communities, sub-communities) per level."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
    n = len(rowptr) - 1
    cap = n if max_comm_size is None else int(max_comm_size)
    labels = np.arange(n, dtype=np.int64)
    if col.size == 0:
        return labels
    w, k, size = None, np.diff(rowptr).astype(np.int64), np.ones(n, np.int64)
    two_m = int(k.sum())
    comm = np.arange(n, dtype=np.int32)
    for level in range(max_levels):
        nl = len(rowptr) - 1
        comm = local_moving(rowptr, col, w, k, size, comm, two_m, resolution, cap, seed, level, max_sweeps, on_sweep)
        uniq, dense = np.unique(comm, return_inverse=True)
        if uniq.size == nl:                                               # every community is one (connected) supernode
            if stats is not None:
                stats.append((nl, uniq.size, nl))
            return dense.astype(np.int64)[labels]
        sub = refine(rowptr, col, w, k, size, comm, two_m, resolution, cap, max_sweeps, level, on_refine)
        usub, dsub = np.unique(sub, return_inverse=True)
        dsub = dsub.astype(np.int64)
        if stats is not None:
            stats.append((nl, uniq.size, usub.size))
        labels = dsub[labels]
        if usub.size == nl or level == max_levels - 1:
            return labels
        comm = np.zeros(usub.size, np.int32)
        comm[dsub] = dense                                                # the bound communities carried onto the supernodes
        rowptr, col, w, k, size = coarsen(rowptr, col, w, k, size, dsub, usub.size)
    return labels


def disconnected(rowptr, col, labels):
    """Connected components of the graph restricted to the entries inside a community, minus the number of communities: 0 when
    every community is connected."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components

    n = len(rowptr) - 1
    lab = np.asarray(labels, dtype=np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    colv = np.asarray(col, dtype=np.int64)
    keep = lab[row] == lab[colv]
    inside = csr_matrix((np.ones(int(keep.sum()), np.int8), (row[keep], colv[keep])), shape=(n, n))
    return int(connected_components(inside, directed=False)[0]) - int(np.unique(lab).size)
