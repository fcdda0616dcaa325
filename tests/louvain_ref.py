"""Host restatement of dgll_amd.community's size-capped Louvain in numpy: the same Philox words (embedding_ref.philox4x32_10), the
same float64 expressions evaluated left to right, the same tie-breaks and the same admission, so targets and labels are bit-equal
to the device's (every weight sum is an exact integer below 2^53)."""
import numpy as np

import embedding_ref as ref


def active_mask(n, seed, level, sweep, all_active):
    if all_active:
        return np.ones(n, dtype=bool)
    ctr = np.zeros((n, 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2] = np.arange(n, dtype=np.uint32), level, sweep
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = ref.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    return (x[:, 0] & 1) == 1


def segment_sums(key, x):
    """(unique keys ascending, int64 sum of x per key)."""
    order = np.argsort(key, kind="stable")
    key, x = key[order], x[order]
    if key.size == 0:
        return key, x
    start = np.nonzero(np.concatenate(([True], key[1:] != key[:-1])))[0]
    return key[start], np.add.reduceat(x, start)


def community_state(k, size, comm, n):
    tot, csize = np.zeros(n, np.int64), np.zeros(n, np.int64)
    np.add.at(tot, comm, k)
    np.add.at(csize, comm, size)
    return tot, csize, np.bincount(comm, minlength=n).astype(np.int32)


def move_targets(rowptr, col, w, k, size, comm, tot, csize, cnt, two_m, resolution, cap, seed, level, sweep, all_active):
    """int32 [n]: what dgll_hip_louvain_move writes to `target`.  Entries with a column outside [0, n) are skipped, as there."""
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    colv = np.asarray(col, dtype=np.int64)
    wt = np.ones(colv.size, np.int64) if w is None else np.asarray(w, dtype=np.int64)
    keep = (colv != row) & (colv >= 0) & (colv < n)                       # self-loop entries count in k only
    a = np.asarray(comm, dtype=np.int64)
    pair, W = segment_sums(row[keep] * n + a[colv[keep]], wt[keep])
    pr, pc = pair // n, pair % n
    own = pc == a[pr]
    wa = np.zeros(n, np.int64)
    wa[pr[own]] = W[own]
    kf, m2, res = k.astype(np.float64), np.float64(two_m), np.float64(resolution)
    stay = wa.astype(np.float64) - res * kf * (tot[a] - k).astype(np.float64) / m2
    gain = W.astype(np.float64) - res * kf[pr] * tot[pc].astype(np.float64) / m2
    ok = ~own & (csize[pc] + size[pr] <= cap) & (gain > stay[pr]) & active_mask(n, seed, level, sweep, all_active)[pr]
    ok &= ~((cnt[a[pr]] == 1) & (cnt[pc] == 1) & (pc > a[pr]))            # two singletons: only the larger id moves
    idx = np.nonzero(ok)[0]
    idx = idx[np.lexsort((pc[idx], -gain[idx], pr[idx]))]                 # per row: largest gain, then smallest id
    first = np.concatenate(([True], pr[idx][1:] != pr[idx][:-1])) if idx.size else np.zeros(0, bool)
    target = np.asarray(comm, dtype=np.int32).copy()
    target[pr[idx[first]]] = pc[idx[first]]
    return target


def admit(comm, target, size, csize, cap):
    """(movers, their targets): movers in (target, id) order, admitted while csize[target] + the running sum of sizes <= cap."""
    movers = np.nonzero(target != comm)[0]
    t = target[movers].astype(np.int64)
    order = np.argsort(t, kind="stable")
    movers, t = movers[order], t[order]
    if movers.size == 0:
        return movers, t
    run = np.cumsum(size[movers])
    start = np.nonzero(np.concatenate(([True], t[1:] != t[:-1])))[0]
    seg = np.cumsum(np.concatenate(([True], t[1:] != t[:-1]))) - 1
    base = np.where(start > 0, run[np.maximum(start - 1, 0)], 0)
    ok = csize[t] + (run - base[seg]) <= cap
    return movers[ok], t[ok]


def aggregate(rowptr, col, w, dense, nc):
    """Coarse CSR: (community of row, community of col) coalesced with int64 weight sums; intra weight becomes self-loop entries."""
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    wt = np.ones(len(col), np.int64) if w is None else w
    key, ws = segment_sums(dense[row] * nc + dense[np.asarray(col, dtype=np.int64)], wt)
    cr = key // nc
    ptr = np.zeros(nc + 1, np.int64)
    np.cumsum(np.bincount(cr, minlength=nc), out=ptr[1:])
    return ptr, (key % nc).astype(np.int32), ws


def louvain(rowptr, col, max_comm_size=None, resolution=1.0, seed=0, max_levels=10, max_sweeps=32, on_sweep=None):
    """int64 [n] dense labels; on_sweep(level, sweep, comm, size) is called after every sweep's admission."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
    n = len(rowptr) - 1
    cap = n if max_comm_size is None else int(max_comm_size)
    labels = np.arange(n, dtype=np.int64)
    if col.size == 0:
        return labels
    w, k, size = None, np.diff(rowptr).astype(np.int64), np.ones(n, np.int64)
    two_m = int(k.sum())
    for level in range(max_levels):
        nl = len(rowptr) - 1
        comm = np.arange(nl, dtype=np.int32)
        for sweep in range(max_sweeps):
            tot, csize, cnt = community_state(k, size, comm, nl)
            target = move_targets(rowptr, col, w, k, size, comm, tot, csize, cnt, two_m, resolution, cap, seed, level, sweep,
                                  sweep == max_sweeps - 1)
            movers, t = admit(comm, target, size, csize, cap)
            comm[movers] = t
            if on_sweep is not None:
                on_sweep(level, sweep, comm, size)
            if sweep >= 2 and movers.size < max(nl // 1000, 1):
                break
        uniq, dense = np.unique(comm, return_inverse=True)
        if uniq.size == nl:
            break
        dense = dense.astype(np.int64)
        labels = dense[labels]
        rowptr, col, w = aggregate(rowptr, col, w, dense, uniq.size)
        k2, s2 = np.zeros(uniq.size, np.int64), np.zeros(uniq.size, np.int64)
        np.add.at(k2, dense, k)
        np.add.at(s2, dense, size)
        k, size = k2, s2
    return labels


def modularity(rowptr, col, labels, resolution=1.0):
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    lab = np.asarray(labels, dtype=np.int64)
    two_m = float(len(col))
    inside = float((lab[row] == lab[np.asarray(col, dtype=np.int64)]).sum())
    tot = np.bincount(lab, weights=np.diff(rowptr).astype(np.float64))
    return inside / two_m - resolution * float((tot * tot).sum()) / (two_m * two_m)
