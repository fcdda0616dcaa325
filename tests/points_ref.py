"""float64 references of farthest point sampling (csrc/fps.hip), the fixed-radius search (csrc/radius.hip) and PointNetConv, the slow
obvious forms, and the integer-lattice cases the emulated and the GPU tests share."""
import numpy as np
import torch

from knn_ref import _stored, edgeconv, lattice_case as knn_case, segment_bounds


def lattice_case(sizes, D, seed=0, same=()):
    """x float64 [sum(sizes), D], integers in [-16, 16]; the segments whose number is in `same` hold copies of one point"""
    rng = np.random.RandomState(77 * D + seed)
    span = 16 if D > 1 else 6                           # one dimension: few distinct values, many ties
    x = rng.randint(-span, span + 1, size=(sum(sizes), D)).astype(np.float64)
    ptr = segment_bounds(sizes)
    for s in same:
        x[ptr[s]:ptr[s + 1]] = x[ptr[s]:ptr[s] + 1]
    return x


def fps_case(D, pts):
    """(sizes, counts, starts, x) for the fps instance with `pts` dmin per lane in registers (0: the scratch array): the instance's
    size edges (256 pts + 1 is the next one's), 37 identical points, one m == size; starts 0, last (-1) and out of range"""
    tier = {4: [1023, 1024], 16: [1025, 4095, 4096], 32: [4097, 8191, 8192], 0: [8193]}[pts]
    sizes = [0, 1, 2, 63, 64, 65, 255, 256, 257, 0] + tier + [37, 65]
    counts = [0, 1, 2, 9, 2, 0, 9, 1, 9, 0] + [9] * len(tier) + [37, 65]
    starts = [0, 0, 1, -1, 64 + 3, 0, 254, 0, 256, 5] + [s - 1 for s in tier] + [3, 1000]
    return sizes, counts, starts, lattice_case(sizes, D, same=(len(sizes) - 2,))


def radius_case(K, D, bipartite):
    """(x_sizes, x, y_sizes, y, (b, e) of the identical candidates): knn_ref.lattice_case's candidates; bipartite queries in other
    segment sizes, one side empty (both ways), 300 that span two tiles, the last nine AT the identical candidates"""
    x_sizes, x, same = knn_case(K, D, 32, 256)
    if not bipartite:
        return x_sizes, x, x_sizes, x, same
    y_sizes = [3, 0, 5, 1, 40, 0, 64, 2, 33, 7, 1, 70, 4, 300, 9]
    y = lattice_case(y_sizes, D, seed=5)
    y[-9:] = x[same[0]]
    return x_sizes, x, y_sizes, y, same


def fps(x, sizes, counts, starts):
    x = np.asarray(x, dtype=np.float64)
    ptr = segment_bounds(sizes)
    idx, dmin = [], []
    for s, (size, m) in enumerate(zip(sizes, counts)):
        if not m:
            continue
        seg = x[ptr[s]:ptr[s + 1]]
        cur, d, left = starts[s] % size, np.full(size, np.inf), np.ones(size, dtype=bool)
        idx.append(ptr[s] + cur)
        dmin.append(np.inf)
        for _ in range(m - 1):
            left[cur] = False
            d = np.minimum(d, ((seg - seg[cur]) ** 2).sum(axis=1))
            cur = int(np.argmax(np.where(left, d, -np.inf)))     # argmax: the first of the largest
            idx.append(ptr[s] + cur)
            dmin.append(d[cur])
    return np.asarray(idx, dtype=np.int64), np.asarray(dmin, dtype=np.float64)


def radius(y, y_sizes, x, x_sizes, r2, K, exclude_self=False):
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    yp, xp = segment_bounds(y_sizes), segment_bounds(x_sizes)
    rowptr, col, dist = [0], [], []
    for s in range(len(y_sizes)):
        for i in range(yp[s], yp[s + 1]):
            d = ((x[xp[s]:xp[s + 1]] - y[i]) ** 2).sum(axis=1)
            j = np.arange(xp[s], xp[s + 1])
            keep = (d <= r2) & ~(exclude_self & (j == i))
            col.append(j[keep][:K])
            dist.append(d[keep][:K])
            rowptr.append(rowptr[-1] + len(col[-1]))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)      # noqa: E731
    return np.asarray(rowptr, dtype=np.int64), cat(col, np.int64), cat(dist, np.float64)


def pointnetconv(rowptr, col, x_src, pos_src, pos_dst, weight, bias, relu, store_dtype=None):
    """float64 torch, differentiable: out_i = max_j local(cat(x_j, pos_j - pos_i)), local = Linear (+ ReLU; monotone, so applied to the
    max), one message per edge.  That message is EdgeConv's theta(h_j - h_i) with h = cat(x, pos), the destinations' x set to 0 and
    phi = 0, so knn_ref.edgeconv materialises it, store_dtype (where the layer stores in bf16) included; the bias is rounded first
    there, as the layer rounds it, so that the ReLU gates on the sign the layer sees."""
    C = 0 if x_src is None else x_src.shape[1]
    h_src = pos_src if x_src is None else torch.cat([x_src, pos_src], dim=1)
    h_dst = torch.cat([pos_dst.new_zeros(pos_dst.shape[0], C), pos_dst], dim=1)
    b = bias if store_dtype is None else _stored(bias, store_dtype)
    out = edgeconv(rowptr, col, h_src, h_dst, weight, b, torch.zeros_like(weight), torch.zeros_like(bias), store_dtype=store_dtype)
    return torch.relu(out) if relu else out
