"""float64 references of the kNN search (csrc/knn.hip) and of EdgeConv, deliberately the slow obvious forms.

    knn(x, sizes, k, exclude_self)   brute force per segment: the squared distances in the DIFFERENCE form sum_c (x_i - x_j)^2, then a
                                     stable sort by (d, j) -> (rowptr int64 [n + 1], col int64 [nnz], dist float64 [nnz])
    all_distances(x, sizes)          per row, the float64 distances to every point of its segment (for the order-statistic checks)
    edgeconv(...)                    h_i = max_j theta(h_j - h_i) + phi(h_i) with the [nnz, out] messages materialised and a scatter max
"""
import numpy as np
import torch


def segment_bounds(sizes):
    ptr = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(np.asarray(sizes, dtype=np.int64), out=ptr[1:])
    return ptr


def out_rowptr(sizes, k, exclude_self=False):
    """the row pointers the search writes at: deg_i = min(k, size - (exclude_self ? 1 : 0))"""
    deg = np.concatenate([np.full(s, min(k, max(s - int(exclude_self), 0)), dtype=np.int64) for s in sizes] + [np.zeros(0, dtype=np.int64)])
    ptr = np.zeros(deg.size + 1, dtype=np.int64)
    np.cumsum(deg, out=ptr[1:])
    return ptr


def lattice_case(k, D, cand_tile, query_tile, seed=0):
    """(sizes, x float64 [n, D], (b, e) of a segment of identical points): integer coordinates in [-16, 16], so that every squared
    distance is an integer below 2^24 -- exact in fp32 whatever the summation order or contraction, with bf16 inputs too -- and ties
    are everywhere.  Segment sizes: 0, 1, 2, k, k + 1, 63, 64, 65, the candidate tile's edges, an empty one in the middle, one that
    spans more than one query tile and starts inside one, and k + 5 copies of one point."""
    sizes = [0, 1, 2, k, k + 1, 63, 64, 65, cand_tile - 1, cand_tile, cand_tile + 1, 2 * cand_tile + 3, 0, query_tile + 41, k + 5]
    rng = np.random.RandomState(1000 * k + D + seed)
    n = sum(sizes)
    span = 16 if D > 1 else 6                           # one dimension: few distinct values, many ties
    x = rng.randint(-span, span + 1, size=(n, D)).astype(np.float64)
    e = n
    b = e - sizes[-1]
    x[b:e] = x[b]
    return sizes, x, (b, e)


def knn(x, sizes, k, exclude_self=False):
    x = np.asarray(x, dtype=np.float64)
    ptr = segment_bounds(sizes)
    assert ptr[-1] == x.shape[0]
    rowptr, col, dist = [0], [], []
    for s in range(len(sizes)):
        b, e = int(ptr[s]), int(ptr[s + 1])
        for i in range(b, e):
            diff = x[b:e] - x[i]
            d = (diff * diff).sum(axis=1)
            j = np.arange(b, e)
            if exclude_self:
                keep = j != i
                d, j = d[keep], j[keep]
            order = np.argsort(d, kind="stable")[:k]        # j ascends, so a stable sort by d is the sort by (d, j)
            col.append(j[order])
            dist.append(d[order])
            rowptr.append(rowptr[-1] + len(order))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)      # noqa: E731
    return np.asarray(rowptr, dtype=np.int64), cat(col, np.int64), cat(dist, np.float64)


def all_distances(x, sizes):
    """list over rows of (first row id of the segment, float64 distances to every row of the segment)"""
    x = np.asarray(x, dtype=np.float64)
    ptr = segment_bounds(sizes)
    out = []
    for s in range(len(sizes)):
        b, e = int(ptr[s]), int(ptr[s + 1])
        for i in range(b, e):
            diff = x[b:e] - x[i]
            out.append((b, (diff * diff).sum(axis=1)))
    return out


def _stored(t, dtype):
    """t rounded to `dtype` as a value, the identity as a function (straight through): where the GPU path stores a matrix"""
    return t + (t.detach().to(dtype).double() - t.detach())


def edgeconv(rowptr, col, h_src, h_dst, w_theta, b_theta, w_phi, b_phi, store_dtype=None):
    """float64 torch, differentiable: out [n_dst, out] of DGL's EdgeConv on the CSR graph (row i lists its sources),
    h_i = max_j theta(h_j - h_i) + phi(h_i).  The message of every edge is materialised ([nnz, out]) and reduced with a scatter max;
    a row without entries gets phi(h_i) + b_theta (the max over nothing counted as 0).

    store_dtype=None: DGL's own order, theta applied to the difference h_j - h_i of every edge.
    store_dtype=torch.bfloat16: rounded where the layer stores in bf16, so that the two agree on WHICH source wins a near-tie (the
    gradient goes to that source alone): the stacked weights W_theta and W_phi - W_theta, the products h W_theta^T and
    h (W_phi - W_theta)^T, and the sum of the max and the second product.  The per-edge message is then the stored row of the
    source; its own -h_i W_theta^T is constant over a row's edges and sits in the second product."""
    n_dst = rowptr.numel() - 1
    deg = rowptr[1:] - rowptr[:-1]
    row = torch.repeat_interleave(torch.arange(n_dst), deg)
    fo = w_theta.shape[0]

    def scatter_max(msg):
        agg = torch.zeros(n_dst, fo, dtype=torch.float64)
        if msg.shape[0]:
            full = torch.full_like(agg, -float("inf")).scatter_reduce(0, row[:, None].expand_as(msg), msg, "amax", include_self=True)
            agg = torch.where((deg > 0)[:, None], full, agg)
        return agg

    if store_dtype is None:
        msg = (h_src[col.long()] - h_dst[row]) @ w_theta.t()                # [nnz, out]
        return scatter_max(msg) + b_theta + h_dst @ w_phi.t() + b_phi
    w_src, w_dst = _stored(w_theta, store_dtype), _stored(w_phi - w_theta, store_dtype)
    z_src, z_dst = _stored(h_src @ w_src.t(), store_dtype), _stored(h_dst @ w_dst.t(), store_dtype)
    # stored values tie: the gradient goes to the tied source of the smallest id, as ops.segment_max sends it (amax would split it)
    msg = z_src[col.long()]                                                 # [nnz, out]
    top = scatter_max(msg.detach())
    ids = torch.where(msg.detach() == top[row], col.long()[:, None].expand_as(msg), h_src.shape[0])
    win = torch.full((n_dst, fo), h_src.shape[0], dtype=torch.int64).scatter_reduce(0, row[:, None].expand_as(ids), ids, "amin")
    agg = torch.where((deg > 0)[:, None], z_src.gather(0, win.clamp(max=h_src.shape[0] - 1)), torch.zeros((), dtype=torch.float64))
    assert torch.equal(agg.detach(), top)
    out = _stored(agg + z_dst, store_dtype)
    own = _stored(h_dst @ w_src.t(), store_dtype) * (deg == 0)[:, None]     # a row without entries: phi(h_i) + b_theta
    return out + own + b_theta + b_phi
