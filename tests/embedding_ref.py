"""Host restatements of dgll_amd.embedding for the tests: a vectorised numpy Philox4x32-10, the walk and the negative draw in
numpy (every decision an integer compare, so they are bit-exact against the device), and one skip-gram step in float64 torch
written as an autograd loss plus `W -= lr * grad`."""
import numpy as np
import torch

MAX_ATTEMPTS = 1024
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: uint32 [..., 4], key: (k0, k1) -> uint32 [..., 4]."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    c0, c1, c2, c3 = (ctr[..., i].copy() for i in range(4))
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _M32, p1 >> np.uint64(32), p1 & _M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def _counters(widx, c2, c3):
    widx = np.asarray(widx, dtype=np.uint64)
    out = np.empty(widx.shape + (4,), dtype=np.uint64)
    out[..., 0] = widx & _M32
    out[..., 1] = widx >> np.uint64(32)
    out[..., 2] = c2
    out[..., 3] = c3
    return out


def thresholds(p, q):
    """T = round(2^32 w / M) for w = (1/p, 1, 1/q), M = max w: float64, as the library computes them."""
    w = np.array([1.0 / p, 1.0, 1.0 / q], dtype=np.float64)
    return np.rint(4294967296.0 * (w / w.max())).astype(np.uint64)


def walks(rowptr, col, starts, length, p=1.0, q=1.0, seed=0, first_walk_index=0, max_attempts=MAX_ATTEMPTS, return_capped=False):
    """int32 [n, length]; rows of the CSR ascend."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n_nodes = len(rowptr) - 1
    deg = np.diff(rowptr)
    edge_key = np.repeat(np.arange(n_nodes, dtype=np.int64), deg) * n_nodes + col       # ascending: rows ascend
    starts = np.asarray(starts, np.int64)
    n = len(starts)
    out = np.full((n, length), -1, dtype=np.int32)
    out[:, 0] = starts
    widx = np.uint64(first_walk_index) + np.arange(n, dtype=np.uint64)
    key = _key(seed)
    T = thresholds(p, q)
    biased = not (p == 1.0 and q == 1.0)
    v, t = starts.copy(), np.full(n, -1, dtype=np.int64)
    capped = 0
    for s in range(1, length):
        nxt = np.full(n, -1, dtype=np.int64)
        vs = np.where(v >= 0, v, 0)
        pending = np.nonzero((v >= 0) & (deg[vs] > 0))[0]
        a = 0
        while pending.size and a < max_attempts:
            x = philox4x32_10(_counters(widx[pending], s, a), key).astype(np.uint64)
            vp = v[pending]
            cand = col[rowptr[vp] + ((x[:, 0] * deg[vp].astype(np.uint64)) >> np.uint64(32)).astype(np.int64)]
            nxt[pending] = cand
            if not biased or s == 1:
                break
            tp = t[pending]
            k = tp * n_nodes + cand
            pos = np.searchsorted(edge_key, k)
            common = (pos < len(edge_key)) & (edge_key[np.minimum(pos, len(edge_key) - 1)] == k)
            thr = np.where(cand == tp, T[0], np.where(common, T[1], T[2]))
            rejected = ~(x[:, 1] < thr)
            pending = pending[rejected]
            a += 1
            if a == max_attempts:
                capped += pending.size
        t, v = v, nxt
        out[:, s] = v
    return (out, capped) if return_capped else out


def slot_offset(s, window):
    return s - window if s < window else s - window + 1


def pair_mask(walk_arr, window):
    """bool [n, L, 2W]: centre j and context j + o(s) both inside the walk and not -1."""
    n, L = walk_arr.shape
    mask = np.zeros((n, L, 2 * window), dtype=bool)
    for s in range(2 * window):
        o = slot_offset(s, window)
        j = np.arange(max(0, -o), min(L, L - o))
        if j.size:
            mask[:, j, s] = (walk_arr[:, j] >= 0) & (walk_arr[:, j + o] >= 0)
    return mask


def noise_cdf(weights):
    """The NoiseTable's fixed-point cumulative table, restated in numpy float64."""
    w = np.asarray(weights, dtype=np.float64)
    c = np.cumsum(w)
    cdf = np.rint(c / c[-1] * 4294967296.0).astype(np.uint64)
    cdf[np.nonzero(w > 0)[0].max():] = np.uint64(4294967296)
    return cdf


def negatives(walk_arr, window, k_neg, cdf, seed, first_walk_index=0):
    """int32 [n, L, 2W, K], -1 where there is no pair."""
    walk_arr = np.asarray(walk_arr)
    n, L = walk_arr.shape
    mask = pair_mask(walk_arr, window)
    widx = np.uint64(first_walk_index) + np.arange(n, dtype=np.uint64)
    pair = (np.arange(L)[:, None] * 2 * window + np.arange(2 * window)[None, :]).astype(np.uint64)          # [L, 2W]
    shape = (n, L, 2 * window, k_neg)
    ctr = _counters(np.broadcast_to(widx[:, None, None, None], shape), np.broadcast_to(pair[None, :, :, None], shape),
                    np.broadcast_to((np.arange(k_neg, dtype=np.uint64) | np.uint64(0x80000000))[None, None, None, :], shape))
    x0 = philox4x32_10(ctr, _key(seed))[..., 0].astype(np.uint64)
    draw = np.searchsorted(np.asarray(cdf, dtype=np.uint64), x0, side="right").astype(np.int32)
    return np.where(mask[..., None], draw, np.int32(-1))


def sgns_step(w_in, w_out, walk_arr, window, negs, lr):
    """One batch-synchronous step in float64: (W_in after, W_out after, loss sum).  negs: the [n, L, 2W, K] draws."""
    walk_arr = np.asarray(walk_arr)
    mask = pair_mask(walk_arr, window)
    wi, ji, si = np.nonzero(mask)
    off = np.array([slot_offset(s, window) for s in range(2 * window)])
    centre = torch.from_numpy(walk_arr[wi, ji].astype(np.int64))
    ctx = torch.from_numpy(walk_arr[wi, ji + off[si]].astype(np.int64))
    a = w_in.detach().to(torch.float64).cpu().clone().requires_grad_()
    b = w_out.detach().to(torch.float64).cpu().clone().requires_grad_()
    u = a[centre]
    loss = torch.nn.functional.softplus(-(u * b[ctx]).sum(-1)).sum()
    if negs.shape[-1]:
        ng = torch.from_numpy(np.asarray(negs)[wi, ji, si].astype(np.int64))          # [P, K]
        coef = (ng != ctx[:, None]).to(torch.float64)                                 # a negative equal to the context: coefficient 0
        loss = loss + (coef * torch.nn.functional.softplus((u[:, None, :] * b[ng]).sum(-1))).sum()
    ga, gb = torch.autograd.grad(loss, (a, b), allow_unused=True)
    ga = torch.zeros_like(a) if ga is None else ga
    gb = torch.zeros_like(b) if gb is None else gb
    return (a - lr * ga).detach(), (b - lr * gb).detach(), float(loss.detach())


def planted_partition(n_per=40, p_in=0.3, p_out=0.01, seed=1):
    """Undirected 2-community graph as a symmetric CSR (rowptr int64, col int32 ascending) and the community of every node."""
    rng = np.random.default_rng(seed)
    n = 2 * n_per
    comm = np.repeat(np.arange(2), n_per)
    prob = np.where(comm[:, None] == comm[None, :], p_in, p_out)
    upper = np.triu(rng.random((n, n)) < prob, 1)
    adj = upper | upper.T
    row, col = np.nonzero(adj)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=n), out=rowptr[1:])
    return rowptr, col.astype(np.int32), comm


def cosine_split(emb, comm):
    """(mean intra-community, mean inter-community) cosine similarity over distinct pairs."""
    e = np.asarray(emb, dtype=np.float64)
    e = e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-30)
    sim = e @ e.T
    same = comm[:, None] == comm[None, :]
    offdiag = ~np.eye(len(comm), dtype=bool)
    return float(sim[same & offdiag].mean()), float(sim[~same].mean())


# lr: the step sums its pairs' gradients (no mean), and a batch of 20 walks of 20 nodes with 6 contexts and 5 negatives each touches
# every one of the 80 nodes some hundreds of times -- 0.005 is about the reference's 0.25 divided by that count; at 0.02 the
# float64 restatement diverges
TRAIN = dict(dim=16, length=20, window=3, negatives=5, walks_per_vertex=2, lr=0.005, batch_walks=20, epochs=6, seed=7)


def train_host(rowptr, col, cfg=TRAIN, p=1.0, q=1.0):
    """The whole trainer in float64 on the host, from the restated pieces: (embeddings, loss sum per epoch)."""
    n = len(rowptr) - 1
    gen = torch.Generator().manual_seed(cfg["seed"])
    w_in = torch.rand((n, cfg["dim"]), generator=gen, dtype=torch.float64)
    w_out = torch.rand((n, cfg["dim"]), generator=gen, dtype=torch.float64)
    cdf = noise_cdf(np.bincount(col, minlength=n).astype(np.float64) ** 0.75)
    rng = np.random.default_rng(cfg["seed"])
    drawn, losses = 0, []
    for _ in range(cfg["epochs"]):
        total = 0.0
        for _ in range(cfg["walks_per_vertex"]):
            order = rng.permutation(n)
            for b0 in range(0, n, cfg["batch_walks"]):
                starts = order[b0:b0 + cfg["batch_walks"]]
                wk = walks(rowptr, col, starts, cfg["length"], p, q, cfg["seed"], drawn)
                ng = negatives(wk, cfg["window"], cfg["negatives"], cdf, cfg["seed"], drawn)
                w_in, w_out, loss = sgns_step(w_in, w_out, wk, cfg["window"], ng, cfg["lr"])
                drawn += len(starts)
                total += loss
        losses.append(total)
    return w_in.numpy(), losses
