"""struc2vec's context graph and its walk on the device: ordered degree sequences by multi-source BFS (one SpMM per level), the
pairs to compare, exact DTW distances (dgll_amd/csrc/struc_dtw.hip), the multilayer graph with its alias table and up-move
thresholds, and the walk over it (struc_walk_kernel in dgll_amd/csrc/walk.hip)."""
import math
import time

import numpy as np
import torch

from .. import _lib
from ..graph import CSRGraph
from .walks import MAX_ATTEMPTS, AliasTable, as_walk_graph

_BFS_BATCH = 128             # roots per multi-source BFS: the indicator matrix is [N, 128] fp32


class DegreeSequences:
    """Ragged ordered degree sequences: the sequence of node v at BFS level l is entries [seq_ptr[v * n_levels + l],
    seq_ptr[v * n_levels + l + 1]) of seq_deg / seq_cnt (int32, degrees ascending); a level the node never reaches is empty."""

    def __init__(self, seq_ptr, seq_deg, seq_cnt, n_nodes, n_levels):
        self.seq_ptr, self.seq_deg, self.seq_cnt = seq_ptr, seq_deg, seq_cnt
        self.n_nodes, self.n_levels = int(n_nodes), int(n_levels)

    def lengths(self):
        return (self.seq_ptr[1:] - self.seq_ptr[:-1]).view(self.n_nodes, self.n_levels)

    def tolist(self):
        """[v][l] -> list of (degree, count), levels the node reaches only (host copy, for tests)."""
        ptr, deg, cnt = self.seq_ptr.cpu().tolist(), self.seq_deg.cpu().tolist(), self.seq_cnt.cpu().tolist()
        out = []
        for v in range(self.n_nodes):
            levels = []
            for l in range(self.n_levels):
                b, e = ptr[v * self.n_levels + l], ptr[v * self.n_levels + l + 1]
                if e == b:
                    break
                levels.append(list(zip(deg[b:e], cnt[b:e])))
            out.append(levels)
        return out


def degree_sequences(g, reduce_len=True, num_layers=None, batch=_BFS_BATCH):
    """struc2vec.py:193-238 for every root at once: levels 0..num_layers (None: until the component is exhausted) of the BFS from
    every node, each reduced to its ascending (degree, count) pairs (reduce_len=False: ascending degrees, count 1).  Level-
    synchronous BFS over `batch` roots at a time: one SpMM per level over the [N, batch] frontier indicator."""
    from .. import ops

    g = as_walk_graph(g)
    if not g.is_cuda:
        raise RuntimeError("dgll_amd.embedding runs on the GPU only (got a %s graph); there is no CPU fallback" % g.device)
    n, dev = g.n_rows, g.device
    if num_layers is not None and int(num_layers) < 0:
        raise ValueError("opt3_num_layers must be >= 0 or None")
    deg = g.degrees()
    span = int(deg.max()) + 1 if n else 1
    gt = g.transpose()[0]                                   # the frontier's out-neighbours: row u of A^T gathers the v with u in row v
    gt = CSRGraph(gt.rowptr, gt.col, None, n, n, check=False)
    parts, n_levels = [], 1
    for r0 in range(0, n, batch):
        b = min(batch, n - r0)
        lane = torch.arange(b, device=dev)
        frontier = torch.zeros((n, b), dtype=torch.float32, device=dev)
        frontier[r0 + lane, lane] = 1.0
        visited = frontier > 0
        nodes, roots, levels = [], [], []
        level = 0
        while True:
            node, root = (frontier > 0).nonzero(as_tuple=True)
            nodes.append(node)
            roots.append(root)
            levels.append(torch.full_like(root, level))
            if num_layers is not None and level >= int(num_layers):
                break
            reached = ops.spmm_raw(gt, frontier)[:, :b] > 0
            new = reached & ~visited
            if not bool(new.any()):
                break
            visited |= new
            frontier = new.to(torch.float32)
            level += 1
        n_batch_levels = level + 1
        n_levels = max(n_levels, n_batch_levels)
        node, root, lev = torch.cat(nodes), torch.cat(roots), torch.cat(levels)
        key = ((root * n_batch_levels + lev) * span + deg[node])
        if reduce_len:
            key, cnt = torch.unique(key, return_counts=True)         # sorted: (root, level, degree) ascending
        else:
            key = torch.sort(key).values
            cnt = torch.ones_like(key)
        d = key % span
        rl = torch.div(key, span, rounding_mode="floor")
        parts.append((r0 + torch.div(rl, n_batch_levels, rounding_mode="floor"), rl % n_batch_levels, d, cnt))
    root = torch.cat([p[0] for p in parts])
    lev = torch.cat([p[1] for p in parts])
    seq_ptr = torch.zeros(n * n_levels + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(root * n_levels + lev, minlength=n * n_levels), 0, out=seq_ptr[1:])
    seq_deg = torch.cat([p[2] for p in parts]).to(torch.int32)
    seq_cnt = torch.cat([p[3] for p in parts]).to(torch.int32)
    return DegreeSequences(seq_ptr, seq_deg, seq_cnt, n, n_levels)


def select_pairs(degrees, reduce_sim_calc=True):
    """int32 [P, 2] host array, in the reference's order.  reduce_sim_calc: every vertex v with the vertices of its own degree and
    then of the nearest degrees (ties go to the larger one), ascending vertex id inside a degree, until more than 2 log2 N are
    taken (utils.py:123-189); a pair may appear in both orders.  Otherwise all pairs v < u."""
    deg = np.asarray(degrees, dtype=np.int64)
    n = len(deg)
    if not reduce_sim_calc:
        a, b = np.triu_indices(n, 1)
        return np.stack([a, b], axis=1).astype(np.int32)
    order = np.argsort(deg, kind="stable")
    uniq, start = np.unique(deg[order], return_index=True)
    end = np.append(start[1:], n)
    group = np.searchsorted(uniq, deg)
    cap = int(math.floor(2 * math.log(n, 2))) + 1            # the loop stops once the count EXCEEDS 2 log2 N
    n_groups = len(uniq)
    out_v, out_u = [], []
    for v in range(n):
        g0 = int(group[v])
        room = cap
        below = g0 - 1
        above = g0 + 1 if g0 + 1 < n_groups else -1
        now = g0
        while True:
            members = order[start[now]:end[now]]
            if now == g0:
                members = members[members != v]
            members = members[:room]
            out_u.append(members)
            out_v.append(np.full(len(members), v, dtype=np.int64))
            room -= len(members)
            if room == 0:
                break
            if now != g0:
                if now == below:
                    below -= 1
                else:
                    above = above + 1 if above + 1 < n_groups else -1
            if below == -1 and above == -1:
                break
            if below == -1:
                now = above
            elif above == -1:
                now = below
            elif abs(uniq[below] - deg[v]) < abs(uniq[above] - deg[v]):
                now = below
            else:
                now = above
    if not out_v:
        return np.zeros((0, 2), dtype=np.int32)
    return np.stack([np.concatenate(out_v), np.concatenate(out_u)], axis=1).astype(np.int32)


def struc_dtw(seqs, pairs, stream=None):
    """float64 [P, n_levels] device tensor: the exact DTW distance of every pair's sequences at every level, -1 from the first level
    either node lacks (dgll_hip_struc_dtw).  Raises ValueError when the shorter sequence of some task is longer than the kernel's
    LDS strip buffer holds (dgll_hip_struc_dtw_max_rows(), 1024 entries); one blocking read."""
    dev = seqs.seq_ptr.device
    pairs = pairs.to(device=dev, dtype=torch.int32).contiguous()
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs must be [P, 2]")
    n_pairs, n_levels = pairs.shape[0], seqs.n_levels
    dist = torch.empty((n_pairs, n_levels), dtype=torch.float64, device=dev)
    if n_pairs == 0:
        return dist
    lens = seqs.lengths()
    pl = pairs.to(torch.int64)
    lo, hi = int(pl.min()), int(pl.max())
    if lo < 0 or hi >= seqs.n_nodes:
        raise ValueError("pairs hold a node id outside [0, N)")
    longest = int(torch.minimum(lens[pl[:, 0]], lens[pl[:, 1]]).max())
    limit = _lib.lib.dgll_hip_struc_dtw_max_rows()
    if longest > limit:
        raise ValueError("struc2vec DTW: a pair's shorter degree sequence has %d entries, the kernel holds %d "
                         "(use opt1_reduce_len=True)" % (longest, limit))
    _lib.launch("dgll_hip_struc_dtw", dev, seqs.seq_ptr.data_ptr(), seqs.seq_deg.data_ptr(), seqs.seq_cnt.data_ptr(), seqs.n_nodes,
                n_levels, pairs.data_ptr(), n_pairs, dist.data_ptr(), stream=stream)
    return dist


def up_thresholds(gamma):
    """uint32 host array round(2^32 x / (x + 1)), x = log(gamma + e): the probability of moving up a layer (biasedRandomWalk.py:49)
    as an integer threshold; always below 2^32.  numpy float64 on the host, so a host restatement gives the same bits."""
    x = np.log(np.asarray(gamma, dtype=np.float64) + math.e)
    return np.rint(4294967296.0 * (x / (x + 1.0))).astype(np.uint64).astype(np.uint32)


class StrucContext:
    """The multilayer context graph of struc2vec.  graph: stacked CSRGraph of n_layers * n_nodes rows (row l * n_nodes + v = v's
    neighbours in layer l, plain node ids, duplicates kept; val = fp32 exp(-(d - the row's smallest d))), alias: its AliasTable,
    t_up: int32 [n_layers * n_nodes] holding the uint32 up-move thresholds, gamma: int64 of the same shape; kept for inspection:
    seqs, pairs [P, 2], dist [P, n_layers] cumulative distances (-1: the layer is invalid for the pair), norm_weights (fp64, per
    stacked edge), layer_average (fp64 [n_layers]) and timings (seconds: bfs, pairs, dtw, graph, alias)."""

    def __init__(self, graph, alias, t_up, gamma, n_nodes, n_layers, seqs, pairs, dist, norm_weights, layer_average, timings):
        self.graph, self.alias, self.t_up, self.gamma = graph, alias, t_up, gamma
        self.n_nodes, self.n_layers = int(n_nodes), int(n_layers)
        self.seqs, self.pairs, self.dist = seqs, pairs, dist
        self.norm_weights, self.layer_average, self.timings = norm_weights, layer_average, timings

    @classmethod
    def from_graph(cls, g, opt1_reduce_len=True, opt2_reduce_sim_calc=True, opt3_num_layers=None):
        g = as_walk_graph(g)
        if not g.is_cuda:
            raise RuntimeError("dgll_amd.embedding runs on the GPU only (got a %s graph); there is no CPU fallback" % g.device)
        dev, n = g.device, g.n_rows
        timings = {}

        def lap(name, t0):
            torch.cuda.synchronize(dev)
            timings[name] = time.perf_counter() - t0
            return time.perf_counter()

        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        seqs = degree_sequences(g, opt1_reduce_len, opt3_num_layers)
        t0 = lap("bfs", t0)
        pairs = torch.from_numpy(select_pairs(g.degrees().cpu().numpy(), opt2_reduce_sim_calc)).to(dev)
        t0 = lap("pairs", t0)
        raw = struc_dtw(seqs, pairs)
        t0 = lap("dtw", t0)
        n_layers = seqs.n_levels
        # convert_dtw_struc_dist: the distance of layer l is the sum over the layers up to l
        valid = raw >= 0
        dist = torch.where(valid, torch.cumsum(torch.where(valid, raw, torch.zeros_like(raw)), dim=1), raw)
        pi, li = valid.nonzero(as_tuple=True)
        a, b = pairs[pi, 0].to(torch.int64), pairs[pi, 1].to(torch.int64)
        d = dist[pi, li]
        rows, order = torch.sort(torch.cat([li * n + a, li * n + b]), stable=True)
        col = torch.cat([b, a])[order]
        d = torch.cat([d, d])[order]
        n_rows = n_layers * n
        rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(rows, minlength=n_rows), 0, out=rowptr[1:])
        # difference (i): exp(-(d - min of the row)); the normalised weights are the reference's, and no row underflows to all zeros
        d_min = torch.full((n_rows,), float("inf"), dtype=torch.float64, device=dev).scatter_reduce_(0, rows, d, "amin")
        w = torch.exp(-(d - d_min[rows]))
        norm = w / torch.zeros(n_rows, dtype=torch.float64, device=dev).index_add_(0, rows, w)[rows]
        layer = torch.div(rows, n, rounding_mode="floor")
        average = torch.zeros(n_layers, dtype=torch.float64, device=dev).index_add_(0, layer, norm) / \
            torch.bincount(layer, minlength=n_layers).clamp(min=1)
        gamma = torch.zeros(n_rows, dtype=torch.int64, device=dev).index_add_(0, rows, (norm > average[layer]).to(torch.int64))
        t_up = torch.from_numpy(up_thresholds(gamma.cpu().numpy()).view(np.int32)).to(dev)
        stacked = CSRGraph(rowptr, col.to(torch.int32), w.to(torch.float32), n_rows, n_rows, check=False)
        t0 = lap("graph", t0)
        alias = AliasTable.from_graph(stacked)
        lap("alias", t0)
        return cls(stacked, alias, t_up, gamma, n, n_layers, seqs, pairs, dist, norm, average, timings)


def struc_walks(ctx, starts, length, stay_prob, seed, first_walk_index, info=None, return_layers=False, max_attempts=MAX_ATTEMPTS,
                stream=None):
    """int32 [n, length] walks over the context graph from `starts` (int64 device tensor) at layer 0: every attempt of a step stays
    in the layer with probability stay_prob (and then emits a neighbour drawn by the layer's weights) or moves a layer up or down;
    a node without neighbours in its layer ends the walk (-1 from there on).  Walk i is a function of (seed, first_walk_index + i)
    only.  info as for random_walks (info[0]: attempts that reached the cap, where the step stays regardless).
    return_layers: also the int32 [n, length] layer every entry was emitted from."""
    if not isinstance(starts, torch.Tensor) or not starts.is_cuda:
        raise RuntimeError("dgll_amd.embedding runs on the GPU only (starts must be a device tensor); there is no CPU fallback")
    if not isinstance(ctx, StrucContext) or ctx.graph.device != starts.device:
        raise ValueError("ctx must be a StrucContext on the device of starts")
    stay_prob, length, max_attempts = float(stay_prob), int(length), int(max_attempts)
    if not 0.0 <= stay_prob <= 1.0:
        raise ValueError("stay_prob must lie in [0, 1]")
    if length < 1:
        raise ValueError("walk length must be >= 1")
    if max_attempts < 1:
        raise ValueError("max_attempts must be >= 1")
    starts = starts.to(torch.int64).reshape(-1).contiguous()
    n = starts.numel()
    walks = torch.empty((n, length), dtype=torch.int32, device=starts.device)
    layers = torch.empty((n, length), dtype=torch.int32, device=starts.device) if return_layers else None
    if info is None:
        info = torch.zeros(2, dtype=torch.int64, device=starts.device)
    g = ctx.graph
    _lib.launch("dgll_hip_struc_walk", starts.device, g.rowptr.data_ptr(), g.col.data_ptr(), ctx.alias.table.data_ptr(),
                ctx.t_up.data_ptr(), ctx.n_nodes, ctx.n_layers, starts.data_ptr(), n, length, int(first_walk_index) & 0xFFFFFFFFFFFFFFFF,
                int(seed) & 0xFFFFFFFFFFFFFFFF, stay_prob, max_attempts, walks.data_ptr(), _lib.ptr(layers), info.data_ptr(),
                stream=stream)
    return (walks, layers) if return_layers else walks
