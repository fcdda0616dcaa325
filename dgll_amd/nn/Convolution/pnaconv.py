"""Principal Neighbourhood Aggregation layer (DGL's PNAConv, "Principal Neighbourhood Aggregation for Graph Nets": argument names,
parameter names and shapes) on the gfx950 aggregation engine.

    PNAConv(in_size, out_size, aggregators, scalers, delta, dropout=0.0, num_towers=1, edge_feat_size=0, residual=True)
    forward(graph, node_feat, edge_feat=None, snorm_n=None)     node_feat: [n_src, in_size], or (feat_src, feat_dst) for blocks
    PNA(nfeat, nhid, nclass, n_layers=2, ...)                   a linear embedding, PNAConv layers, a linear classifier

`graph` is a CSRGraph [n_dst x n_src] or anything as_csr_graph takes (rectangular blocks of NeighborSampler allowed; edge values are
ignored).  Tower t works on the columns [t Fi, (t + 1) Fi) of the input, Fi = in_size / num_towers, Fo = out_size / num_towers:

    msg_ij  = M(cat(h_j, h_i))                                   M = Linear(2 Fi, Fi)
    h_neigh = cat over scalers s, aggregators a of  scaler_s(D_i) * agg_a over j of msg_ij           (a row without entries: 0)
    h       = dropout(batchnorm(U(cat(h_i, h_neigh)) * snorm_n))  U = Linear((n_agg n_scaler + 1) Fi, Fo), BatchNorm1d(Fo)

and the layer concatenates the towers, applies mixing_layer = Sequential(Linear(out_size, out_size), LeakyReLU()) and adds h_i when
`residual` (which needs in_size == out_size).  aggregators: "mean", "sum", "max", "min", "var", "std" (DGL's "moment3" .. "moment5"
raise NotImplementedError); scalers: "identity", "amplification" log(D + 1) / delta, "attenuation" delta / log(D + 1); delta is
usually dgll_amd.ops_agg.pna_delta(training graph).  snorm_n [n_dst, 1] is DGL's graph-size normalisation; its default is None
because a CSRGraph has no batch.

The message is linear, so it splits into a source and a destination term,

    msg_ij = P[j] + Q[i],     P = h_src . Ms^T,   Q = h_dst . Md^T + b          (Ms = M.weight[:, :Fi], Md = M.weight[:, Fi:])

and on the GPU no [nnz, Fi] tensor exists: two dense transforms (dense.linear) and ONE autograd node over the fused gather passes of
ops_agg.multi_aggregate (one gather of P per edge feeds every aggregator).  That is also why per-edge features are not built:
edge_feat_size != 0 or an edge_feat argument raises NotImplementedError (a per-edge term does not split).  A tower width that is not a
whole number of 16-byte vectors is padded with zero rows in M's halves (zero columns of P and Q) and unpadded after the aggregation.
bf16 features are accepted and returned, but on the GPU the layer's interior runs in fp32 and the result is rounded once (PNAConv.forward
says why, with figures); the bf16 kernels serve ops_agg.multi_aggregate called directly.
max / min send their gradient to the smallest source id among the entries attaining the extreme (torch: an unspecified one), so the
gradients differ from a torch restatement on ties only.  Host tensors take `_host_aggregate`, the same semantics with torch's segment
ops on explicit per-edge messages, so that the layer's own logic can be exercised without a GPU; a GPU tensor never reaches it.
"""
from ... import backend as F
from ... import dense, ops, ops_agg
from ...graph import as_csr_graph
from .dotgatconv import _split_feat

_STD_EPS = 1e-30


def _host_extreme(msg, row, col, n, largest):
    """[n, Fi]: the largest / smallest message per row and column, gathered from the entry the tie rule selects (smallest source id,
    then the first such entry); 0 for a row without entries."""
    nnz, width = msg.shape
    seg = row.unsqueeze(1).expand(nnz, width)
    m = msg.detach()
    ext = F.full((n, width), -float("inf") if largest else float("inf"), dtype=msg.dtype).scatter_reduce(0, seg, m, "amax" if largest else "amin")
    hit = m == ext[row]
    big = int(col.max()) + 1
    src = col.unsqueeze(1).expand(nnz, width)
    arg = F.full((n, width), big, dtype=F.int64).scatter_reduce(0, seg, F.where(hit, src, big), "amin")
    at = F.arange(nnz).unsqueeze(1).expand(nnz, width)
    first = F.full((n, width), nnz, dtype=F.int64).scatter_reduce(0, seg, F.where(hit & (src == arg[row]), at, nnz), "amin")
    value = msg.gather(0, first.clamp(max=nnz - 1))
    return F.where(first == nnz, F.zeros_like(value), value)


def _host_aggregate(graph, h_src, h_dst, fc_m, aggregators, scalers, delta):
    """[n_dst, n_scaler * n_agg * Fi] with per-edge messages fc_m(cat(h_src[col], h_dst[row])) (host tensors only)."""
    row, col, n = graph.row_index(), graph.col.long(), graph.n_rows
    msg = fc_m(F.cat([h_src[col], h_dst[row]], 1))                              # [nnz, Fi]
    width = msg.shape[1]
    if graph.nnz == 0:
        return msg.new_zeros((n, len(aggregators) * len(scalers) * width)) + 0 * msg.sum()
    deg = graph.degrees()
    has = (deg > 0).unsqueeze(1)
    cnt = deg.clamp(min=1).to(msg.dtype).unsqueeze(1)
    seg_sum = lambda t: F.zeros(n, width, dtype=msg.dtype).index_add_(0, row, t)     # noqa: E731
    first = msg[graph.rowptr[:-1].clamp(max=graph.nnz - 1)] * has               # the mean about the row's first message: a row of
    mean = first + seg_sum(msg - first[row]) / cnt                              # equal messages has exactly that mean and var 0
    var = F.relu(seg_sum((msg - mean[row]) ** 2) / cnt)
    value = {}
    for a in aggregators:
        if a == "mean":
            value[a] = mean
        elif a == "sum":
            value[a] = seg_sum(msg)
        elif a in ("max", "min"):
            value[a] = _host_extreme(msg, row, col, n, a == "max")
        elif a == "var":
            value[a] = var
        else:
            value[a] = F.sqrt(var + _STD_EPS)
    logd = F.log(cnt + 1.0)
    scale = {"identity": F.ones_like(logd), "amplification": logd / delta, "attenuation": delta / logd}
    return F.cat([F.where(has, scale[s] * value[a], F.zeros_like(mean)) for s in scalers for a in aggregators], 1)


def _linear(h, weight, bias=None):
    """h . weight^T + bias: on the GPU through the dense transform path (bf16 activations with fp32 parameters included)."""
    if not h.is_cuda:
        out = h @ weight.t().to(h.dtype)
        return out if bias is None else out + bias.to(h.dtype)
    out = dense.linear(h.contiguous(), weight.contiguous().t())
    return out if bias is None else out + bias.to(out.dtype)


def _pad_rows(t, pad):
    """t with `pad` zero rows appended (a weight [Fi, *] or a bias [Fi])"""
    return t if not pad else F.cat([t, t.new_zeros((pad,) + tuple(t.shape[1:]))], 0)


class PNAConvTower(F.nn.Module):
    """One tower: M, U, batchnorm, dropout (DGL's PNAConvTower: the same parameter names)."""

    def __init__(self, in_size, out_size, aggregators, scalers, delta, dropout=0.0):
        super().__init__()
        self.in_size, self.out_size = in_size, out_size
        self.aggregators, self.scalers, self.delta = aggregators, scalers, delta
        self.M = F.nn.Linear(2 * in_size, in_size)
        self.U = F.nn.Linear((len(aggregators) * len(scalers) + 1) * in_size, out_size)
        self.dropout = F.nn.Dropout(dropout)
        self.batchnorm = F.nn.BatchNorm1d(out_size)

    def _aggregate(self, graph, h_src, h_dst):
        if not h_src.is_cuda:
            return _host_aggregate(graph, h_src, h_dst, self.M, self.aggregators, self.scalers, self.delta)
        fi = self.in_size
        pad = ops.head_width_padded(fi, h_src.dtype, pow2=False) - fi
        p = _linear(h_src, _pad_rows(self.M.weight[:, :fi], pad))
        q = _linear(h_dst, _pad_rows(self.M.weight[:, fi:], pad), _pad_rows(self.M.bias, pad))
        out = ops_agg.multi_aggregate(graph, p, q, self.aggregators, self.scalers, self.delta)
        if pad:                                     # the zero columns of every block go
            out = out.view(out.shape[0], -1, fi + pad)[:, :, :fi].reshape(out.shape[0], -1)
        return out

    def forward(self, graph, h_src, h_dst, snorm_n=None):
        h = _linear(F.cat([h_dst, self._aggregate(graph, h_src, h_dst)], 1), self.U.weight, self.U.bias)
        if snorm_n is not None:
            h = h * snorm_n.to(h.dtype)
        if h.dtype == F.float32 or not h.is_cuda:
            h = self.batchnorm(h)
        else:                                       # bf16 activations: the statistics in fp32
            h = self.batchnorm(h.float()).to(h.dtype)
        return self.dropout(h)


class PNAConv(F.nn.Module):
    """DGL's PNAConv.  forward(graph, node_feat, edge_feat=None, snorm_n=None) -> [n_dst, out_size]."""

    def __init__(self, in_size, out_size, aggregators, scalers, delta, dropout=0.0, num_towers=1, edge_feat_size=0, residual=True):
        super().__init__()
        if edge_feat_size != 0:
            raise NotImplementedError("PNAConv: edge features are not built (edge_feat_size must be 0): the fused aggregation rests on "
                                      "the message splitting into a source and a destination term, and a per-edge term does not split")
        if num_towers < 1 or in_size % num_towers or out_size % num_towers:
            raise ValueError("PNAConv: in_size = %d and out_size = %d must be divisible by num_towers = %d" % (in_size, out_size, num_towers))
        if residual and in_size != out_size:
            raise ValueError("PNAConv: residual=True requires in_size == out_size (got %d and %d)" % (in_size, out_size))
        aggregators = (aggregators,) if isinstance(aggregators, str) else tuple(aggregators)
        scalers = (scalers,) if isinstance(scalers, str) else tuple(scalers)
        ops_agg._codes(aggregators, ops_agg.AGGREGATORS, "aggregator")          # unknown, repeated and unbuilt names raise here
        ops_agg._codes(scalers, ops_agg.SCALERS, "scaler")
        if not float(delta) > 0.0:
            raise ValueError("PNAConv: delta must be positive, got %r" % (delta,))
        self.in_size, self.out_size, self.num_towers, self.residual = in_size, out_size, num_towers, residual
        self.aggregators, self.scalers, self.delta = aggregators, scalers, float(delta)
        self.tower_in_size, self.tower_out_size = in_size // num_towers, out_size // num_towers
        self.towers = F.nn.ModuleList([PNAConvTower(self.tower_in_size, self.tower_out_size, aggregators, scalers, self.delta, dropout)
                                       for _ in range(num_towers)])
        self.mixing_layer = F.nn.Sequential(F.nn.Linear(out_size, out_size), F.nn.LeakyReLU())

    def forward(self, graph, node_feat, edge_feat=None, snorm_n=None):
        if edge_feat is not None:
            raise NotImplementedError("PNAConv: edge features are not built: a per-edge term does not split into source + destination")
        graph = as_csr_graph(graph)
        h_src, h_dst = _split_feat(graph, node_feat)
        if h_src.shape[1] != self.in_size or h_dst.shape[1] != self.in_size:
            raise ValueError("PNAConv: features of width %d / %d for in_size = %d" % (h_src.shape[1], h_dst.shape[1], self.in_size))
        # bf16 features on the GPU: fp32 inside, one rounding at the end.  Any activation stored in bf16 ahead of the mixing layer flips
        # the sign of ~0.3 % of the LeakyReLU's inputs, and its derivative jumps from 1 to 0.01 there: rounding h_neigh, U's output or
        # the batch norm's output alone, everything else float64, moves EVERY parameter gradient by 3e-2 .. 5e-2 relative L2 (64
        # columns, 4 towers, 1024 nodes), and messages rounded to bf16 move M.weight's by 5e-2 more (other entries attain max / min, a
        # small std drowns in the rounding) -- against a bar of 1.5e-2.
        dtype, same = h_src.dtype, h_dst is h_src
        if h_src.is_cuda and dtype != F.float32:
            h_src = h_src.float()
            h_dst = h_src if same else h_dst.float()
        fi = self.tower_in_size
        outs = []
        for t, tower in enumerate(self.towers):
            hs = h_src if self.num_towers == 1 else h_src[:, t * fi:(t + 1) * fi]
            hd = hs if same else (h_dst if self.num_towers == 1 else h_dst[:, t * fi:(t + 1) * fi])
            outs.append(tower(graph, hs, hd, snorm_n))
        h = outs[0] if self.num_towers == 1 else F.cat(outs, 1)
        h = self.mixing_layer[1](_linear(h, self.mixing_layer[0].weight, self.mixing_layer[0].bias))
        return (h + h_dst if self.residual else h).to(dtype)

    def extra_repr(self):
        return "in_size=%d, out_size=%d, aggregators=%s, scalers=%s, delta=%g, num_towers=%d, residual=%s" % (
            self.in_size, self.out_size, list(self.aggregators), list(self.scalers), self.delta, self.num_towers, self.residual)


class PNA(F.nn.Module):
    """h = embed(x); n_layers PNAConv(nhid, nhid) with a ReLU between them; logits = cls(h).  forward(graph, x) -> [N, nclass]."""

    def __init__(self, nfeat, nhid, nclass, n_layers=2, aggregators=("mean", "max", "min", "std"),
                 scalers=("identity", "amplification", "attenuation"), delta=1.0, dropout=0.0, num_towers=1, residual=True):
        super().__init__()
        self.embed = F.nn.Linear(nfeat, nhid)
        self.layers = F.nn.ModuleList([PNAConv(nhid, nhid, aggregators, scalers, delta, dropout, num_towers, 0, residual)
                                       for _ in range(n_layers)])
        self.cls = F.nn.Linear(nhid, nclass)

    def forward(self, graph, x):
        graph = as_csr_graph(graph)
        h = _linear(x, self.embed.weight, self.embed.bias)
        for layer in self.layers:
            h = F.nn.functional.relu(layer(graph, h))
        return _linear(h, self.cls.weight, self.cls.bias)
