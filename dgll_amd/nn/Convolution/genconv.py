"""The generalized graph convolution of DeeperGCN (PyG's GENConv; Li et al., "DeeperGCN: All You Need to Train Deeper GCNs":
argument names, module names and hence state-dict keys) on the gfx950 aggregation engine.

    GENConv(in_channels, out_channels, aggr="softmax", t=1.0, learn_t=False, p=1.0, learn_p=False, msg_norm=False,
            learn_msg_scale=False, norm="batch", num_layers=2, expansion=2, eps=1e-7, bias=False, edge_dim=None)
    DeeperGCN(in_channels, hidden, out_channels, num_layers, ...)      res+ blocks: h = h + conv(dropout(relu(norm(h))))

Over the entries of the graph (a CSRGraph [n_dst x n_src], anything as_csr_graph takes; rectangular blocks of NeighborSampler
allowed; edge values are ignored), entry k of row i being the edge j -> i and edge_attr[k] its row in the graph's entry order
(ops_ef.edge_graph_from_coo puts COO edge data into that order):

    m_k   = relu(lin_src(x_j) + lin_edge(edge_attr_k)) + eps
    agg_i = softmax aggregation: sum_k softmax_k(t m_k) m_k      or power mean: (mean_k min(m_k, 100)^p)^(1/p)       per column
    out_i = mlp(msg_norm(x_i, agg_i) + lin_dst(x_i))

`in_channels` is an int or a (src, dst) pair; forward(graph, x, edge_attr=None) takes x as a tensor or as (x_src, x_dst).  lin_src is
present when the source width differs from out_channels, lin_dst when the destination width does (otherwise x_i itself is added),
lin_edge when edge_dim is given and differs from out_channels -- a plain Linear that produces the [nnz, out_channels] array; fusing it
into the gather is not built.  aggr is "softmax", "softmax_sg" (the weights are constants of the backward) or "power" / "powermean";
anything else raises NotImplementedError.  aggr_module.t / aggr_module.p has shape [1]: a Parameter when learned, else a buffer.
msg_norm (MessageNorm: normalize(agg_i) * ||x_i||_2 * scale, msg_norm.scale a Parameter [1] that is trained iff learn_msg_scale).
mlp: Linear, norm, ReLU, Dropout(0) repeated, a plain Linear last, of widths [out] + [out * expansion] * (num_layers - 1) + [out];
norm is "batch", "layer" or None.  PyG's PowerMeanAggregation skips the clamp and the powers when p == 1 exactly; here the formula
always holds -- the two differ only for messages above 100.

On the GPU the projections run through dense.linear and the aggregation is ONE autograd node of ops_softagg: nothing of the size of
the edge list is stored but lin_edge's output and its gradient, and t / p reach the kernels as a pointer, never through the host.
An out_channels that is not a whole number of 16-byte vectors is padded with zero columns, which are sliced off right after the
aggregation (a zero column aggregates to eps, not to 0).  bf16 activations keep fp32 parameters; the element-wise tail and the norms
are formed in fp32.  Host tensors (any float dtype) take `_host_soft_aggregate`, the same formulas with torch's index ops, so that the
layer's own logic can be exercised without a GPU; a GPU tensor never reaches it.
"""
from ... import backend as F
from ... import ops, ops_softagg
from ...graph import as_csr_graph
from .dotgatconv import _split_feat
from .pnaconv import _linear, _pad_rows

_AGGR = {"softmax": ("softmax", False), "softmax_sg": ("softmax", True), "power": ("power", False), "powermean": ("power", False)}


def _host_soft_aggregate(graph, x, e, theta, mode, semi_grad=False, eps=1e-7):
    """out [n_dst, F] with per-edge tensors (host tensors only); theta: a one-element tensor."""
    row, col = graph.row_index(), graph.col.long()
    m = F.relu(x[col] if e is None else x[col] + e) + eps
    n, width = graph.n_rows, x.shape[1]
    zeros = F.zeros(n, width, dtype=x.dtype)
    theta = theta.to(x.dtype)
    if mode == "softmax":
        z = theta * m
        if semi_grad:
            z = z.detach()
        index = row.unsqueeze(1).expand(-1, width)
        top = F.full((n, width), -float("inf"), dtype=x.dtype).scatter_reduce(0, index, z.detach(), "amax", include_self=True)
        w = F.exp(z - top[row])
        return zeros.index_add(0, row, w / zeros.index_add(0, row, w)[row] * m)
    deg = graph.degrees()
    live = (deg > 0).unsqueeze(1)
    mean = zeros.index_add(0, row, m.clamp(max=100.0) ** theta) / deg.clamp(min=1).to(x.dtype).unsqueeze(1)
    return F.where(live, F.where(live, mean, F.ones_like(mean)) ** (1.0 / theta), zeros)


class SoftAggregation(F.nn.Module):
    """The aggregation of a GENConv: mode "softmax" (parameter t) or "power" (parameter p), a Parameter [1] when `learn`, else a buffer."""

    def __init__(self, mode, value=1.0, learn=False, semi_grad=False, eps=1e-7):
        super().__init__()
        if mode == "power" and float(value) == 0.0:
            raise ValueError("GENConv: p must not be 0 (the geometric mean is not built)")
        if mode == "power" and not eps > 0:
            raise ValueError("GENConv: the power mean needs eps > 0 (a zero message has no power mean), got %r" % (eps,))
        if semi_grad and learn:
            raise ValueError("GENConv: aggr='softmax_sg' treats the weights as constants, so t cannot be learned (learn_t=False)")
        self.mode, self.name, self.learn, self.semi_grad, self.eps = mode, "t" if mode == "softmax" else "p", bool(learn), bool(semi_grad), float(eps)
        value = F.full((1,), float(value))
        if learn:
            self.register_parameter(self.name, F.nn.Parameter(value))
        else:
            self.register_buffer(self.name, value)

    def forward(self, graph, x, e=None):
        theta = getattr(self, self.name)
        if not x.is_cuda:
            return _host_soft_aggregate(graph, x, e, theta, self.mode, self.semi_grad, self.eps)
        if self.mode == "softmax":
            return ops_softagg.softmax_aggregate(graph, x, e, theta, self.semi_grad, self.eps)
        return ops_softagg.powermean_aggregate(graph, x, e, theta, self.eps)

    def extra_repr(self):
        return "%s, learn=%s%s" % (self.mode, self.learn, ", semi_grad=True" if self.semi_grad else "")


class MessageNorm(F.nn.Module):
    """normalize(msg) * ||x||_2 * scale (PyG's MessageNorm)."""

    def __init__(self, learn_scale=False):
        super().__init__()
        self.scale = F.nn.Parameter(F.ones(1), requires_grad=bool(learn_scale))

    def forward(self, x, msg):
        return F.nn.functional.normalize(msg, p=2.0, dim=-1) * x.norm(p=2, dim=-1, keepdim=True) * self.scale.to(msg.dtype)


def _pad_cols(t, pad):
    return t if not pad else F.cat([t, t.new_zeros((t.shape[0], pad))], 1)


def _run_mlp(mlp, h, dtype):
    """mlp(h), h fp32 or of `dtype`: the Linears through dense.linear on activations of `dtype`, everything else in h's own precision"""
    for layer in mlp:
        if isinstance(layer, F.nn.Linear):
            h = _linear(h.to(dtype), layer.weight, layer.bias)
            h = h.float() if dtype == F.bfloat16 else h
        else:
            h = layer(h)
    return h


class GENConv(F.nn.Module):
    """PyG's GENConv.  forward(graph, x, edge_attr=None) -> [n_dst, out_channels]; x: a tensor [n_src, in_channels], or (x_src, x_dst)
    for blocks; edge_attr [nnz, edge_dim] in the graph's entry order."""

    def __init__(self, in_channels, out_channels, aggr="softmax", t=1.0, learn_t=False, p=1.0, learn_p=False, msg_norm=False,
                 learn_msg_scale=False, norm="batch", num_layers=2, expansion=2, eps=1e-7, bias=False, edge_dim=None):
        super().__init__()
        if not isinstance(aggr, str) or aggr not in _AGGR:
            raise NotImplementedError("GENConv: aggr must be 'softmax', 'softmax_sg', 'power' or 'powermean', got %r (other aggregations "
                                      "and MultiAggregation are not built)" % (aggr,))
        if norm not in ("batch", "layer", None):
            raise ValueError("GENConv: norm must be 'batch', 'layer' or None, got %r" % (norm,))
        if num_layers < 1 or expansion < 1:
            raise ValueError("GENConv: num_layers and expansion must be >= 1, got %r and %r" % (num_layers, expansion))
        pair = isinstance(in_channels, (tuple, list))
        src, dst = in_channels if pair else (in_channels, in_channels)
        self.in_channels, self.out_channels = in_channels, int(out_channels)
        self.aggr, self.eps, self.edge_dim = aggr, float(eps), edge_dim
        mode, semi = _AGGR[aggr]
        self.aggr_module = SoftAggregation(mode, t if mode == "softmax" else p, learn_t if mode == "softmax" else learn_p, semi, eps)
        if src != out_channels:
            self.lin_src = F.nn.Linear(src, out_channels, bias=bias)
        if edge_dim is not None and edge_dim != out_channels:
            self.lin_edge = F.nn.Linear(edge_dim, out_channels, bias=bias)
        if dst != out_channels:
            self.lin_dst = F.nn.Linear(dst, out_channels, bias=bias)
        widths = [out_channels] + [out_channels * expansion] * (num_layers - 1) + [out_channels]
        layers = []
        for i in range(1, len(widths)):
            layers.append(F.nn.Linear(widths[i - 1], widths[i], bias=bias))
            if i < len(widths) - 1:
                if norm == "batch":
                    layers.append(F.nn.BatchNorm1d(widths[i]))
                elif norm == "layer":
                    layers.append(F.nn.LayerNorm(widths[i]))
                layers += [F.nn.ReLU(), F.nn.Dropout(0.0)]
        self.mlp = F.nn.Sequential(*layers)
        if msg_norm:
            self.msg_norm = MessageNorm(learn_msg_scale)

    def forward(self, graph, x, edge_attr=None):
        graph = as_csr_graph(graph)
        x_src, x_dst = _split_feat(graph, x)
        if x_src.dtype != x_dst.dtype:
            raise TypeError("GENConv: source and destination features must have one dtype, got %s and %s" % (x_src.dtype, x_dst.dtype))
        dtype, width = x_src.dtype, self.out_channels
        pad = ops.head_width_padded(width, dtype, pow2=False) - width if x_src.is_cuda else 0
        lin = lambda name, h: _linear(h, _pad_rows(getattr(self, name).weight, pad),        # noqa: E731
                                      None if getattr(self, name).bias is None else _pad_rows(getattr(self, name).bias, pad))
        h = lin("lin_src", x_src) if hasattr(self, "lin_src") else _pad_cols(x_src, pad)
        e = None
        if edge_attr is not None:
            if edge_attr.dtype != dtype:
                raise TypeError("GENConv: edge_attr must have the features' dtype, got %s and %s" % (edge_attr.dtype, dtype))
            if edge_attr.dim() != 2 or edge_attr.shape[0] != graph.nnz:
                raise ValueError("GENConv: edge_attr must be [nnz, edge_dim] with nnz = %d, got %s" % (graph.nnz, tuple(edge_attr.shape)))
            if hasattr(self, "lin_edge"):
                e = lin("lin_edge", edge_attr)
            elif edge_attr.shape[1] != width:
                raise ValueError("GENConv: edge_attr has %d columns and the messages %d: give edge_dim so that lin_edge projects them"
                                 % (edge_attr.shape[1], width))
            else:
                e = _pad_cols(edge_attr, pad)
        out = self.aggr_module(graph, h, e)
        if pad:
            out = out[:, :width]
        # what follows is element-wise or a norm: bf16 activations take it in fp32
        up = (lambda t: t.float()) if dtype == F.bfloat16 else (lambda t: t)
        out = up(out)
        if hasattr(self, "msg_norm"):
            out = self.msg_norm(up(x_dst), out)
        out = out + up(_linear(x_dst, self.lin_dst.weight, self.lin_dst.bias) if hasattr(self, "lin_dst") else x_dst)
        return _run_mlp(self.mlp, out, dtype).to(dtype)

    def extra_repr(self):
        return "%s, %d, aggr=%s" % (self.in_channels, self.out_channels, self.aggr)


class DeeperGCN(F.nn.Module):
    """DeeperGCN with res+ blocks: h = encoder(x); h = conv_0(h); then for every further layer h = h + conv(dropout(relu(norm(h))));
    logits = cls(dropout(relu(norm(h)))).  forward(graph, x, edge_attr=None) -> [N, out_channels]; `edge_dim` attributes go to every layer.
    `mlp_layers` is the num_layers of every GENConv; `activation` replaces the relu of the blocks (the tests use a smooth one for bf16)."""

    def __init__(self, in_channels, hidden, out_channels, num_layers, aggr="softmax", t=1.0, learn_t=True, p=1.0, learn_p=False,
                 msg_norm=False, learn_msg_scale=False, norm="layer", dropout=0.0, edge_dim=None, mlp_layers=2,
                 activation=F.nn.functional.relu):
        super().__init__()
        if norm not in ("batch", "layer"):
            raise ValueError("DeeperGCN: norm must be 'batch' or 'layer', got %r" % (norm,))
        self.encoder = F.nn.Linear(in_channels, hidden)
        self.convs = F.nn.ModuleList([GENConv(hidden, hidden, aggr=aggr, t=t, learn_t=learn_t, p=p, learn_p=learn_p, msg_norm=msg_norm,
                                              learn_msg_scale=learn_msg_scale, norm=norm, num_layers=mlp_layers, edge_dim=edge_dim)
                                      for _ in range(num_layers)])
        make = F.nn.BatchNorm1d if norm == "batch" else F.nn.LayerNorm
        self.norms = F.nn.ModuleList([make(hidden) for _ in range(num_layers)])
        self.dropout = F.nn.Dropout(dropout)
        self.activation = activation
        self.cls = F.nn.Linear(hidden, out_channels)

    def _block(self, h, norm):
        """dropout(activation(norm(h))): the norm in fp32, the result in h's dtype"""
        return self.dropout(self.activation(norm(h.float() if h.dtype == F.bfloat16 else h))).to(h.dtype)

    def forward(self, graph, x, edge_attr=None):
        graph = as_csr_graph(graph)
        h = _linear(x, self.encoder.weight, self.encoder.bias)
        h = self.convs[0](graph, h, edge_attr)
        for conv, norm in zip(self.convs[1:], self.norms[:-1]):
            h = h + conv(graph, self._block(h, norm), edge_attr)
        return _linear(self._block(h, self.norms[-1]), self.cls.weight, self.cls.bias)
