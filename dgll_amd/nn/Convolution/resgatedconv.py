"""Residual gated graph convolution without edge features (PyG's ResGatedGraphConv, Bresson & Laurent's "Residual Gated Graph
ConvNets": argument names, module names and hence state-dict keys) on the gfx950 aggregation engine.

    ResGatedGraphConv(in_channels, out_channels, act=None, edge_dim=None, root_weight=True, bias=True, aggr="add")
    ResGatedGCN(nfeat, nhid, nclass, layers=2, dropout=0.0, aggr="mean")      conv, relu and dropout per layer, a linear classifier

Over the entries of the graph (a CSRGraph [n_dst x n_src], anything as_csr_graph takes; rectangular blocks of NeighborSampler
allowed; edge values are ignored), entry e of row i being the edge j -> i:

    out_i = sum_e sigmoid(lin_key(x_i) + lin_query(x_j)) * lin_value(x_j) + lin_skip(x_i) + bias        (aggr="mean": the sum / deg_i)

`in_channels` is an int or a (src, dst) pair; forward(graph, x) takes x as a tensor or as (x_src, x_dst): lin_key and lin_skip apply
to the destination features, lin_query and lin_value to the source features.  lin_key, lin_query and lin_value are Linear layers with
bias, lin_skip (present iff root_weight) one without, `bias` (present iff bias) a Parameter.  The gate is the sigmoid (`act` None or
torch.nn.Sigmoid; anything else raises NotImplementedError), and there are no edge features here (`edge_dim` other than None raises
NotImplementedError: GatedGCNConv is the layer with them).

On the GPU the projections run through dense.linear and the gather is ONE autograd node of ops_res_gated (res_gated_sum): the gate is
recomputed from two node rows in every pass and nothing of the size of the edge list is stored, forward or backward -- unlike
GatedGCNConv, whose edge features are [nnz, F] arrays.  An out_channels that is not a whole number of 16-byte vectors is padded with
zero weight rows (a padded column has a gate of 1/2 and a value of 0) and sliced off after the aggregation.  bf16 activations keep
fp32 parameters; the element-wise tail (the sum with lin_skip's output and the bias) is formed in fp32 and rounded once.  Host tensors
take `_host_res_gated_sum`, the same formula with torch's index ops, so that the layer's own logic can be exercised without a GPU; a
GPU tensor never reaches it.
"""
from ... import backend as F
from ... import ops, ops_res_gated
from ...graph import as_csr_graph
from .dotgatconv import _split_feat
from .pnaconv import _linear, _pad_rows

_AGGR = {"add": "sum", "sum": "sum", "mean": "mean"}


def _host_res_gated_sum(graph, k, q, v, reduce="sum"):
    """out [n_dst, F] with per-edge tensors (host tensors only)."""
    row, col = graph.row_index(), graph.col.long()
    out = F.zeros(graph.n_rows, k.shape[1], dtype=k.dtype).index_add_(0, row, F.sigmoid(k[row] + q[col]) * v[col])
    if reduce == "mean":
        out = out / graph.degrees().clamp(min=1).to(k.dtype).unsqueeze(1)
    return out


class ResGatedGraphConv(F.nn.Module):
    """PyG's ResGatedGraphConv.  forward(graph, x) -> [n_dst, out_channels]; x: a tensor [n_src, in_channels], or (x_src, x_dst) for
    blocks."""

    def __init__(self, in_channels, out_channels, act=None, edge_dim=None, root_weight=True, bias=True, aggr="add"):
        super().__init__()
        if not (act is None or act is F.nn.Sigmoid or isinstance(act, F.nn.Sigmoid)):
            raise NotImplementedError("ResGatedGraphConv: the gate is the sigmoid the kernels compute (act=None or torch.nn.Sigmoid), got %r" % (act,))
        if edge_dim is not None:
            raise NotImplementedError("ResGatedGraphConv: edge_dim is not supported here; GatedGCNConv is the gated layer with edge features")
        if aggr not in _AGGR:
            raise ValueError("ResGatedGraphConv: aggr must be 'add', 'sum' or 'mean', got %r" % (aggr,))
        pair = isinstance(in_channels, (tuple, list))
        src, dst = in_channels if pair else (in_channels, in_channels)
        self.in_channels, self.out_channels = in_channels, int(out_channels)
        self.edge_dim, self.root_weight, self.aggr = None, bool(root_weight), aggr
        self.lin_key = F.nn.Linear(dst, out_channels)
        self.lin_query = F.nn.Linear(src, out_channels)
        self.lin_value = F.nn.Linear(src, out_channels)
        if root_weight:
            self.lin_skip = F.nn.Linear(dst, out_channels, bias=False)
        else:
            self.register_parameter("lin_skip", None)
        if bias:
            self.bias = F.nn.Parameter(F.zeros(out_channels))
        else:
            self.register_parameter("bias", None)

    def forward(self, graph, x):
        graph = as_csr_graph(graph)
        x_src, x_dst = _split_feat(graph, x)
        if x_src.dtype != x_dst.dtype:
            raise TypeError("ResGatedGraphConv: source and destination features must have one dtype, got %s and %s" % (x_src.dtype, x_dst.dtype))
        width = self.out_channels
        pad = ops.head_width_padded(width, x_src.dtype, pow2=False) - width if x_src.is_cuda else 0
        k, q, v = (_linear(h, _pad_rows(fc.weight, pad), _pad_rows(fc.bias, pad)) for fc, h in
                   ((self.lin_key, x_dst), (self.lin_query, x_src), (self.lin_value, x_src)))
        if x_src.is_cuda:
            out = ops_res_gated.res_gated_sum(graph, k, q, v, _AGGR[self.aggr])
        else:
            out = _host_res_gated_sum(graph, k, q, v, _AGGR[self.aggr])
        # what follows is element-wise: bf16 activations take it in fp32 and are rounded once, at the end
        up = (lambda t: t.float()) if x_src.dtype == F.bfloat16 else (lambda t: t)
        out = up(out)
        if self.lin_skip is not None:
            out = out + up(_linear(x_dst, _pad_rows(self.lin_skip.weight, pad)))
        if pad:
            out = out[:, :width]
        if self.bias is not None:
            out = out + self.bias.to(out.dtype)
        return out.to(x_src.dtype)

    def extra_repr(self):
        return "%s, %d, aggr=%s, root_weight=%s" % (self.in_channels, self.out_channels, self.aggr, self.root_weight)


class ResGatedGCN(F.nn.Module):
    """`layers` of h = dropout(activation(ResGatedGraphConv(graph, h))), the first nfeat -> nhid, the others at width nhid; logits =
    cls(h).  forward(graph, x) -> logits [N, nclass]."""

    def __init__(self, nfeat, nhid, nclass, layers=2, dropout=0.0, aggr="mean", activation=F.nn.functional.relu):
        super().__init__()
        self.convs = F.nn.ModuleList([ResGatedGraphConv(nfeat if i == 0 else nhid, nhid, aggr=aggr) for i in range(layers)])
        self.dropout = F.nn.Dropout(dropout)
        self.activation = activation
        self.cls = F.nn.Linear(nhid, nclass)

    def forward(self, graph, x):
        graph = as_csr_graph(graph)
        h = x
        for conv in self.convs:
            h = self.dropout(self.activation(conv(graph, h)))
        return _linear(h, self.cls.weight, self.cls.bias)
