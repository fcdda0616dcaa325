"""Graph isomorphism layer with edge features (DGL's GINEConv, "Strategies for Pre-training Graph Neural Networks": argument names,
parameter name and shape) on the gfx950 aggregation engine.

    GINEConv(apply_func=None, init_eps=0, learn_eps=False, edge_dim=None, in_feats=None)
    GINE(nfeat, edge_feat, nhid, nclass, n_layers=2, fused_edge=False)
                                                          a model of GINEConv layers, each with its own encoder of the edge attributes

Over the entries j of row i of the graph (a CSRGraph [n_dst x n_src], anything as_csr_graph takes; rectangular blocks of
NeighborSampler allowed; edge values are ignored), with e_ij the feature row of that entry, of the node features' width and in the
graph's entry order (ops_ef.edge_graph_from_coo puts COO edge data into that order):

    out_i = apply_func((1 + eps) * h_i + sum_j relu(h_j + e_ij))

`eps` is a 1-element Parameter, or a buffer of the same name when learn_eps=False (state_dict() has the one key "eps" either way,
as DGL's has).  A row without entries aggregates 0.  The aggregation is ONE pass of ops_ef (u_add_e_sum with act="relu"): neither
h_j + e_ij nor its relu exists per edge, and the backward recomputes the gate.  A feature width that is not a whole number of
16-byte vectors is padded with zero columns on h and e alike (relu(0 + 0) = 0) and unpadded after the aggregation.  Edge attributes
of another width go through a Linear first, which is what GINE does per layer.  Host tensors take `_host_aggregate`, the same
semantics with torch's index ops, so that the layer's own logic can be exercised without a GPU; a GPU tensor never reaches it.

With edge_dim (PyG's argument; in_feats, the node width, is then required) the layer owns that Linear as `lin` (PyG's name) and
forward takes the RAW attributes [nnz, edge_dim], edge_dim <= 16: e_ij = lin(a_ij) is formed inside the aggregation kernel
(ops_efp.u_op_proj_e_sum) and no [nnz, F] array exists in the forward or the backward.  GINE(fused_edge=True) hands each layer its
encoder's weight and bias that way; parameters and state_dict() keys are the same either way.
"""
from ... import backend as F
from ... import ops_edge, ops_ef, ops_efp
from ...graph import as_csr_graph
from .agnnconv import _linear
from .dotgatconv import _split_feat


def _host_aggregate(graph, h_src, e, op, act=None):
    """[n_dst, F]: sum over the entries of act(h_src[col_k] op e[k]), with per-edge tensors (host tensors only)."""
    row, col = graph.row_index(), graph.col.long()
    m = h_src[col] * e if op == "mul" else h_src[col] + e
    if act == "relu":
        m = F.nn.functional.relu(m)
    return F.zeros(graph.n_rows, h_src.shape[1], dtype=h_src.dtype).index_add_(0, row, m)


def _check_edge_feat(graph, h_src, e, name):
    if e.dim() != 2 or e.shape[0] != graph.nnz or e.shape[1] != h_src.shape[1]:
        raise ValueError("%s: edge features must be [nnz, F] = [%d, %d] in the graph's entry order, got %s (another width: project "
                         "them first)" % (name, graph.nnz, h_src.shape[1], tuple(e.shape)))
    if e.dtype != h_src.dtype:
        raise TypeError("%s: node and edge features must have one dtype, got %s and %s" % (name, h_src.dtype, e.dtype))


def _aggregate(graph, h_src, e, op, act=None):
    """ops_ef.u_op_e_sum on the GPU (zero columns up to a whole 16-byte vector, sliced off again), _host_aggregate for host tensors."""
    if not h_src.is_cuda:
        return _host_aggregate(graph, h_src, e, op, act)
    width = h_src.shape[1]
    pad = ops_edge.head_width_padded(width, h_src.dtype, pow2=False) - width
    if pad:                                         # zero columns: 0 under all three messages
        h_src, e = F.nn.functional.pad(h_src, (0, pad)), F.nn.functional.pad(e, (0, pad))
    out = ops_ef.u_op_e_sum(graph, h_src, e, op, act)
    return out[:, :width] if pad else out


def _aggregate_projected(graph, h_src, a, lin):
    """sum over the entries of relu(h_src[col_k] + lin(a[k])), lin a Linear(edge_dim, F): ops_efp.u_op_proj_e_sum on the GPU (h and
    the weight's output columns zero-padded to a whole 16-byte vector: relu(0 + 0) = 0; sliced off again), _linear then
    _host_aggregate for host tensors."""
    weight, bias = lin.weight, lin.bias
    if a.dim() != 2 or a.shape[0] != graph.nnz or a.shape[1] != weight.shape[1]:
        raise ValueError("GINEConv: edge features must be [nnz, edge_dim] = [%d, %d] in the graph's entry order, got %s"
                         % (graph.nnz, weight.shape[1], tuple(a.shape)))
    if a.dtype != h_src.dtype:
        raise TypeError("GINEConv: node and edge features must have one dtype, got %s and %s" % (h_src.dtype, a.dtype))
    if not h_src.is_cuda:
        return _host_aggregate(graph, h_src, _linear(lin, a), "add", "relu")
    width = h_src.shape[1]
    pad = ops_edge.head_width_padded(width, h_src.dtype, pow2=False) - width
    if pad:
        h_src, weight = F.nn.functional.pad(h_src, (0, pad)), F.nn.functional.pad(weight, (0, 0, 0, pad))
        bias = None if bias is None else F.nn.functional.pad(bias, (0, pad))
    out = ops_efp.u_op_proj_e_sum(graph, h_src, a, weight, bias, "add", "relu")
    return out[:, :width] if pad else out


class GINEConv(F.nn.Module):
    """DGL's GINEConv.  forward(graph, node_feat, edge_feat) -> apply_func's output, [n_dst, F] without one; node_feat: a tensor
    [n_src, F], or (feat_src, feat_dst) for blocks; edge_feat [nnz, F] in the graph's entry order -- with edge_dim: [nnz, edge_dim],
    projected by the layer's own `lin` = Linear(edge_dim, in_feats) inside the aggregation kernel."""

    def __init__(self, apply_func=None, init_eps=0, learn_eps=False, edge_dim=None, in_feats=None):
        super().__init__()
        self.apply_func = apply_func
        if edge_dim is not None:
            if in_feats is None:
                raise ValueError("GINEConv: edge_dim needs in_feats, the node feature width that the edge attributes are projected to")
            if not 1 <= int(edge_dim) <= ops_efp.MAX_DE:
                raise ValueError("GINEConv: edge_dim must be in 1..%d, got %r (wider attributes: project them first)" % (ops_efp.MAX_DE, edge_dim))
            self.lin = F.nn.Linear(int(edge_dim), int(in_feats))
        eps = F.tensor([float(init_eps)])
        if learn_eps:
            self.eps = F.nn.Parameter(eps)
        else:
            self.register_buffer("eps", eps)

    def forward(self, graph, node_feat, edge_feat):
        graph = as_csr_graph(graph)
        h_src, h_dst = _split_feat(graph, node_feat)
        if getattr(self, "lin", None) is not None:
            if h_src.shape[1] != self.lin.out_features:
                raise ValueError("GINEConv: node features have %d columns, in_feats is %d" % (h_src.shape[1], self.lin.out_features))
            agg = _aggregate_projected(graph, h_src, edge_feat, self.lin)
        else:
            _check_edge_feat(graph, h_src, edge_feat, "GINEConv")
            agg = _aggregate(graph, h_src, edge_feat, "add", "relu")
        out = (1 + self.eps.to(h_dst.dtype)) * h_dst + agg
        return out if self.apply_func is None else self.apply_func(out)

    def forward_projected(self, graph, node_feat, edge_attr, lin):
        """forward with e_ij = lin(a_ij) formed inside the aggregation, for a caller that owns the Linear (GINE)."""
        graph = as_csr_graph(graph)
        h_src, h_dst = _split_feat(graph, node_feat)
        out = (1 + self.eps.to(h_dst.dtype)) * h_dst + _aggregate_projected(graph, h_src, edge_attr, lin)
        return out if self.apply_func is None else self.apply_func(out)

    def extra_repr(self):
        return "learn_eps=%s" % isinstance(self.eps, F.nn.Parameter)


class GINE(F.nn.Module):
    """n_layers of: e = enc_l(edge_attr); h = relu(lin_l(GINEConv_l(graph, h, e))), then logits = cls(h).  Every layer has its own
    Linear(edge_feat, width) encoder of the edge attributes (the width of that layer's input) and a learned eps.
    forward(graph, x, edge_attr) -> logits [N, nclass]; edge_attr [nnz, edge_feat] in the graph's entry order.  fused_edge=True
    (edge_feat <= 16): e is not materialised -- each layer's aggregation forms it per entry from edge_attr and its encoder's weight
    and bias.  The parameters and state_dict() keys do not depend on it: one state dict loads into both."""

    def __init__(self, nfeat, edge_feat, nhid, nclass, n_layers=2, fused_edge=False):
        super().__init__()
        if fused_edge and not 1 <= int(edge_feat) <= ops_efp.MAX_DE:
            raise ValueError("GINE: fused_edge needs edge_feat in 1..%d, got %r" % (ops_efp.MAX_DE, edge_feat))
        self.fused_edge = bool(fused_edge)
        widths = [nfeat] + [nhid] * (n_layers - 1)
        self.edge_encoders = F.nn.ModuleList([F.nn.Linear(edge_feat, w) for w in widths])
        self.convs = F.nn.ModuleList([GINEConv(None, 0, learn_eps=True) for _ in widths])
        self.lins = F.nn.ModuleList([F.nn.Linear(w, nhid) for w in widths])
        self.cls = F.nn.Linear(nhid, nclass)

    def forward(self, graph, x, edge_attr):
        graph = as_csr_graph(graph)
        h = x
        for enc, conv, lin in zip(self.edge_encoders, self.convs, self.lins):
            if self.fused_edge:
                agg = conv.forward_projected(graph, h, edge_attr.to(h.dtype), enc)
            else:
                agg = conv(graph, h, _linear(enc, edge_attr).to(h.dtype))
            h = F.nn.functional.relu(_linear(lin, agg))
        return _linear(self.cls, h)
