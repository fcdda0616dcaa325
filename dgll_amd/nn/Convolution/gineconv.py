"""Graph isomorphism layer with edge features (DGL's GINEConv, "Strategies for Pre-training Graph Neural Networks": argument names,
parameter name and shape) on the gfx950 aggregation engine.

    GINEConv(apply_func=None, init_eps=0, learn_eps=False)
    GINE(nfeat, edge_feat, nhid, nclass, n_layers=2)      a model of GINEConv layers, each with its own encoder of the edge attributes

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
"""
from ... import backend as F
from ... import ops_edge, ops_ef
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


class GINEConv(F.nn.Module):
    """DGL's GINEConv.  forward(graph, node_feat, edge_feat) -> apply_func's output, [n_dst, F] without one; node_feat: a tensor
    [n_src, F], or (feat_src, feat_dst) for blocks; edge_feat [nnz, F] in the graph's entry order."""

    def __init__(self, apply_func=None, init_eps=0, learn_eps=False):
        super().__init__()
        self.apply_func = apply_func
        eps = F.tensor([float(init_eps)])
        if learn_eps:
            self.eps = F.nn.Parameter(eps)
        else:
            self.register_buffer("eps", eps)

    def forward(self, graph, node_feat, edge_feat):
        graph = as_csr_graph(graph)
        h_src, h_dst = _split_feat(graph, node_feat)
        _check_edge_feat(graph, h_src, edge_feat, "GINEConv")
        out = (1 + self.eps.to(h_dst.dtype)) * h_dst + _aggregate(graph, h_src, edge_feat, "add", "relu")
        return out if self.apply_func is None else self.apply_func(out)

    def extra_repr(self):
        return "learn_eps=%s" % isinstance(self.eps, F.nn.Parameter)


class GINE(F.nn.Module):
    """n_layers of: e = enc_l(edge_attr); h = relu(lin_l(GINEConv_l(graph, h, e))), then logits = cls(h).  Every layer has its own
    Linear(edge_feat, width) encoder of the edge attributes (the width of that layer's input) and a learned eps.
    forward(graph, x, edge_attr) -> logits [N, nclass]; edge_attr [nnz, edge_feat] in the graph's entry order."""

    def __init__(self, nfeat, edge_feat, nhid, nclass, n_layers=2):
        super().__init__()
        widths = [nfeat] + [nhid] * (n_layers - 1)
        self.edge_encoders = F.nn.ModuleList([F.nn.Linear(edge_feat, w) for w in widths])
        self.convs = F.nn.ModuleList([GINEConv(None, 0, learn_eps=True) for _ in widths])
        self.lins = F.nn.ModuleList([F.nn.Linear(w, nhid) for w in widths])
        self.cls = F.nn.Linear(nhid, nclass)

    def forward(self, graph, x, edge_attr):
        graph = as_csr_graph(graph)
        h = x
        for enc, conv, lin in zip(self.edge_encoders, self.convs, self.lins):
            e = _linear(enc, edge_attr).to(h.dtype)
            h = F.nn.functional.relu(_linear(lin, conv(graph, h, e)))
        return _linear(self.cls, h)
