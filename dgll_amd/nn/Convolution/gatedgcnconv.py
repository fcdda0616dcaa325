"""Gated graph convolution with edge outputs (DGL's GatedGCNConv, Bresson & Laurent's "Residual Gated Graph ConvNets" as the
benchmarking-GNNs suite and GraphGPS use it: argument names, module names and hence state-dict keys) on the gfx950 aggregation
engine.

    GatedGCNConv(input_feats, edge_feats, output_feats, dropout=0, batch_norm=True, residual=True, activation=relu)
    GatedGCN(nfeat, efeat, nhid, nclass, layers=2)        node and edge embeddings, GatedGCNConv layers, a node classifier

Over the entries of the graph (a CSRGraph [n_dst x n_src], anything as_csr_graph takes; rectangular blocks of NeighborSampler
allowed; edge values are ignored), entry k of row i being the edge j -> i with the feature row edge_feat[k] in the graph's entry
order (ops_ef.edge_graph_from_coo puts COO edge data into that order):

    ehat_k = C(edge_feat_k) + D(feat_j) + E(feat_i)
    h_i    = A(feat_i) + (sum_k sigmoid(ehat_k) * B(feat_j)) / (sum_k sigmoid(ehat_k) + 1e-6)          e_k = ehat_k
    batch norm of h (bn_node) and e (bn_edge), the activation of both, the residual (h = feat + h, e = edge_feat + e), dropout of both

forward returns (h [n_dst, output_feats], e [nnz, output_feats]): the layer updates the edge features too, and the next layer takes
them.  `residual` silently turns off when input_feats or edge_feats differs from output_feats, as in DGL.  The submodules are the
Linear layers A, B, C, D, E (all with bias) and the BatchNorm1d layers bn_node and bn_edge.  With a (feat_src, feat_dst) pair A and E
apply to feat_dst, B and D to feat_src, and the residual adds feat_dst.

On the GPU the five projections run through dense.linear and the gather is ONE autograd node of ops_gated (gated_sum): per edge only
C's output, ehat and their gradients exist, and the backward recomputes the gate from the stored ehat.  An output width that is not
a whole number of 16-byte vectors is padded with zero weight rows (a padded column has ehat = 0, a gate of 1/2 and values of 0) and
sliced off after the aggregation.  bf16 activations keep fp32 parameters; the element-wise tail of the layer (the sum A h + out, batch
norm, activation, residual) is formed in fp32 and rounded once.  Host
tensors take `_host_gated_sum`, the same formula with torch's index ops, so that the layer's own logic can be exercised without a
GPU; a GPU tensor never reaches it.
"""
from ... import backend as F
from ... import ops, ops_gated
from ...graph import as_csr_graph
from .dotgatconv import _split_feat
from .pnaconv import _linear, _pad_rows

EPS = 1e-6


def _host_gated_sum(graph, a, b, c, v, eps=EPS):
    """(out [n_dst, F], ehat [nnz, F]) with per-edge tensors (host tensors only)."""
    row, col = graph.row_index(), graph.col.long()
    ehat = c + a[row] + b[col]
    sig = F.sigmoid(ehat)
    num = F.zeros(graph.n_rows, a.shape[1], dtype=a.dtype).index_add_(0, row, sig * v[col])
    den = F.zeros(graph.n_rows, a.shape[1], dtype=a.dtype).index_add_(0, row, sig)
    return num / (den + eps), ehat


class GatedGCNConv(F.nn.Module):
    """DGL's GatedGCNConv.  forward(graph, feat, edge_feat) -> (h [n_dst, output_feats], e [nnz, output_feats]); feat: a tensor
    [n_src, input_feats], or (feat_src, feat_dst) for blocks; edge_feat [nnz, edge_feats] in the graph's entry order."""

    def __init__(self, input_feats, edge_feats, output_feats, dropout=0, batch_norm=True, residual=True, activation=F.nn.functional.relu):
        super().__init__()
        self.dropout = F.nn.Dropout(dropout)
        self.batch_norm = batch_norm
        self.residual = residual and input_feats == output_feats and edge_feats == output_feats
        self.A = F.nn.Linear(input_feats, output_feats, bias=True)
        self.B = F.nn.Linear(input_feats, output_feats, bias=True)
        self.C = F.nn.Linear(edge_feats, output_feats, bias=True)
        self.D = F.nn.Linear(input_feats, output_feats, bias=True)
        self.E = F.nn.Linear(input_feats, output_feats, bias=True)
        self.bn_node = F.nn.BatchNorm1d(output_feats)
        self.bn_edge = F.nn.BatchNorm1d(output_feats)
        self.activation = activation

    def forward(self, graph, feat, edge_feat):
        graph = as_csr_graph(graph)
        h_src, h_dst = _split_feat(graph, feat)
        if edge_feat.dim() != 2 or edge_feat.shape[0] != graph.nnz:
            raise ValueError("GatedGCNConv: edge features must be [nnz, edge_feats] with nnz = %d in the graph's entry order, got %s"
                             % (graph.nnz, tuple(edge_feat.shape)))
        if edge_feat.dtype != h_src.dtype:
            raise TypeError("GatedGCNConv: node and edge features must have one dtype, got %s and %s" % (h_src.dtype, edge_feat.dtype))
        width = self.A.out_features
        pad = ops.head_width_padded(width, h_src.dtype, pow2=False) - width if h_src.is_cuda else 0
        ah, bh, dh, eh, ce = (_linear(x, _pad_rows(fc.weight, pad), _pad_rows(fc.bias, pad)) for fc, x in
                              ((self.A, h_dst), (self.B, h_src), (self.D, h_src), (self.E, h_dst), (self.C, edge_feat)))
        if h_src.is_cuda:
            out, e = ops_gated.gated_sum(graph, eh, dh, ce, bh, EPS)
        else:
            out, e = _host_gated_sum(graph, eh, dh, ce, bh)
        # what follows is element-wise: bf16 activations take it in fp32 and are rounded once, at the end
        up = (lambda t: t.float()) if h_src.dtype == F.bfloat16 else (lambda t: t)
        h, e = up(ah) + up(out), up(e)
        if pad:
            h, e = h[:, :width], e[:, :width]
        if self.batch_norm:
            h, e = self.bn_node(h), self.bn_edge(e)
        if self.activation is not None:
            h, e = self.activation(h), self.activation(e)
        if self.residual:
            h, e = up(h_dst) + h, up(edge_feat) + e
        return self.dropout(h.to(h_src.dtype)), self.dropout(e.to(h_src.dtype))

    def extra_repr(self):
        return "batch_norm=%s, residual=%s" % (self.batch_norm, self.residual)


class GatedGCN(F.nn.Module):
    """h = embed_h(x), e = embed_e(edge_attr); `layers` of (h, e) = GatedGCNConv(graph, h, e) at width nhid; logits = cls(h).
    forward(graph, x, edge_attr) -> logits [N, nclass]; edge_attr [nnz, efeat] in the graph's entry order."""

    def __init__(self, nfeat, efeat, nhid, nclass, layers=2, dropout=0.0, batch_norm=True, residual=True, activation=F.nn.functional.relu):
        super().__init__()
        self.embed_h = F.nn.Linear(nfeat, nhid)
        self.embed_e = F.nn.Linear(efeat, nhid)
        self.convs = F.nn.ModuleList([GatedGCNConv(nhid, nhid, nhid, dropout, batch_norm, residual, activation) for _ in range(layers)])
        self.cls = F.nn.Linear(nhid, nclass)

    def forward(self, graph, x, edge_attr):
        graph = as_csr_graph(graph)
        h = _linear(x, self.embed_h.weight, self.embed_h.bias)
        e = _linear(edge_attr, self.embed_e.weight, self.embed_e.bias).to(h.dtype)
        for conv in self.convs:
            h, e = conv(graph, h, e)
        return _linear(h, self.cls.weight, self.cls.bias)
