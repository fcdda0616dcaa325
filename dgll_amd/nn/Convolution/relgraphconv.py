"""RelGraphConv -- the relational graph convolution of R-GCN (Schlichtkrull et al., "Modeling Relational Data with Graph Convolutional
Networks"), with the argument names, the state dict and the order of operations of DGL's dgl.nn.pytorch.conv.RelGraphConv.

    h_i = act( LN?( sum_{e = (j -> i)} norm_e x_j W_{r_e} ) + h_bias + x_i loop_weight )

    regularizer="basis":  W_r = sum_b linear_r.coeff[r, b] linear_r.W[b]      (num_bases shared matrices, one coefficient row per type)
    regularizer=None:     W_r = linear_r.W[r]                                 (a matrix per type)

| parameter                       | shape                                                  | present       |
| linear_r.W                      | [num_bases, in, out] (basis), [num_rels, in, out] (None)| always        |
| linear_r.coeff                  | [num_rels, num_bases]                                  | basis only    |
| h_bias                          | [out]                                                  | bias=True     |
| loop_weight                     | [in, out]                                              | self_loop=True|
| layer_norm_weight.{weight,bias} | nn.LayerNorm(out)                                      | layer_norm    |

Initialisers as DGL's: W uniform in +-1/sqrt(in), coeff and loop_weight Xavier-uniform with the ReLU gain, h_bias zeros.  DGL is not
installed where this was written and the project this package was modelled on has no R-GCN, so there are no recorded DGL outputs
behind it: names and order of operations follow DGL's documented module, and parity is tested against a float64 restatement of the
formulas above (tests/typed_ref.py).

On the GPU the message sum never forms W_r or a per-edge message: Z[i, b, :] = sum_e norm_e coeff[r_e, b] x_j is ONE fused gather
(ops_typed.typed_spmm: x_j loaded once per edge, B accumulators) and h = Z . stack_b(W[b]) one dense transform of reduction length
B * in -- together with x_i loop_weight in a single launch (dense.sage_transform) when there is no layer norm, the activation is
ReLU or none, and no bias stands between the sum and the ReLU.  An `in` that is not a whole number of 16-byte vectors is padded: zero columns on
x, zero rows behind every basis block of the stacked weight.  regularizer=None takes the same path with B = num_rels and a frozen
identity table (a buffer outside the state dict; no gradient is formed for it), up to _MAX_DIRECT_RELS types; "bdd" is not built.
"""
import math

from ... import backend as F
from ... import dense, ops_typed
from ...graph import as_csr_graph
from ...ops_typed import TypedEdges

_MAX_DIRECT_RELS = 4 * ops_typed.BASIS_BLOCK      # regularizer=None: one accumulator block per 8 types, at most four gathers of x


def _host_aggregate(graph, edges, x, coeff):
    """Z [n_dst, B * F] of ops_typed.typed_spmm with torch index ops (host tensors only)."""
    row, col = graph.row_index(), graph.col.long()
    w = coeff.to(x.dtype)[edges.etypes.long()]                                   # [nnz, B]
    if edges.norm is not None:
        w = w * edges.norm.to(x.dtype).unsqueeze(1)
    xs = x[col]
    return F.cat([F.zeros(graph.n_rows, x.shape[1], dtype=x.dtype).index_add_(0, row, w[:, b:b + 1] * xs) for b in range(coeff.shape[1])], dim=1)


def _is_relu(activation):
    return activation is F.relu or activation is F.nn.functional.relu or isinstance(activation, F.nn.ReLU)


class _LinearR(F.nn.Module):
    """Holder of DGL's `linear_r` sub-module parameters (W, and coeff for the basis regulariser)."""

    def __init__(self, in_feat, out_feat, num_rels, num_bases, basis):
        super().__init__()
        self.W = F.Parameter(F.empty(num_bases if basis else num_rels, in_feat, out_feat))
        if basis:
            self.coeff = F.Parameter(F.empty(num_rels, num_bases))
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.W.shape[1])
        F.nn.init.uniform_(self.W, -bound, bound)
        if hasattr(self, "coeff"):
            F.nn.init.xavier_uniform_(self.coeff, gain=F.nn.init.calculate_gain("relu"))


class RelGraphConv(F.nn.Module):
    """DGL's RelGraphConv.  forward(graph, feat, etypes, norm=None) -> [n_dst, out_feat]."""

    def __init__(self, in_feat, out_feat, num_rels, regularizer=None, num_bases=None, bias=True, activation=None, self_loop=True,
                 dropout=0.0, layer_norm=False):
        super().__init__()
        self.in_feat, self.out_feat, self.num_rels = int(in_feat), int(out_feat), int(num_rels)
        if regularizer == "bdd":
            raise NotImplementedError('RelGraphConv: regularizer="bdd" (block-diagonal decomposition) is not built; use "basis" or None')
        if regularizer not in (None, "basis"):
            raise ValueError('RelGraphConv: regularizer must be None, "basis" or "bdd", got %r' % (regularizer,))
        self.regularizer = regularizer
        if regularizer is None:
            if self.num_rels > _MAX_DIRECT_RELS:
                raise NotImplementedError('RelGraphConv: regularizer=None holds a matrix per edge type and is built for num_rels <= %d '
                                          '(got %d); use regularizer="basis" with num_bases' % (_MAX_DIRECT_RELS, self.num_rels))
            self.num_bases = self.num_rels
            self.register_buffer("_identity", F.eye(self.num_rels), persistent=False)
        else:
            self.num_bases = self.num_rels if num_bases is None else int(num_bases)
            if self.num_bases < 1:
                raise ValueError("num_bases must be >= 1")
        self.linear_r = _LinearR(self.in_feat, self.out_feat, self.num_rels, self.num_bases, regularizer == "basis")
        if bias:
            self.h_bias = F.Parameter(F.zeros(self.out_feat))
        else:
            self.register_parameter("h_bias", None)
        if self_loop:
            self.loop_weight = F.Parameter(F.empty(self.in_feat, self.out_feat))
            F.nn.init.xavier_uniform_(self.loop_weight, gain=F.nn.init.calculate_gain("relu"))
        else:
            self.register_parameter("loop_weight", None)
        self.layer_norm_weight = F.nn.LayerNorm(self.out_feat, elementwise_affine=True) if layer_norm else None
        self.activation = activation
        self.dropout = F.nn.Dropout(dropout)

    def _coeff(self):
        return self.linear_r.coeff if self.regularizer == "basis" else self._identity

    def _layer_norm(self, h):
        ln = self.layer_norm_weight         # fp32 parameters under bf16 activations: cast like every other weight of the layer
        return F.nn.functional.layer_norm(h, ln.normalized_shape, ln.weight.to(h.dtype), ln.bias.to(h.dtype), ln.eps)

    def typed_edges(self, graph, etypes, norm=None):
        """The checked, cached form of (etypes, norm) for `graph`: build it once and pass it in place of etypes."""
        return TypedEdges(as_csr_graph(graph), etypes, self.num_rels, norm)

    def forward(self, graph, feat, etypes, norm=None, *, presorted=False):
        graph = as_csr_graph(graph)
        if isinstance(etypes, TypedEdges):
            edges = etypes
            if norm is not None:
                raise ValueError("norm travels inside the TypedEdges; pass one or the other")
            if edges.num_rels != self.num_rels:
                raise ValueError("the TypedEdges have %d edge types, the layer %d" % (edges.num_rels, self.num_rels))
        else:
            edges = TypedEdges(graph, etypes, self.num_rels, norm)
        if feat.dim() != 2 or feat.shape[1] != self.in_feat or feat.shape[0] != graph.n_cols:
            raise ValueError("feat must be [n_src = %d, in_feat = %d], got %s" % (graph.n_cols, self.in_feat, tuple(feat.shape)))
        if graph.n_rows > graph.n_cols:
            raise ValueError("a block's destinations must come first among its sources (n_dst <= n_src)")
        B, fin, coeff, W = self.num_bases, self.in_feat, self._coeff(), self.linear_r.W
        feat_dst = feat if graph.n_rows == graph.n_cols else feat[:graph.n_rows]
        relu = _is_relu(self.activation)
        fused_act = False
        if feat.is_cuda:
            epv = 16 // feat.element_size()
            fin_pad = -(-fin // epv) * epv
            if fin_pad != fin:      # zero columns on x, zero rows behind every basis block of the stacked weight
                x = F.nn.functional.pad(feat, (0, fin_pad - fin))
                vstack = F.cat([W, W.new_zeros((B, fin_pad - fin, self.out_feat))], dim=1).reshape(B * fin_pad, self.out_feat)
            else:
                x, vstack = feat, W.reshape(B * fin, self.out_feat)
            z = ops_typed.typed_spmm(graph, edges, x, coeff)
            one_launch = self.loop_weight is not None and self.layer_norm_weight is None and (self.activation is None or relu) \
                and not (relu and self.h_bias is not None)
            if one_launch:          # Z . Vstack + x_i . loop_weight (and the ReLU) in one dense launch
                h = dense.sage_transform(feat_dst, z, self.loop_weight, vstack, relu)
                fused_act = relu
                if self.h_bias is not None:
                    h = h + self.h_bias.to(h.dtype)
            else:
                h = dense.linear(z, vstack)
                if self.layer_norm_weight is not None:
                    h = self._layer_norm(h)
                if self.h_bias is not None:
                    h = h + self.h_bias.to(h.dtype)
                if self.loop_weight is not None:
                    h = h + dense.linear(feat_dst, self.loop_weight)
        else:
            h = _host_aggregate(graph, edges, feat, coeff) @ W.reshape(B * fin, self.out_feat).to(feat.dtype)
            if self.layer_norm_weight is not None:
                h = self._layer_norm(h)
            if self.h_bias is not None:
                h = h + self.h_bias.to(h.dtype)
            if self.loop_weight is not None:
                h = h + feat_dst @ self.loop_weight.to(feat.dtype)
        if self.activation is not None and not fused_act:
            h = self.activation(h)
        return self.dropout(h)

    def extra_repr(self):
        return "%d -> %d, %d edge types, %s" % (self.in_feat, self.out_feat, self.num_rels,
                                                "%d bases" % self.num_bases if self.regularizer == "basis" else "a matrix per type")


class RGCN(F.nn.Module):
    """The entity-classification model of DGL's R-GCN example: basis layers, ReLU between them, none after the last.
    forward(graph, feat, etypes, norm=None) -> logits [n_dst, n_classes]; etypes may be a TypedEdges.  The checked, cached TypedEdges
    of (graph, etypes, norm) are built once and reused while the same tensors come back."""

    def __init__(self, in_feat, hidden, n_classes, num_rels, num_bases, n_layers=2, dropout=0.0):
        super().__init__()
        if n_layers < 1:
            raise ValueError("n_layers must be >= 1")
        widths = [in_feat] + [hidden] * (n_layers - 1) + [n_classes]
        self.layers = F.nn.ModuleList(
            RelGraphConv(widths[k], widths[k + 1], num_rels, regularizer="basis", num_bases=num_bases,
                         activation=F.nn.functional.relu if k < n_layers - 1 else None, dropout=dropout if k < n_layers - 1 else 0.0)
            for k in range(n_layers))
        self.num_rels = int(num_rels)
        self._edges = None      # (key, TypedEdges)

    def _layer_norm(self, h):
        ln = self.layer_norm_weight         # fp32 parameters under bf16 activations: cast like every other weight of the layer
        return F.nn.functional.layer_norm(h, ln.normalized_shape, ln.weight.to(h.dtype), ln.bias.to(h.dtype), ln.eps)

    def typed_edges(self, graph, etypes, norm=None):
        if isinstance(etypes, TypedEdges):
            return etypes
        key = (id(graph), etypes.data_ptr(), etypes._version, None if norm is None else (norm.data_ptr(), norm._version))
        if self._edges is None or self._edges[0] != key:
            self._edges = (key, TypedEdges(graph, etypes, self.num_rels, norm))
        return self._edges[1]

    def forward(self, graph, feat, etypes, norm=None):
        graph = as_csr_graph(graph)
        edges = self.typed_edges(graph, etypes, norm)
        h = feat
        for layer in self.layers:
            h = layer(graph, h, edges)
        return h
