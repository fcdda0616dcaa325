"""Graph transformer layer (PyG's TransformerConv, "Masked Label Prediction: Unified Message Passing Model", UniMP: argument names,
parameter names and shapes) on the gfx950 aggregation engine.

    TransformerConv(in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None, bias=True, root_weight=True)
    GraphTransformer(nfeat, nhid, nclass, heads, layer="transformer" | "dotgat", beta=False)     the two-layer model of the example

Per head, over the entries j of row i of the graph (a CSRGraph [n_dst x n_src], anything as_csr_graph takes; rectangular blocks of
NeighborSampler allowed; edge values are ignored):

    q = lin_query(x_dst)   k = lin_key(x_src)   v = lin_value(x_src)
    alpha = softmax_j(<q_i, k_j> / sqrt(out_channels))   out_i = sum_j alpha_ij v_j

then the heads are concatenated ([n, heads * out_channels]) or averaged (concat=False: [n, out_channels]), and with root_weight
x_r = lin_skip(x_dst) is added -- or, with beta, gated in:  b = sigmoid(lin_beta([x_r, out, out - x_r])),  out = b x_r + (1 - b) out.
A row without entries aggregates 0.

On the GPU the projections run on the dense transform path (dense.linear) and everything per edge is ONE autograd node over three
fused gather passes (ops_attn.sparse_attention): no [nnz, heads] tensor exists.  Heads whose width is not a whole number of
16-byte vectors are padded with zero rows in the WEIGHTS (and biases) and unpadded after the aggregation; the scale stays that of
the true head width.  Host tensors take the torch segment-op path of dotgatconv._host_aggregate.

Not built: attention dropout inside the gather kernels (dropout != 0 raises, as GATv2Conv.attn_drop does) and edge features
(edge_dim is not None raises: they would need an [nnz, heads * out_channels] tensor).  A layer that needs something per edge can be
written on the general path, dgll_amd.ops_mp (u_dot_v, u_add_v, edge_softmax, u_mul_e_sum, copy_e_sum: per-edge tensors with
autograd), which pays [nnz, heads] fp32 per tensor for it.
"""
from ... import backend as F
from ... import dense, ops, ops_attn
from ...graph import as_csr_graph
from .dotgatconv import DotGatConv, _host_aggregate, _project, _split_feat
from .gatconv import _unpad_heads


class TransformerConv(F.nn.Module):
    """PyG's TransformerConv.  forward(graph, feat) -> [n_dst, heads * out_channels] (concat) or [n_dst, out_channels]; feat: a
    tensor, or (feat_src, feat_dst) for blocks."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None, bias=True,
                 root_weight=True):
        super().__init__()
        if float(dropout) != 0.0:
            raise ValueError("TransformerConv: dropout=%r -- in-kernel attention dropout for the dot-product passes is not built "
                             "(dropout must be 0.0)" % (dropout,))
        if edge_dim is not None:
            raise ValueError("TransformerConv: edge_dim=%r -- edge features are not built (they need an [nnz, heads * out_channels] "
                             "tensor; edge_dim must be None)" % (edge_dim,))
        self.in_channels, self.out_channels, self.heads = in_channels, int(out_channels), int(heads)
        self.concat, self.beta, self.root_weight = bool(concat), bool(beta) and bool(root_weight), bool(root_weight)
        self.dropout, self.edge_dim = 0.0, None
        in_src, in_dst = in_channels if isinstance(in_channels, (tuple, list)) else (in_channels, in_channels)
        width = self.heads * self.out_channels
        self.lin_key = F.nn.Linear(in_src, width)
        self.lin_query = F.nn.Linear(in_dst, width)
        self.lin_value = F.nn.Linear(in_src, width)
        self.lin_skip = self.lin_beta = None
        if self.root_weight:
            skip = width if self.concat else self.out_channels
            self.lin_skip = F.nn.Linear(in_dst, skip, bias=bias)
            if self.beta:
                self.lin_beta = F.nn.Linear(3 * skip, 1, bias=False)

    def reset_parameters(self):
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip, self.lin_beta):
            if lin is not None:
                lin.reset_parameters()

    def forward(self, graph, feat):
        graph = as_csr_graph(graph)
        heads, fo = self.heads, self.out_channels
        x_src, x_dst = _split_feat(graph, feat)
        cuda = x_src.is_cuda
        fo_pad = ops.head_width_padded(fo, x_src.dtype, pow2=False) if cuda else fo
        scale = float(fo) ** -0.5                   # of the true head width: the padding columns are zeros and add nothing to <q, k>
        q = _project(self.lin_query, x_dst, heads, fo, fo_pad)
        k = _project(self.lin_key, x_src, heads, fo, fo_pad)
        v = _project(self.lin_value, x_src, heads, fo, fo_pad)
        if cuda:
            out = ops_attn.sparse_attention(graph, q, k, v, heads, scale)
            out = _unpad_heads(out, heads, fo, fo_pad).reshape(graph.n_rows, heads, fo)
        else:
            out = _host_aggregate(graph, q.view(-1, heads, fo), k.view(-1, heads, fo), v.view(-1, heads, fo), scale)
        out = out.reshape(graph.n_rows, heads * fo) if self.concat else out.mean(1)
        if self.root_weight:
            if cuda:
                x_r = dense.linear(x_dst, self.lin_skip.weight.t())
                if self.lin_skip.bias is not None:
                    x_r = x_r + self.lin_skip.bias.to(x_r.dtype)
            else:
                x_r = self.lin_skip(x_dst)
            if self.lin_beta is not None:
                gate_in = F.cat([x_r, out, out - x_r], dim=-1)
                b = F.sigmoid(gate_in @ self.lin_beta.weight.t().to(gate_in.dtype))     # one output column: a matrix-vector product
                out = b * x_r + (1 - b) * out
            else:
                out = out + x_r
        return out

    def extra_repr(self):
        return "%s -> %d x %d%s%s" % (self.in_channels, self.heads, self.out_channels, "" if self.concat else ", head mean",
                                      ", beta" if self.lin_beta is not None else "")


class GraphTransformer(F.nn.Module):
    """The transformer example's two-layer model: heads concatenated after the first layer with ELU, one head on the output layer.
    layer: "transformer" (TransformerConv, skip connections) or "dotgat" (DotGatConv).  forward(graph, x) -> logits [N, nclass]."""

    def __init__(self, nfeat, nhid, nclass, heads, layer="transformer", beta=False):
        super().__init__()
        if layer not in ("transformer", "dotgat"):
            raise ValueError("layer must be 'transformer' or 'dotgat', got %r" % (layer,))
        self.kind = layer
        if layer == "transformer":
            self.layer1 = TransformerConv(nfeat, nhid, heads=heads, beta=beta)
            self.layer2 = TransformerConv(nhid * heads, nclass, heads=1, beta=beta)
        else:
            self.layer1 = DotGatConv(nfeat, nhid, heads)
            self.layer2 = DotGatConv(nhid * heads, nclass, 1)

    def forward(self, graph, x):
        graph = as_csr_graph(graph)
        h = F.nn.functional.elu(self.layer1(graph, x).flatten(1))
        return self.layer2(graph, h).flatten(1)
