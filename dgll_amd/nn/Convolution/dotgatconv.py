"""Dot-product graph attention layer (DGL's DotGatConv: argument names, parameter names and shapes) on the gfx950 aggregation engine.

    DotGatConv(in_feats, out_feats, num_heads, allow_zero_in_degree=True)

Per head, over the entries j of row i of the graph (a CSRGraph [n_dst x n_src], anything as_csr_graph takes; rectangular blocks of
NeighborSampler allowed; edge values are ignored):

    q = fc(h_dst)   k = v = fc(h_src)   alpha = softmax_j(<q_i, k_j> / sqrt(out_feats))   out_i = sum_j alpha_ij v_j

One bias-free `fc`, or `fc_src` / `fc_dst` for a pair of input widths.  A row without entries gives 0 (allow_zero_in_degree=False
raises for one instead, as DGL does).

On the GPU the products run on the dense transform path (dense.linear) and everything per edge is ONE autograd node over three
fused gather passes (ops_attn.sparse_attention, k and v one buffer: one gather per edge): no [nnz, heads] tensor exists.  Heads
whose width is not a whole number of 16-byte vectors are padded with zero rows in the WEIGHTS and unpadded after the aggregation;
the scale stays that of the true head width.  Host tensors take `_host_aggregate`, the same semantics with torch's segment ops, so
that the layer's own logic can be exercised without a GPU; a GPU tensor never reaches it.

get_attention=True raises NotImplementedError: the attention weights are never formed per edge.  Where they are wanted, the general
path forms them: dgll_amd.ops_mp (`edge_softmax(graph, scale * u_dot_v(graph, k, q, heads))`, then `u_mul_e_sum`), at the price of
[nnz, heads] fp32 tensors.
"""
from ... import backend as F
from ... import dense, ops, ops_attn
from ...graph import as_csr_graph
from .gatconv import _unpad_heads
from .gatv2conv import _pad_head_rows


def _host_aggregate(graph, q, k, v, scale):
    """[n_dst, heads, D] from q [n_dst, heads, D], k and v [n_src, heads, D] with per-edge tensors (host tensors only)."""
    row, col = graph.row_index(), graph.col.long()
    n = graph.n_rows
    s = (q[row] * k[col]).sum(-1) * scale                                                              # [nnz, heads]
    top = F.full((n, s.shape[1]), -float("inf"), dtype=s.dtype).scatter_reduce(0, row.unsqueeze(1).expand_as(s), s.detach(), "amax")
    w = F.exp(s - top[row])
    den = F.zeros(n, s.shape[1], dtype=s.dtype).index_add_(0, row, w)
    alpha = w / den[row]
    return F.zeros(n, v.shape[1], v.shape[2], dtype=v.dtype).index_add_(0, row, alpha.unsqueeze(-1) * v[col])


def _project(fc, h, heads, fo, fo_pad):
    """fc(h) as [n, heads * fo_pad]: on the GPU through the dense transform path, padding applied to the weights."""
    if not h.is_cuda:
        return fc(h)
    out = dense.linear(h, _pad_head_rows(fc.weight, heads, fo, fo_pad).t())
    if fc.bias is not None:
        out = out + _pad_head_rows(fc.bias, heads, fo, fo_pad).to(out.dtype)
    return out


def _split_feat(graph, feat):
    """(h_src, h_dst) of forward(graph, feat): a tensor (a block's destinations come first) or a (feat_src, feat_dst) pair."""
    if isinstance(feat, (tuple, list)):
        h_src, h_dst = feat[0], feat[1]
    else:
        h_src = feat
        h_dst = h_src if graph.n_rows == graph.n_cols else h_src[:graph.n_rows]
    if h_src.shape[0] != graph.n_cols or h_dst.shape[0] != graph.n_rows:
        raise ValueError("features of %d sources and %d destinations for a graph of %d x %d"
                         % (h_src.shape[0], h_dst.shape[0], graph.n_cols, graph.n_rows))
    return h_src, h_dst


class DotGatConv(F.nn.Module):
    """DGL's DotGatConv.  forward(graph, feat) -> [n_dst, num_heads, out_feats]; feat: a tensor, or (feat_src, feat_dst) for blocks."""

    def __init__(self, in_feats, out_feats, num_heads, allow_zero_in_degree=True):
        super().__init__()
        pair = isinstance(in_feats, (tuple, list))
        self._in_src_feats, self._in_dst_feats = in_feats if pair else (in_feats, in_feats)
        self._out_feats, self._num_heads = int(out_feats), int(num_heads)
        self._allow_zero_in_degree = allow_zero_in_degree
        width = self._out_feats * self._num_heads
        if pair:
            self.fc_src = F.nn.Linear(self._in_src_feats, width, bias=False)
            self.fc_dst = F.nn.Linear(self._in_dst_feats, width, bias=False)
        else:
            self.fc = F.nn.Linear(self._in_src_feats, width, bias=False)

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def forward(self, graph, feat, get_attention=False):
        if get_attention:
            raise NotImplementedError("DotGatConv: get_attention=True needs per-edge output, which the fused passes never form")
        graph = as_csr_graph(graph)
        heads, fo = self._num_heads, self._out_feats
        h_src, h_dst = _split_feat(graph, feat)
        if not self._allow_zero_in_degree and bool((graph.degrees() == 0).any()):
            raise ValueError("DotGatConv: the graph has rows without entries (their output is 0); add self-loops or pass "
                             "allow_zero_in_degree=True")
        cuda = h_src.is_cuda
        fo_pad = ops.head_width_padded(fo, h_src.dtype, pow2=False) if cuda else fo
        scale = float(fo) ** -0.5                   # of the true head width: the padding columns are zeros and add nothing to <q, k>
        if hasattr(self, "fc"):
            k = _project(self.fc, h_src, heads, fo, fo_pad)
            if h_dst is h_src:
                q = k
            elif not isinstance(feat, (tuple, list)):
                q = k[:graph.n_rows]                # a block: the destinations are the first sources
            else:
                q = _project(self.fc, h_dst, heads, fo, fo_pad)
        else:
            k = _project(self.fc_src, h_src, heads, fo, fo_pad)
            q = _project(self.fc_dst, h_dst, heads, fo, fo_pad)
        if cuda:
            out = ops_attn.sparse_attention(graph, q, k, k, heads, scale)
            return _unpad_heads(out, heads, fo, fo_pad).reshape(graph.n_rows, heads, fo)
        kh = k.view(-1, heads, fo)
        return _host_aggregate(graph, q.view(-1, heads, fo), kh, kh, scale)

    def extra_repr(self):
        return "%d -> %d x %d" % (self._in_src_feats, self._num_heads, self._out_feats)
