"""Attention-based graph neural network layer (DGL's AGNNConv, "Attention-based Graph Neural Network for Semi-Supervised Learning":
argument names, parameter name and shape) on the gfx950 aggregation engine.

    AGNNConv(init_beta=1.0, learn_beta=True, allow_zero_in_degree=True)
    AGNN(nfeat, nhid, nclass, n_layers=2)        the paper's model: a linear embedding, attention layers, a linear classifier

Over the entries j of row i of the graph (a CSRGraph [n_dst x n_src], anything as_csr_graph takes; rectangular blocks of
NeighborSampler allowed; edge values are ignored), with one head and no weights but the scalar beta:

    e_ij = beta * cos(h_i, h_j) = beta <h_i / |h_i|, h_j / |h_j|>      P = softmax_j e_ij      out_i = sum_j P_ij h_j

`beta` is a 1-element Parameter, or a buffer of the same name when learn_beta=False (state_dict() has the one key "beta" either
way, as DGL's has).  A row without entries gives 0 (allow_zero_in_degree=False raises for one instead, as DGL does; DGL's default
is False, here it defaults to True as DotGatConv's does).

The learnable scale is why this layer is not ops_attn.sparse_attention, whose scale is a float without a gradient: it is written
with the per-edge operators of dgll_amd.ops_mp -- u_dot_v, edge_softmax, u_mul_e_sum -- and autograd sends the gradient of beta
through the [nnz, 1] logits.  That is the general path and it pays for it: three [nnz, 1] fp32 tensors live until the backward.  A
feature width that is not a whole number of 16-byte vectors is padded with zero columns (they change neither norm nor dot product)
and unpadded after the aggregation; the one head must fit a wavefront's lanes (at most 256 fp32 / 512 bf16 columns: wider
features raise).  Host tensors take `_host_aggregate`, the same semantics with torch's segment ops, so that the
layer's own logic can be exercised without a GPU; a GPU tensor never reaches it.
"""
from ... import backend as F
from ... import dense, ops, ops_mp
from ...graph import as_csr_graph
from .dotgatconv import _split_feat


def _host_aggregate(graph, h_src, h_dst, beta):
    """[n_dst, F] with per-edge tensors (host tensors only)."""
    row, col = graph.row_index(), graph.col.long()
    n = graph.n_rows
    e = beta * (F.nn.functional.normalize(h_src, p=2, dim=-1)[col] * F.nn.functional.normalize(h_dst, p=2, dim=-1)[row]).sum(-1)     # [nnz]
    top = F.full((n,), -float("inf"), dtype=e.dtype).scatter_reduce(0, row, e.detach(), "amax")
    w = F.exp(e - top[row])
    den = F.zeros(n, dtype=e.dtype).index_add_(0, row, w)
    p = w / den[row]
    return F.zeros(n, h_src.shape[1], dtype=h_src.dtype).index_add_(0, row, p.unsqueeze(-1) * h_src[col])


def _unit_rows(h):
    """h / |h| per row in h's dtype; the norm of a bf16 matrix is formed in fp32, so the unit rows are rounded once"""
    if h.dtype == F.float32:
        return F.nn.functional.normalize(h, p=2, dim=-1)
    return F.nn.functional.normalize(h.float(), p=2, dim=-1).to(h.dtype)


def _linear(fc, h):
    """fc(h): on the GPU through the dense transform path (bf16 activations with fp32 parameters included)."""
    if not h.is_cuda:
        return fc(h)
    out = dense.linear(h, fc.weight.t())
    return out if fc.bias is None else out + fc.bias.to(out.dtype)


class AGNNConv(F.nn.Module):
    """DGL's AGNNConv.  forward(graph, feat) -> [n_dst, F]; feat: a tensor [n_src, F], or (feat_src, feat_dst) for blocks."""

    def __init__(self, init_beta=1.0, learn_beta=True, allow_zero_in_degree=True):
        super().__init__()
        self._allow_zero_in_degree = allow_zero_in_degree
        beta = F.tensor([float(init_beta)])
        if learn_beta:
            self.beta = F.nn.Parameter(beta)
        else:
            self.register_buffer("beta", beta)

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def forward(self, graph, feat):
        graph = as_csr_graph(graph)
        h_src, h_dst = _split_feat(graph, feat)
        if not self._allow_zero_in_degree and bool((graph.degrees() == 0).any()):
            raise ValueError("AGNNConv: the graph has rows without entries (their output is 0); add self-loops or pass "
                             "allow_zero_in_degree=True")
        if not h_src.is_cuda:
            return _host_aggregate(graph, h_src, h_dst, self.beta.to(h_src.dtype))
        width = h_src.shape[1]
        pad = ops.head_width_padded(width, h_src.dtype, pow2=False) - width
        if pad:                                     # zero columns: |h| and <h_i, h_j> do not see them
            same = h_dst is h_src
            h_src = F.nn.functional.pad(h_src, (0, pad))
            h_dst = h_src if same else F.nn.functional.pad(h_dst, (0, pad))
        n_src = _unit_rows(h_src)
        n_dst = n_src if h_dst is h_src else _unit_rows(h_dst)
        e = self.beta.float() * ops_mp.u_dot_v(graph, n_src, n_dst, 1)          # [nnz, 1] fp32
        p = ops_mp.edge_softmax(graph, e)
        out = ops_mp.u_mul_e_sum(graph, h_src, p, 1)
        return out[:, :width] if pad else out

    def extra_repr(self):
        return "learn_beta=%s" % isinstance(self.beta, F.nn.Parameter)


class AGNN(F.nn.Module):
    """The paper's model (and DGL's example): h = relu(proj(x)); n_layers AGNNConv, the first with a fixed beta = 1; logits = cls(h).
    forward(graph, x) -> logits [N, nclass]."""

    def __init__(self, nfeat, nhid, nclass, n_layers=2, init_beta=1.0):
        super().__init__()
        self.proj = F.nn.Linear(nfeat, nhid)
        self.layers = F.nn.ModuleList([AGNNConv(init_beta, learn_beta=i > 0) for i in range(n_layers)])
        self.cls = F.nn.Linear(nhid, nclass)

    def forward(self, graph, x):
        graph = as_csr_graph(graph)
        h = F.nn.functional.relu(_linear(self.proj, x))
        for layer in self.layers:
            h = layer(graph, h)
        return _linear(self.cls, h)
