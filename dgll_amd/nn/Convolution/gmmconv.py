"""GMMConv -- the Gaussian-mixture convolution of MoNet (Monti et al., "Geometric deep learning on graphs and manifolds using mixture
model CNNs"), with the argument names, the state dict and the order of operations of DGL's dgl.nn.pytorch.conv.GMMConv.

    GMMConv(in_feats, out_feats, dim, n_kernels, aggregator_type="sum", residual=False, bias=True, allow_zero_in_degree=False)
    forward(graph, feat, pseudo) -> [n_dst, out_feats]      feat: a tensor or (feat_src, feat_dst); pseudo: [nnz, dim], CSR entry order

    w_k(e) = exp(-0.5 * sum_d ((pseudo[e, d] - mu[k, d]) * inv_sigma[k, d])^2)
    out_i  = s_i * sum_{e = (j -> i)} sum_k w_k(e) * (x_j W_k) + res_fc(x_i) + bias          s_i = 1 ("sum") or 1 / deg_i ("mean")

| parameter     | shape                                                    | present                            |
| mu            | [n_kernels, dim]                                         | always                             |
| inv_sigma     | [n_kernels, dim]                                         | always                             |
| fc.weight     | [n_kernels * out, in_src]; W_k = view(K, out, in)[k].T   | always                             |
| res_fc.weight | [out, in_dst]                                            | residual and in_dst != out (else the identity) |
| bias          | [out]                                                    | bias=True                          |

Initialisers as DGL's: fc and res_fc Xavier-normal with the ReLU gain, mu normal(0, 0.1), inv_sigma ones, bias zeros.  DGL is not
installed where this was written and the project this package was modelled on has no MoNet, so there are no recorded DGL outputs
behind it: names and order of operations follow DGL's documented module, and parity is tested against a float64 restatement of the
formulas above (tests/gmm_ref.py).

On the GPU no [nnz, K, out] message exists: the sums are linear, so out = s_i Z . V with Z[i, k, :] = sum_e w_k(e) x_j ONE fused
gather (ops_gmm.gmm_expand: x_j loaded once per entry, the weights computed per entry in registers) and V = stack_k(W_k) one dense
transform of reduction length K * in -- together with res_fc(x_i) in a single launch (dense.sage_transform) when res_fc is a matrix.
An `in` that is not a whole number of 16-byte vectors is padded: zero columns on x, zero rows behind every kernel block of V.  Always
this expand-then-transform order; the project-first order (which would gather less only when in > K * out) is not built, and neither
is aggregator_type="max" (a max over K * out wide messages is not linear and would need it).  A row without entries gives
res_fc(x_i) + bias; allow_zero_in_degree=False raises for one instead, as DGL does.  Host tensors take `_host_aggregate`, the same
semantics with torch index ops; a GPU tensor never reaches it.
"""
from ... import backend as F
from ... import dense, ops_gmm
from ...graph import as_csr_graph
from .dotgatconv import _split_feat


def _host_aggregate(graph, x, pseudo, mu, inv_sigma, reduce):
    """Z [n_dst, K * F] of ops_gmm.gmm_expand with torch index ops (host tensors only)."""
    row, col = graph.row_index(), graph.col.long()
    t = (pseudo.to(x.dtype).unsqueeze(1) - mu.to(x.dtype).unsqueeze(0)) * inv_sigma.to(x.dtype).unsqueeze(0)
    w = F.exp(-0.5 * (t * t).sum(-1))                                               # [nnz, K]
    xs = x[col]
    z = F.cat([F.zeros(graph.n_rows, x.shape[1], dtype=x.dtype).index_add_(0, row, w[:, k:k + 1] * xs) for k in range(mu.shape[0])], dim=1)
    if reduce == "mean":
        z = z / graph.degrees().clamp(min=1).to(x.dtype).unsqueeze(1)
    return z


def degree_pseudo(graph):
    """[nnz, 2] fp32, in CSR entry order: (1 / sqrt(deg_i + 1), 1 / sqrt(deg_j + 1)) for the entry j -> i, deg the number of entries of
    a node's row (a source of a block that is no destination has none) -- the pseudo-coordinates of the citation-graph MoNet."""
    graph = as_csr_graph(graph)
    deg = graph.degrees().to(F.float32)
    if graph.n_cols > graph.n_rows:
        deg = F.cat([deg, deg.new_zeros(graph.n_cols - graph.n_rows)])
    inv = (deg + 1.0).rsqrt()
    return F.stack([inv[graph.row_index()], inv[graph.col.long()]], dim=1)


class GMMConv(F.nn.Module):
    """DGL's GMMConv.  forward(graph, feat, pseudo) -> [n_dst, out_feats]."""

    def __init__(self, in_feats, out_feats, dim, n_kernels, aggregator_type="sum", residual=False, bias=True, allow_zero_in_degree=False):
        super().__init__()
        pair = isinstance(in_feats, (tuple, list))
        self._in_src_feats, self._in_dst_feats = (int(v) for v in (in_feats if pair else (in_feats, in_feats)))
        self._out_feats, self._dim, self._n_kernels = int(out_feats), int(dim), int(n_kernels)
        if aggregator_type == "max":
            raise NotImplementedError('GMMConv: aggregator_type="max" is not built (a max over the K * out wide messages is not linear '
                                      'in them); use "sum" or "mean"')
        if aggregator_type not in ("sum", "mean"):
            raise ValueError('GMMConv: aggregator_type must be "sum", "mean" or "max", got %r' % (aggregator_type,))
        if not 1 <= self._dim <= ops_gmm.MAX_DIM:
            raise ValueError("GMMConv: dim must be in 1..%d, got %d" % (ops_gmm.MAX_DIM, self._dim))
        if not 1 <= self._n_kernels <= ops_gmm.MAX_KERNELS:
            raise ValueError("GMMConv: n_kernels must be in 1..%d, got %d" % (ops_gmm.MAX_KERNELS, self._n_kernels))
        self._reduce = aggregator_type
        self._allow_zero_in_degree = allow_zero_in_degree
        self.mu = F.Parameter(F.empty(self._n_kernels, self._dim))
        self.inv_sigma = F.Parameter(F.empty(self._n_kernels, self._dim))
        self.fc = F.nn.Linear(self._in_src_feats, self._n_kernels * self._out_feats, bias=False)
        if residual:
            if self._in_dst_feats != self._out_feats:
                self.res_fc = F.nn.Linear(self._in_dst_feats, self._out_feats, bias=False)
            else:
                self.res_fc = F.nn.Identity()
        else:
            self.register_buffer("res_fc", None)
        if bias:
            self.bias = F.Parameter(F.empty(self._out_feats))
        else:
            self.register_buffer("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        gain = F.nn.init.calculate_gain("relu")
        F.nn.init.xavier_normal_(self.fc.weight, gain=gain)
        if isinstance(self.res_fc, F.nn.Linear):
            F.nn.init.xavier_normal_(self.res_fc.weight, gain=gain)
        F.nn.init.normal_(self.mu.data, 0, 0.1)
        F.nn.init.constant_(self.inv_sigma.data, 1)
        if self.bias is not None:
            F.nn.init.zeros_(self.bias.data)

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def forward(self, graph, feat, pseudo):
        graph = as_csr_graph(graph)
        K, fin, fo = self._n_kernels, self._in_src_feats, self._out_feats
        h_src, h_dst = _split_feat(graph, feat)
        if h_src.dim() != 2 or h_src.shape[1] != fin or h_dst.shape[1] != self._in_dst_feats:
            raise ValueError("GMMConv: features must be [n_src, %d] and [n_dst, %d], got %s and %s"
                             % (fin, self._in_dst_feats, tuple(h_src.shape), tuple(h_dst.shape)))
        if pseudo.dim() != 2 or tuple(pseudo.shape) != (graph.nnz, self._dim):
            raise ValueError("GMMConv: pseudo must be [nnz = %d, dim = %d] in the graph's entry order, got %s"
                             % (graph.nnz, self._dim, tuple(pseudo.shape)))
        if not self._allow_zero_in_degree and bool((graph.degrees() == 0).any()):
            raise ValueError("GMMConv: the graph has rows without entries (their output is res_fc(x_i) + bias); add self-loops or pass "
                             "allow_zero_in_degree=True")
        W = self.fc.weight.view(K, fo, fin).transpose(1, 2)                         # [K, in, out]: W_k
        res_matrix = isinstance(self.res_fc, F.nn.Linear)
        if h_src.is_cuda:
            epv = 16 // h_src.element_size()
            fin_pad = -(-fin // epv) * epv
            if fin_pad != fin:      # zero columns on x, zero rows behind every kernel block of the stacked weight
                x = F.nn.functional.pad(h_src, (0, fin_pad - fin))
                vstack = F.cat([W, W.new_zeros((K, fin_pad - fin, fo))], dim=1).reshape(K * fin_pad, fo)
            else:
                x, vstack = h_src, W.reshape(K * fin, fo)
            z = ops_gmm.gmm_expand(graph, x, pseudo, self.mu, self.inv_sigma, self._reduce)
            if res_matrix:          # Z . V + x_i . res_fc^T in one dense launch
                h = dense.sage_transform(h_dst, z, self.res_fc.weight.t(), vstack, False)
            else:
                h = dense.linear(z, vstack)
                if self.res_fc is not None:
                    h = h + h_dst
        else:
            h = _host_aggregate(graph, h_src, pseudo, self.mu, self.inv_sigma, self._reduce) @ W.reshape(K * fin, fo).to(h_src.dtype)
            if res_matrix:
                h = h + h_dst @ self.res_fc.weight.t().to(h_dst.dtype)
            elif self.res_fc is not None:
                h = h + h_dst
        if self.bias is not None:
            h = h + self.bias.to(h.dtype)
        return h

    def extra_repr(self):
        return "%d -> %d, %d kernels over %d pseudo-coordinates, %s" % (self._in_src_feats, self._out_feats, self._n_kernels, self._dim,
                                                                     self._reduce)


class MoNet(F.nn.Module):
    """The node-classification MoNet of benchmarking-gnns: n_layers of GMMConv, each with its own pseudo_proj = Linear(2, dim) + Tanh over
    the raw pseudo-coordinates [nnz, 2] (degree_pseudo(graph), or the caller's), ReLU between the layers, none after the last.
    forward(graph, feat, pseudo=None) -> logits [n_dst, n_classes]."""

    def __init__(self, in_feats, hidden, n_classes, dim=2, n_kernels=3, n_layers=2, aggregator_type="sum", residual=False, dropout=0.0):
        super().__init__()
        if n_layers < 1:
            raise ValueError("n_layers must be >= 1")
        widths = [in_feats] + [hidden] * (n_layers - 1) + [n_classes]
        self.layers = F.nn.ModuleList(GMMConv(widths[k], widths[k + 1], dim, n_kernels, aggregator_type, residual=residual,
                                              allow_zero_in_degree=True) for k in range(n_layers))
        self.pseudo_proj = F.nn.ModuleList(F.nn.Sequential(F.nn.Linear(2, dim), F.nn.Tanh()) for _ in range(n_layers))
        self.dropout = F.nn.Dropout(dropout)

    def forward(self, graph, feat, pseudo=None):
        graph = as_csr_graph(graph)
        if pseudo is None:
            pseudo = degree_pseudo(graph)
        if pseudo.dim() != 2 or tuple(pseudo.shape) != (graph.nnz, 2):
            raise ValueError("MoNet: pseudo must be [nnz = %d, 2], got %s" % (graph.nnz, tuple(pseudo.shape)))
        h = feat
        for k, (layer, proj) in enumerate(zip(self.layers, self.pseudo_proj)):
            u = proj(pseudo.to(proj[0].weight.dtype))
            h = layer(graph, h, u)
            if k + 1 < len(self.layers):
                h = self.dropout(F.relu(h))
        return h
