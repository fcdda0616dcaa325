"""EdgeConv and Dynamic Graph CNN (Wang et al., "Dynamic Graph CNN for Learning on Point Clouds"; DGL's dgl.nn.EdgeConv with
dgl.nn.KNNGraph / SegmentedKNNGraph) on the HIP engine.

    EdgeConv(in_feat, out_feat, batch_norm=False, allow_zero_in_degree=False)     forward(graph, feat) -> [n_dst, out_feat]
    DGCNN(in_dim, hidden=(64, 64, 128, 256), k=20, emb=1024, n_classes=40)        forward(x [B, N, in_dim]) or forward(x [N, in_dim], segs)

DGL computes h_i = max_j theta(h_j - h_i) + phi(h_i) with one message per edge.  theta is linear, so the max splits:

    out_i = max_j (h_j W_theta^T) + h_i (W_phi - W_theta)^T + b_theta + b_phi

ONE dense product of h with the stacked weight [W_theta | W_phi - W_theta] (dense.linear), ops.segment_max over its first half, one
add of the second half and the two biases.  No [nnz, out] message tensor exists, and the gradients come through the two existing ops
(segment_max sends a row's gradient to its arg-max source).  Each half of the stacked weight is padded with zero columns to a whole
number of 16-byte vectors, so the first half is gathered as it lies.  `feat` is a tensor or a pair (h_src, h_dst) for sampler blocks,
as in DGL; a pair of two different tensors takes one product each.  A row without entries raises unless allow_zero_in_degree; it then
gives phi(h_i) + b_theta: the max over nothing counts as 0 (what segment_max returns there), and the row's own -h_i W_theta^T is
taken back.  A graph from knn_graph carries its smallest degree, so the check reads nothing back; any other graph is checked once
(cached on it).

batch_norm=True raises NotImplementedError: DGL's norm acts on the per-edge message theta(h_j - h_i) + phi(h_i) BEFORE the max, its
statistics run over all edges, and a negative learned scale turns the max into a min -- none of which survives the split above.
DGCNN applies BatchNorm1d to the node rows after the layer instead.
"""
from ... import backend as F
from ... import dense, ops
from ...graph import as_csr_graph
from ...knn import knn_graph
from ..GlobalPooling.Pooling import Pooling
from .dotgatconv import _split_feat


def _pad8(n):
    return -(-n // 8) * 8


class EdgeConv(F.nn.Module):
    """DGL's EdgeConv.  forward(graph, feat) -> [n_dst, out_feat]; feat: a tensor, or (feat_src, feat_dst) for blocks."""

    def __init__(self, in_feat, out_feat, batch_norm=False, allow_zero_in_degree=False):
        super().__init__()
        if batch_norm:
            raise NotImplementedError("EdgeConv: batch_norm=True is not built: the norm acts on the per-edge message before the max (its "
                                      "statistics run over all edges and a negative scale turns the max into a min), which the split "
                                      "max_j (h_j W_theta^T) + h_i (W_phi - W_theta)^T cannot express; normalise the node rows after the "
                                      "layer, as nn.DGCNN does")
        self._in_feat, self._out_feat = int(in_feat), int(out_feat)
        self._allow_zero_in_degree = allow_zero_in_degree
        self.batch_norm = False
        self.theta = F.nn.Linear(self._in_feat, self._out_feat)
        self.phi = F.nn.Linear(self._in_feat, self._out_feat)

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def forward(self, graph, feat):
        graph = as_csr_graph(graph)
        h_src, h_dst = _split_feat(graph, feat)
        if h_src.dim() != 2 or h_src.shape[1] != self._in_feat or h_dst.shape[1] != self._in_feat:
            raise ValueError("EdgeConv: features must be [n_src, %d] and [n_dst, %d], got %s and %s"
                             % (self._in_feat, self._in_feat, tuple(h_src.shape), tuple(h_dst.shape)))
        low = getattr(graph, "min_degree", None)
        if low is None and graph.n_rows:
            low = graph.min_degree = int(graph.degrees().min())
        if low == 0 and not self._allow_zero_in_degree:
            raise ValueError("EdgeConv: the graph has rows without entries (their output is phi(h_i) plus the biases); add self-loops "
                             "or pass allow_zero_in_degree=True")
        fo, half = self._out_feat, _pad8(self._out_feat)
        wt, wp = self.theta.weight, self.phi.weight                                # [out, in]
        zeros = wt.new_zeros((self._in_feat, half - fo))
        w_src = F.cat([wt.t(), zeros], dim=1)                                       # [in, half]
        w_dst = F.cat([(wp - wt).t(), zeros], dim=1)
        if h_src is h_dst:
            z = dense.linear(h_src, F.cat([w_src, w_dst], dim=1))                  # [n, 2 half]: {h W_theta^T | h (W_phi - W_theta)^T}
            z_src, z_dst, own = z[:, :half], z[:, half:half + fo], z[:, :fo]
        else:
            z_src, z_dst, own = dense.linear(h_src, w_src), dense.linear(h_dst, w_dst)[:, :fo], None
        out = ops.segment_max(graph, z_src)[:, :fo] + z_dst
        if low == 0:                    # a row without entries: the max counts as 0, and its own -h_i W_theta^T is taken back
            if own is None:
                own = dense.linear(h_dst, w_src)[:, :fo]
            out = out + own * (graph.degrees() == 0).unsqueeze(1).to(own.dtype)
        return out + (self.theta.bias + self.phi.bias).to(out.dtype)

    def extra_repr(self):
        return "%d -> %d" % (self._in_feat, self._out_feat)


class DGCNN(F.nn.Module):
    """Dynamic Graph CNN for point-cloud classification.  Each layer: knn_graph on the CURRENT features, segmented by cloud, EdgeConv,
    BatchNorm1d on the node rows, LeakyReLU(0.2).  Then the concatenation of all layer outputs, a Linear to `emb`, max and mean
    pooling per cloud (nn.GlobalPooling.Pooling), and a two-layer classifier.  forward(x [B, N, in_dim]) or forward(x [N, in_dim],
    segs) with the clouds' sizes -> logits [B, n_classes].  bf16 points keep the layers' activations in bf16 (fp32 parameters); the
    read-out runs in the parameters' dtype."""

    def __init__(self, in_dim, hidden=(64, 64, 128, 256), k=20, emb=1024, n_classes=40, dropout=0.5):
        super().__init__()
        widths = [int(in_dim)] + [int(h) for h in hidden]
        self.k = int(k)
        self.convs = F.nn.ModuleList(EdgeConv(widths[i], widths[i + 1]) for i in range(len(hidden)))
        self.norms = F.nn.ModuleList(F.nn.BatchNorm1d(widths[i + 1]) for i in range(len(hidden)))
        self.proj = F.nn.Linear(sum(widths[1:]), int(emb))
        self.pool = Pooling(["max", "mean"])
        self.classifier = F.nn.Sequential(F.nn.Linear(2 * int(emb), int(emb) // 2), F.nn.LeakyReLU(0.2), F.nn.Dropout(dropout),
                                          F.nn.Linear(int(emb) // 2, int(n_classes)))

    def forward(self, x, segs=None):
        if isinstance(x, (tuple, list)):
            x, segs = x
        if x.dim() == 3:
            if segs is not None:
                raise ValueError("DGCNN: a [B, N, D] input is already segmented; segs must be None")
            segs = [x.shape[1]] * x.shape[0]
            x = x.reshape(-1, x.shape[-1])
        elif segs is None:
            segs = [x.shape[0]]
        elif not isinstance(segs, (list, tuple)):
            segs = [int(s) for s in segs.tolist()]
        if min(segs) < 1:
            raise ValueError("DGCNN: every cloud needs at least one point")
        sizes = F.tensor(segs, dtype=F.int64)
        batch = F.repeat_interleave(F.arange(len(segs)), sizes).to(x.device)
        h, outs = x, []
        for conv, norm in zip(self.convs, self.norms):
            graph = knn_graph(h, self.k, segs)
            h = F.nn.functional.leaky_relu(norm(conv(graph, h)), 0.2)
            outs.append(h)
        h = F.cat(outs, dim=1).to(self.proj.weight.dtype)
        h = F.nn.functional.leaky_relu(self.proj(h), 0.2)
        return self.classifier(self.pool(h, batch, len(segs)))
