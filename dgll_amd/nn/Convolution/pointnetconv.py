"""PointNetConv, the set abstraction of PointNet++ and a small PointNet++ classifier (Qi et al., "PointNet++: Deep Hierarchical
Feature Learning on Point Sets in a Metric Space"; PyG's PointNetConv with fps and radius) on the HIP engine.

    PointNetConv(local_nn, global_nn=None, allow_zero_in_degree=False)      forward(graph, x, pos) -> [n_dst, F]
    SetAbstraction(ratio, r, max_num_neighbors, local_nn, global_nn=None)   forward(x, pos, segs) -> (x', pos', segs')
    PointNet2(in_dim, n_classes, ...)                                       forward(x [B, N, 3 + in_dim]) or forward((x, pos, segs))

PyG computes out_i = global_nn(max_j local_nn(cat(x_j, pos_j - pos_i))) with one message per edge.  The built case is local_nn a
Linear(C + D, F), or Sequential(Linear, ReLU): the Linear splits over the concatenation, its position part over the difference, and
ReLU is monotone, so max_j relu(a_j) = relu(max_j a_j) exactly:

    out_i = global_nn(relu(max_j (x_j W_x^T + pos_j W_p^T) - pos_i W_p^T + b))

One dense.linear per side, ops.segment_max, one add: no [nnz, F] tensor exists, and the gradients come through the two existing ops
(segment_max sends a row's gradient to its arg-max source).  The module holds the user's own local_nn and global_nn, so state_dict()
has PyG's keys.  Any other local_nn raises NotImplementedError: a deeper per-edge MLP IS a [nnz, F] computation, which is not built
(DESIGN section 9).  `x` and `pos` are tensors or (src, dst) pairs; a single tensor on a bipartite graph stands for the sources, and
its first n_dst rows for the destinations, as for blocks.  x may be None (positions only).  add_self_loops is not offered: a centroid
taken from the cloud lies in its own ball.  A row without entries raises unless allow_zero_in_degree (EdgeConv's rule; the max over
nothing counts as 0); a graph from points.radius does not know its smallest degree, so it is read once and cached on the graph
(SetAbstraction too: a centroid lies in its own ball, but one with a NaN coordinate does not, and then the layer raises).
"""
from ... import backend as F
from ... import dense, ops, points
from ...graph import as_csr_graph
from ..GlobalPooling.Pooling import Pooling
from .dotgatconv import _split_feat
from .edgeconv import _pad8


def _linear_of(local_nn):
    """(Linear, relu?) of a local_nn the split can express, else NotImplementedError"""
    if isinstance(local_nn, F.nn.Linear):
        return local_nn, False
    if isinstance(local_nn, F.nn.Sequential) and len(local_nn) in (1, 2) and isinstance(local_nn[0], F.nn.Linear) \
            and (len(local_nn) == 1 or isinstance(local_nn[1], F.nn.ReLU)):
        return local_nn[0], len(local_nn) == 2
    raise NotImplementedError("PointNetConv: local_nn must be a Linear or Sequential(Linear, ReLU): the max over the neighbours is taken "
                              "of the Linear's node-wise products, max_j (x_j W_x^T + pos_j W_p^T) - pos_i W_p^T + b.  A deeper per-edge "
                              "MLP needs the [nnz, F] messages, which is not built; put the further layers into global_nn")


class PointNetConv(F.nn.Module):
    """PyG's PointNetConv.  forward(graph, x, pos) -> [n_dst, F]; x: None, a tensor or (x_src, x_dst); pos: a tensor or (src, dst)."""

    def __init__(self, local_nn, global_nn=None, allow_zero_in_degree=False):
        super().__init__()
        _linear_of(local_nn)
        self.local_nn, self.global_nn = local_nn, global_nn
        self._allow_zero_in_degree = allow_zero_in_degree

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def forward(self, graph, x, pos):
        graph = as_csr_graph(graph)
        lin, relu = _linear_of(self.local_nn)
        p_src, p_dst = _split_feat(graph, pos)
        D = p_src.shape[1]
        x_src = None if x is None else _split_feat(graph, x)[0]
        C = 0 if x_src is None else x_src.shape[1]
        if p_dst.shape[1] != D or C + D != lin.in_features:
            raise ValueError("PointNetConv: local_nn takes %d columns, got x of %d and pos of %d" % (lin.in_features, C, D))
        low = getattr(graph, "min_degree", None)
        if low is None and graph.n_rows:
            low = graph.min_degree = int(graph.degrees().min())
        if low == 0 and not self._allow_zero_in_degree:
            raise ValueError("PointNetConv: the graph has rows without entries (their output is -pos_i W_p^T plus the bias); use a "
                             "larger radius or pass allow_zero_in_degree=True")
        fo, half = lin.out_features, _pad8(lin.out_features)
        w = F.cat([lin.weight.t(), lin.weight.new_zeros((C + D, half - fo))], dim=1)          # [C + D, half]; the rows of W_p last
        h_src = p_src if x_src is None else F.cat([x_src, p_src.to(x_src.dtype)], dim=1)
        z_src = dense.linear(h_src, w)                                                          # x_j W_x^T + pos_j W_p^T
        z_dst = dense.linear(p_dst.to(h_src.dtype), w[C:])[:, :fo]                              # pos_i W_p^T
        out = ops.segment_max(graph, z_src)[:, :fo] - z_dst
        if lin.bias is not None:
            out = out + lin.bias.to(out.dtype)
        if relu:
            out = F.relu(out)
        return out if self.global_nn is None else self.global_nn(out.to(_param_dtype(self.global_nn, out)))


def _param_dtype(module, like):
    for p in module.parameters():
        return p.dtype
    return like.dtype


class SetAbstraction(F.nn.Module):
    """One level of PointNet++: points.fps picks ceil(ratio * size) centroids of every cloud, points.radius groups the first
    max_num_neighbors points within r of each, PointNetConv reduces each group.  forward(x, pos, segs) -> (x', pos', segs'):
    x [N, C] or None, pos [N, D], segs the clouds' sizes; x' [M, F], pos' [M, D] the centroids, segs' their number per cloud."""

    def __init__(self, ratio, r, max_num_neighbors, local_nn, global_nn=None):
        super().__init__()
        self.ratio, self.r, self.max_num_neighbors = float(ratio), float(r), int(max_num_neighbors)
        self.conv = PointNetConv(local_nn, global_nn)

    def forward(self, x, pos, segs):
        idx = points.fps(pos, segs, ratio=self.ratio)
        centres = pos[idx]
        graph = points.radius(pos, centres, self.r, segs, idx.seg_sizes, max_num_neighbors=self.max_num_neighbors)
        return self.conv(graph, x, (pos, centres)), centres, idx.seg_sizes


class PointNet2(F.nn.Module):
    """PointNet++ for point-cloud classification (single-scale grouping): two SetAbstraction levels, a global stage (Linear + ReLU on
    cat(x, pos), max over each cloud) and a two-layer classifier.  forward(x [B, N, 3 + in_dim]) -- the first three columns are the
    positions -- or forward((x [N, in_dim] or None, pos [N, 3], segs)) for clouds of unequal size -> logits [B, n_classes].  With
    bf16 points the run is MIXED precision: the searches and the first level's products and max run in bf16; every global_nn has fp32
    parameters and returns fp32, so from the first level's output on the features, and with them the second level, are fp32."""

    def __init__(self, in_dim, n_classes, hidden=(64, 128, 256), ratios=(0.5, 0.25), radii=(0.2, 0.4), max_num_neighbors=32,
                 dropout=0.5):
        super().__init__()
        h1, h2, h3 = (int(h) for h in hidden)
        local = lambda i, o: F.nn.Sequential(F.nn.Linear(i, o), F.nn.ReLU())                   # noqa: E731
        globl = lambda o: F.nn.Sequential(F.nn.Linear(o, o), F.nn.ReLU())                      # noqa: E731
        self.in_dim = int(in_dim)
        self.sa1 = SetAbstraction(ratios[0], radii[0], max_num_neighbors, local(self.in_dim + 3, h1), globl(h1))
        self.sa2 = SetAbstraction(ratios[1], radii[1], max_num_neighbors, local(h1 + 3, h2), globl(h2))
        self.global_nn = F.nn.Sequential(F.nn.Linear(h2 + 3, h3), F.nn.ReLU())
        self.pool = Pooling("max")
        self.classifier = F.nn.Sequential(F.nn.Linear(h3, h3 // 2), F.nn.ReLU(), F.nn.Dropout(dropout), F.nn.Linear(h3 // 2, int(n_classes)))

    def forward(self, x, pos=None, segs=None):
        if isinstance(x, (tuple, list)):
            x, pos, segs = x
        elif pos is None:
            if x.dim() != 3 or x.shape[2] != 3 + self.in_dim:
                raise ValueError("PointNet2: a single input must be [B, N, %d] (positions first), got %s" % (3 + self.in_dim, tuple(x.shape)))
            segs = [x.shape[1]] * x.shape[0]
            flat = x.reshape(-1, x.shape[2])
            pos, x = flat[:, :3], (flat[:, 3:] if self.in_dim else None)
        segs = [int(s) for s in (segs.tolist() if hasattr(segs, "tolist") else segs)]
        if min(segs) < 1:
            raise ValueError("PointNet2: every cloud needs at least one point")
        x, pos, segs = self.sa1(x, pos, segs)
        x, pos, segs = self.sa2(x, pos, segs)
        dt = self.global_nn[0].weight.dtype
        h = self.global_nn(F.cat([x.to(dt), pos.to(dt)], dim=1))
        batch = F.repeat_interleave(F.arange(len(segs)), F.tensor(segs, dtype=F.int64)).to(h.device)
        return self.classifier(self.pool(h, batch, len(segs)))
