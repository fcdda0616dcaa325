"""Pooling by selection: TopKPooling (Graph U-Nets, Gao & Ji 2019), SAGPooling (Lee et al. 2019) and SortPooling (the read-out of the
DGCNN graph classifier, Zhang et al. 2018; PyG's global_sort_pool / SortAggregation), on the segmented score sort and the scaled gather of
ops_pool (csrc/seg_sort.hip).

TopKPooling and SAGPooling differ only in where the score of a node comes from -- a learned projection x . p / |p|, or a one-output
graph convolution -- and share one forward:

    x_out, graph_out, segs_out, perm, score_kept = layer(graph, x, segs=None, batch=None)

perm holds the ceil(ratio * size) best nodes of every graph, best first (score descending, ties to the smaller index), x_out =
x[perm] * act(score[perm]), graph_out = sampling.subgraph.node_subgraph(graph, perm) (graph=None skips it), segs_out the nodes kept
per graph (a Python list: the next layer's `segs`, no read-back) and score_kept = act(score)[perm].  Gradients reach x and the
score's parameters through the gather's backward.  The projection and the scoring convolution are the torch / HIP code they were
before; the selection, the gather and its backward are the new kernels.

Not built: PyG's min_score / softmax mode and `multiplier`, DGL's per-row feature sort inside SortPooling, edge
pooling, ASAPooling, DiffPool, the partitioned path.
"""
import torch

from ... import ops_pool
from ...sampling.subgraph import node_subgraph
from ..Convolution.gcnconv import gcnConv

_TORCH_ACT = {"none": lambda s: torch.ones_like(s), "identity": lambda s: s, "tanh": torch.tanh, "sigmoid": torch.sigmoid}


class _SelectPooling(torch.nn.Module):
    def __init__(self, in_channels, ratio, nonlinearity):
        super().__init__()
        if not 0.0 < float(ratio) <= 1.0:
            raise ValueError("ratio must be in (0, 1], got %r" % (ratio,))
        if nonlinearity not in _TORCH_ACT:
            raise ValueError("nonlinearity must be one of %s, got %r" % (sorted(_TORCH_ACT), nonlinearity))
        self.in_channels, self.ratio, self.nonlinearity = int(in_channels), float(ratio), nonlinearity

    def score(self, graph, x):
        raise NotImplementedError

    def forward(self, graph, x, segs=None, batch=None):
        score = self.score(graph, x).reshape(-1)
        perm, inv = ops_pool.segment_topk(score, segs, batch, ratio=self.ratio, return_inverse=True)
        x_out = ops_pool.select(x, score, perm, inv, act=self.nonlinearity)
        graph_out = None if graph is None else node_subgraph(graph, perm)
        return x_out, graph_out, perm.seg_sizes, perm, _TORCH_ACT[self.nonlinearity](score)[perm]

    def extra_repr(self):
        return "%d, ratio=%g, nonlinearity=%s" % (self.in_channels, self.ratio, self.nonlinearity)


class TopKPooling(_SelectPooling):
    """score = x . p / |p| with a learned p [in_channels]"""

    def __init__(self, in_channels, ratio=0.5, nonlinearity="tanh"):
        super().__init__(in_channels, ratio, nonlinearity)
        self.p = torch.nn.Parameter(torch.empty(self.in_channels))
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / self.in_channels ** 0.5
        with torch.no_grad():
            self.p.uniform_(-bound, bound)

    def score(self, graph, x):
        p = self.p.to(x.dtype)
        return (x @ p) / p.norm()


class SAGPooling(_SelectPooling):
    """score = gnn(x, graph), a graph convolution with one output channel (default: this project's gcnConv(in_channels, 1))"""

    def __init__(self, in_channels, ratio=0.5, gnn=None, nonlinearity="tanh"):
        super().__init__(in_channels, ratio, nonlinearity)
        self.gnn = gcnConv(self.in_channels, 1) if gnn is None else gnn

    def score(self, graph, x):
        if graph is None:
            raise ValueError("SAGPooling scores the nodes with a graph convolution: it needs the graph")
        return self.gnn(x, graph)


def global_sort_pool(x, segs=None, batch=None, *, k):
    """[B, k * F]: the k nodes of every graph with the largest last channel, in that order, zero rows behind a short graph."""
    return ops_pool.sort_pool(x, segs, batch, k=k)


class SortPooling(torch.nn.Module):
    def __init__(self, k):
        super().__init__()
        if int(k) != k or int(k) < 1:
            raise ValueError("k must be an integer >= 1, got %r" % (k,))
        self.k = int(k)

    def forward(self, x, segs=None, batch=None):
        return ops_pool.sort_pool(x, segs, batch, k=self.k)

    def extra_repr(self):
        return "k=%d" % self.k
