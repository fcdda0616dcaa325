"""k-nearest-neighbour graphs computed from node features on the device (DGL's knn_graph / segmented_knn_graph and the modules
KNNGraph / SegmentedKNNGraph): csrc/knn.hip, one launch, nothing stored per pair of points.

    knn_graph(x, k, segs=None, *, exclude_self=False, dist="euclidean", return_dist=False)  -> CSRGraph  (or (CSRGraph, fp32 [nnz]))
    segmented_knn_graph(x, k, segs)                                                          -> CSRGraph

`x` is [N, D] or DGL's [B, N, D] (B segments of N points, node ids offset by b * N), float32 or bfloat16, 1 <= D <= MAX_D; `segs` is
DGL's list of segment sizes (a Python sequence or an integer tensor that sums to N; None: one segment).  1 <= k <= MAX_K.  Row i of
the result (the destination) lists its neighbours (the sources), as DGL's edges point: the min(k, size - exclude_self) points of its
own segment with the smallest (d, j), in that order, d the fp32 squared Euclidean distance in the difference form; among equal
distances the smaller index wins, and exclude_self skips j == i by index (a duplicate point is still a neighbour).  return_dist also
gives those squared distances.  dist="cosine" normalises the rows and then searches Euclidean, as DGL does.  The graph has
n_rows == n_cols == N, no values and max_degree = k, so CSRGraph.plan() takes its host-only path.  The result is not differentiable
with respect to x, as in DGL.

Rows that are not contiguous go to the kernel through their pitch, without a copy (16-byte loads where ops.pitch16_ok(x), scalar
loads otherwise); only a column stride other than 1 is copied.

EQUAL segments ([B, N, D], or segs all equal, or none): the row pointers and the segment table are cached per (S, size, k,
exclude_self, device); after the first call there is no host synchronisation and no upload, and the call can be captured into a
graph (the tables of the 64 most recent shapes are kept; a captured call goes on reading the tables it was captured with, which
every graph it returned keeps alive).  UNEQUAL segments read `segs` on the host once per call (a tensor on the device synchronises) and upload two small tables.
There is no CPU implementation: a CPU tensor raises.

Not built: k > 64, D > 256, approximate search, knn(x, y) between two point sets, radius graphs.
"""
import torch

from . import _lib
from .graph import CSRGraph
from .ops import _dtype_code, _require_cuda

MAX_K, MAX_D = _lib.KNN_MAX_K, _lib.KNN_MAX_D
QUERY_TILE = _lib.KNN_QUERY_TILE        # rows of one workgroup's tile of queries (one lane each)
CAND_TILE = _lib.KNN_CAND_TILE          # rows of a segment staged in LDS at a time

_tables = {}                            # (S, size, k, exclude_self, device) -> (seg_ptr, out_rowptr, nnz, smallest degree)
_TABLES_KEPT = 64


def _equal_tables(n_segs, size, k, exclude_self, device):
    key = (n_segs, size, k, exclude_self, device)
    hit = _tables.get(key)
    if hit is None:
        deg = min(k, max(size - int(exclude_self), 0))
        n = n_segs * size
        seg_ptr = torch.arange(0, n + 1, max(size, 1), dtype=torch.int64, device=device) if size else \
            torch.zeros(n_segs + 1, dtype=torch.int64, device=device)
        rowptr = torch.arange(0, n * deg + 1, deg, dtype=torch.int64, device=device) if deg else \
            torch.zeros(n + 1, dtype=torch.int64, device=device)
        if len(_tables) >= _TABLES_KEPT:
            _tables.pop(next(iter(_tables)))
        hit = _tables[key] = (seg_ptr, rowptr, n * deg, deg if n else None)
    return hit


def _unequal_tables(sizes, k, exclude_self, device):
    sz = torch.tensor(sizes, dtype=torch.int64)
    seg_ptr = torch.zeros(len(sizes) + 1, dtype=torch.int64)
    torch.cumsum(sz, 0, out=seg_ptr[1:])
    deg = torch.repeat_interleave((sz - int(exclude_self)).clamp(min=0, max=k), sz)
    rowptr = torch.zeros(deg.numel() + 1, dtype=torch.int64)
    torch.cumsum(deg, 0, out=rowptr[1:])
    return seg_ptr.to(device), rowptr.to(device), int(rowptr[-1]), int(deg.min()) if deg.numel() else None


def _segment_sizes(segs, n):
    if isinstance(segs, torch.Tensor):
        if segs.is_floating_point() or segs.dim() != 1:
            raise ValueError("knn_graph: segs must be a 1-D integer tensor or a sequence of segment sizes")
        segs = segs.tolist()
    sizes = [int(s) for s in segs]
    if any(s < 0 for s in sizes) or sum(sizes) != n:
        raise ValueError("knn_graph: the segment sizes must be >= 0 and sum to the number of points %d, got a sum of %d" % (n, sum(sizes)))
    return sizes


def knn_graph(x, k, segs=None, *, exclude_self=False, dist="euclidean", return_dist=False):
    """CSRGraph whose row i lists the k nearest points of i's segment (module docstring); with return_dist also their fp32 squared
    distances [nnz]."""
    if dist not in ("euclidean", "cosine"):
        raise ValueError("knn_graph: dist must be 'euclidean' or 'cosine', got %r" % (dist,))
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3):
        raise ValueError("knn_graph: x must be a tensor [N, D] or [B, N, D]")
    _dtype_code(x)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("knn_graph: k must be in [1, %d], got %d (a larger k is not built)" % (MAX_K, k))
    D = x.shape[-1]
    if not 1 <= D <= MAX_D:
        raise ValueError("knn_graph: the width D must be in [1, %d], got %d (wider rows are not built)" % (MAX_D, D))
    exclude_self = bool(exclude_self)
    if x.dim() == 3:
        if segs is not None:
            raise ValueError("knn_graph: a [B, N, D] input is already segmented; segs must be None")
        sizes, equal = None, (x.shape[0], x.shape[1])
        x = x.reshape(-1, D)
    elif segs is None:
        sizes, equal = None, (1, x.shape[0])
    else:
        sizes = _segment_sizes(segs, x.shape[0])
        equal = (len(sizes), sizes[0]) if sizes and all(s == sizes[0] for s in sizes) else None
    _require_cuda(x)
    n = x.shape[0]
    x = x.detach()
    if dist == "cosine":
        x = torch.nn.functional.normalize(x, dim=1)
    if x.stride(1) != 1 or x.stride(0) < D:
        x = x.contiguous()
    if equal is not None:
        seg_ptr, rowptr, nnz, min_deg = _equal_tables(equal[0], equal[1], k, exclude_self, x.device)
    else:
        seg_ptr, rowptr, nnz, min_deg = _unequal_tables(sizes, k, exclude_self, x.device)
    col = torch.empty(nnz, dtype=torch.int32, device=x.device)
    d = torch.empty(nnz, dtype=torch.float32, device=x.device) if return_dist else None
    if n and nnz:
        _lib.launch("dgll_hip_knn", x.device, x.data_ptr(), x.stride(0), _dtype_code(x), n, D, seg_ptr.data_ptr(), seg_ptr.numel() - 1,
                    k, int(exclude_self), rowptr.data_ptr(), col.data_ptr(), _lib.ptr(d), nnz, tag=lambda: ("knn", D, n))
    graph = CSRGraph(rowptr, col, None, n, n, check=False)
    graph.max_degree = k
    graph.seg_ptr = seg_ptr             # int64 [S + 1]: the segments the search ran in (and what keeps a cached table alive)
    graph.min_degree = min_deg          # known on the host: nn.EdgeConv's empty-row check needs no synchronisation
    return (graph, d) if return_dist else graph


def segmented_knn_graph(x, k, segs, **kwargs):
    """DGL's name for knn_graph(x, k, segs)."""
    return knn_graph(x, k, segs, **kwargs)


class KNNGraph(torch.nn.Module):
    """DGL's dgl.nn.KNNGraph: forward(x) = knn_graph(x, k) for x [N, D] or [B, N, D]."""

    def __init__(self, k):
        super().__init__()
        self.k = k

    def forward(self, x, dist="euclidean", exclude_self=False):
        return knn_graph(x, self.k, dist=dist, exclude_self=exclude_self)


class SegmentedKNNGraph(torch.nn.Module):
    """DGL's dgl.nn.SegmentedKNNGraph: forward(x, segs) = segmented_knn_graph(x, k, segs)."""

    def __init__(self, k):
        super().__init__()
        self.k = k

    def forward(self, x, segs, dist="euclidean", exclude_self=False):
        return knn_graph(x, self.k, segs, dist=dist, exclude_self=exclude_self)
