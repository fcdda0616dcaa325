"""Sampling and grouping of point clouds on the device, the two operations of PointNet++'s set abstraction: farthest point sampling
(DGL's dgl.geometry.farthest_point_sampler, PyG's fps; csrc/fps.hip, one launch) and the fixed-radius search between two point sets
(PyG's radius / radius_graph, PointNet++'s ball query, SchNet's interaction graph; csrc/radius.hip).

    fps(x, segs=None, *, ratio=None, npoints=None, start=0, return_dmin=False)      -> int64 idx  (or (idx, fp32 dmin))
    farthest_point_sampler(pos [B, N, C], npoints, start_idx=None)                  -> int64 [B, npoints], offsets inside each cloud
    radius(x, y, r, segs_x=None, segs_y=None, *, max_num_neighbors=32, return_dist=False)   -> CSRGraph [len(y) x len(x)]
    radius_graph(x, r, segs=None, *, loop=False, max_num_neighbors=32, return_dist=False)   -> CSRGraph [N x N]

Points are [N, D] or [B, N, D] (B segments of N points), float32 or bfloat16, 1 <= D <= MAX_D; `segs` is a list of segment sizes as in
knn_graph.  Distances are fp32 squared Euclidean in the difference form, computed on the inputs as they are stored.

fps picks m_s well-spread points of every segment: `ratio` gives ceil(ratio * size) per segment (as PyG), `npoints` the same count in
every segment (it raises above the smallest segment).  Sample 0 is the point at offset `start` of its segment (an int, an int64 tensor
[S], or "random": one torch.randint on the device, nothing read back; offsets wrap modulo the size); every later sample is the point
farthest from the ones chosen so far, ties to the smaller index, no point twice.  idx holds global row ids, segment after segment, and
carries idx.seg_sizes, the m_s as a Python list, so that the next call needs no read-back.  return_dmin also gives the squared
distance each sample had to the chosen set when it was taken (+inf for sample 0): the coverage radius.  With EQUAL segments the
tables come from a small cache: no host synchronisation, and the call can be captured into a graph.

radius lists, for every query row of y, the points of x in the same segment within distance r, in ascending index, at most
max_num_neighbors of them -- the FIRST by index, PointNet++'s ball-query order, which is what makes the result deterministic (PyG's
own pick is unspecified).  Row i of the graph (the destination) is query i, its entries (the sources) are rows of x; max_degree is
max_num_neighbors and seg_ptr the query segments.  r is compared as float32(r) * float32(r) against the fp32 squared distance.
radius_graph(x, r) is radius(x, x, r) without the self pairs unless loop=True.  The call reads nnz back once (8 bytes), so it is not
capturable, and returns col[:nnz] as a view of the padded buffer.  There is no CPU implementation: a CPU tensor raises.

Not built: knn(x, y) between two sets and knn_interpolate, a padded fixed-degree (capturable) ball query, D > 32, more than 64
neighbours, one segment spread over several workgroups in fps (a segment of more than 8192 points is sampled correctly but slowly),
approximate or grid-hashed search, the partitioned path.
"""
import math

import torch

from . import _lib
from .graph import CSRGraph
from .ops import _dtype_code, _require_cuda

MAX_D, MAX_K = _lib.FPS_MAX_D, _lib.RADIUS_MAX_K
MAX_REG_SEG = _lib.FPS_MAX_REG_SEG      # fps keeps dmin in registers up to this segment size

_tables = {}                            # (S, size, m or None, device) -> (seg_ptr, out_ptr or None)
_TABLES_KEPT = 64


def _ptr_of(sizes, device):
    ptr = torch.zeros(len(sizes) + 1, dtype=torch.int64)
    torch.cumsum(torch.tensor(sizes, dtype=torch.int64), 0, out=ptr[1:])
    return ptr.to(device)


def _equal_tables(n_segs, size, m, device):
    key = (n_segs, size, m, device)
    hit = _tables.get(key)
    if hit is None:
        step = lambda w: torch.arange(0, n_segs * w + 1, w, dtype=torch.int64, device=device) if w else \
            torch.zeros(n_segs + 1, dtype=torch.int64, device=device)                                  # noqa: E731
        if len(_tables) >= _TABLES_KEPT:
            _tables.pop(next(iter(_tables)))
        hit = _tables[key] = (step(size), None if m is None else step(m))
    return hit


def _points(what, x, segs):
    """(x [N, D] detached on a unit column stride, sizes) of a [N, D] / [B, N, D] input with its `segs`"""
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3):
        raise ValueError("%s: points must be a tensor [N, D] or [B, N, D]" % what)
    _dtype_code(x)
    D = x.shape[-1]
    if not 1 <= D <= MAX_D:
        raise ValueError("%s: the width D must be in [1, %d], got %d (wider points are not built)" % (what, MAX_D, D))
    if x.dim() == 3:
        if segs is not None:
            raise ValueError("%s: a [B, N, D] input is already segmented; segs must be None" % what)
        sizes = [x.shape[1]] * x.shape[0]
        x = x.reshape(-1, D)
    elif segs is None:
        sizes = [x.shape[0]]
    else:
        if isinstance(segs, torch.Tensor):
            if segs.is_floating_point() or segs.dim() != 1:
                raise ValueError("%s: segs must be a 1-D integer tensor or a sequence of segment sizes" % what)
            segs = segs.tolist()
        sizes = [int(s) for s in segs]
        if any(s < 0 for s in sizes) or sum(sizes) != x.shape[0]:
            raise ValueError("%s: the segment sizes must be >= 0 and sum to the number of points %d, got a sum of %d"
                             % (what, x.shape[0], sum(sizes)))
    _require_cuda(x)
    x = x.detach()
    if x.stride(1) != 1 or x.stride(0) < D:
        x = x.contiguous()
    return x, sizes


def _seg_ptr(sizes, counts, device):
    """(seg_ptr, out_ptr) on the device for segments of `sizes` yielding `counts` samples (None: no out_ptr); from the cache, without
    an upload, when all segments are equal"""
    if sizes and len(set(sizes)) == 1 and (counts is None or len(set(counts)) == 1):
        return _equal_tables(len(sizes), sizes[0], None if counts is None else counts[0], device)
    return _ptr_of(sizes, device), None if counts is None else _ptr_of(counts, device)


def sample_counts(sizes, ratio=None, npoints=None):
    """m_s of fps for segments of `sizes`: ceil(ratio * size) each, or npoints each"""
    if (ratio is None) == (npoints is None):
        raise ValueError("fps: give exactly one of ratio and npoints")
    if npoints is not None:
        npoints = int(npoints)
        if npoints < 0 or (sizes and npoints > min(sizes)):
            raise ValueError("fps: npoints must be in [0, %d], the smallest segment, got %d" % (min(sizes) if sizes else 0, npoints))
        return [npoints] * len(sizes)
    if not 0.0 < float(ratio) <= 1.0:
        raise ValueError("fps: ratio must be in (0, 1], got %r" % (ratio,))
    return [min(s, int(math.ceil(float(ratio) * s))) for s in sizes]


class _Samples(torch.Tensor):
    """the int64 index tensor fps returns; seg_sizes: the samples per segment, known on the host"""
    seg_sizes = None
    __torch_function__ = torch._C._disabled_torch_function_impl        # what is computed from it is a plain tensor


def fps(x, segs=None, *, ratio=None, npoints=None, start=0, return_dmin=False):
    """int64 row ids of the farthest-point samples of every segment (module docstring); with return_dmin also fp32 dmin."""
    x, sizes = _points("fps", x, segs)
    counts = sample_counts(sizes, ratio, npoints)
    n, D, dev, S = x.shape[0], x.shape[1], x.device, len(sizes)
    seg_ptr, out_ptr = _seg_ptr(sizes, counts, dev)
    n_out = sum(counts)
    if isinstance(start, str):
        if start != "random":
            raise ValueError("fps: start must be an int, an int64 tensor [S] or 'random', got %r" % (start,))
        start_t = torch.randint(0, 1 << 31, (S,), dtype=torch.int64, device=dev)
    elif isinstance(start, torch.Tensor):
        if start.dtype != torch.int64 or start.shape != (S,):
            raise ValueError("fps: a start tensor must be int64 [%d], got %s %s" % (S, start.dtype, tuple(start.shape)))
        _require_cuda(start)
        start_t = start.contiguous()
    else:
        start_t = None if int(start) == 0 else torch.full((S,), int(start), dtype=torch.int64, device=dev)
    idx = torch.empty(n_out, dtype=torch.int64, device=dev)
    dmin = torch.empty(n_out, dtype=torch.float32, device=dev) if return_dmin else None
    max_seg = max(sizes) if sizes else 0
    scratch = torch.empty(n, dtype=torch.float32, device=dev) if max_seg > MAX_REG_SEG else None
    if n_out:
        _lib.launch("dgll_hip_fps", dev, x.data_ptr(), x.stride(0), _dtype_code(x), n, D, seg_ptr.data_ptr(), S, max_seg, out_ptr.data_ptr(),
                    _lib.ptr(start_t), idx.data_ptr(), _lib.ptr(dmin), n_out, _lib.ptr(scratch), tag=lambda: ("fps", D, n))
    idx = idx.as_subclass(_Samples)
    idx.seg_sizes = counts
    return (idx, dmin) if return_dmin else idx


def farthest_point_sampler(pos, npoints, start_idx=None):
    """DGL's dgl.geometry.farthest_point_sampler: pos [B, N, C] -> int64 [B, npoints], each row the offsets inside its own cloud.
    start_idx: the first sample's offset in every cloud; None draws it at random, as DGL does."""
    if not isinstance(pos, torch.Tensor) or pos.dim() != 3:
        raise ValueError("farthest_point_sampler: pos must be [B, N, C]")
    B, N = pos.shape[0], pos.shape[1]
    idx = fps(pos, npoints=npoints, start="random" if start_idx is None else start_idx)
    return idx.as_subclass(torch.Tensor).view(B, int(npoints)) - torch.arange(B, device=pos.device).unsqueeze(1) * N


def radius(x, y, r, segs_x=None, segs_y=None, *, max_num_neighbors=32, return_dist=False, _exclude_self=False):
    """CSRGraph [len(y) x len(x)]: row i lists the first max_num_neighbors points of x, by index, within r of y[i] in its segment
    (module docstring); with return_dist also their fp32 squared distances [nnz]."""
    K = int(max_num_neighbors)
    if not 1 <= K <= MAX_K:
        raise ValueError("radius: max_num_neighbors must be in [1, %d], got %d (more are not built)" % (MAX_K, K))
    r2 = torch.tensor(r, dtype=torch.float32)
    if not float(r2) >= 0.0:
        raise ValueError("radius: r must be >= 0, got %r" % (r,))
    r2 = float(r2 * r2)
    same = y is x and segs_y is segs_x
    if _exclude_self and not same:
        raise ValueError("radius: self pairs can be skipped only when the queries are the candidates (radius_graph)")
    x, sizes_x = _points("radius", x, segs_x)
    y, sizes_y = (x, sizes_x) if same else _points("radius", y, segs_y)
    if x.dtype != y.dtype or x.shape[1] != y.shape[1] or x.device != y.device or len(sizes_x) != len(sizes_y):
        raise ValueError("radius: x and y must have the same dtype, width, device and number of segments, got %s %s in %d and %s %s in %d"
                         % (x.dtype, tuple(x.shape), len(sizes_x), y.dtype, tuple(y.shape), len(sizes_y)))
    n, m, D, dev, S = x.shape[0], y.shape[0], x.shape[1], x.device, len(sizes_x)
    x_seg = _seg_ptr(sizes_x, None, dev)[0]
    y_seg = x_seg if same else _seg_ptr(sizes_y, None, dev)[0]
    rowptr = torch.empty(m + 1, dtype=torch.int64, device=dev)
    col = torch.empty(m * K, dtype=torch.int32, device=dev)
    dist = torch.empty(m * K, dtype=torch.float32, device=dev) if return_dist else None
    nnz = torch.empty(1, dtype=torch.int64, device=dev)
    scratch = torch.empty(m * K + m, dtype=torch.int32, device=dev)
    _lib.launch("dgll_hip_radius", dev, y.data_ptr(), y.stride(0), m, y_seg.data_ptr(), x.data_ptr(), x.stride(0), n, x_seg.data_ptr(), S,
                _dtype_code(x), D, r2, K, int(_exclude_self), rowptr.data_ptr(), col.data_ptr(), _lib.ptr(dist), nnz.data_ptr(),
                scratch.data_ptr(), tag=lambda: ("radius", D, m))
    total = int(nnz)                                    # the one read-back (8 bytes)
    graph = CSRGraph(rowptr, col[:total], None, m, n, check=False)
    graph.max_degree = K
    graph.seg_ptr = y_seg
    return (graph, dist[:total]) if return_dist else graph


def radius_graph(x, r, segs=None, *, loop=False, max_num_neighbors=32, return_dist=False):
    """PyG's radius_graph: radius(x, x, r, segs, segs) without the pairs (i, i) unless loop=True."""
    return radius(x, x, r, segs, segs, max_num_neighbors=max_num_neighbors, return_dist=return_dist, _exclude_self=not loop)
