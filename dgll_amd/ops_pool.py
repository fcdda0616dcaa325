"""Selecting rows of every graph of a batch by a score, on the device (csrc/seg_sort.hip): the core of TopKPooling, SAGPooling and
SortPooling (nn/GlobalPooling/select.py).

    segment_topk(score, segs=None, batch=None, *, ratio=None, k=None, return_inverse=False)   -> int64 idx  (or (idx, int32 inv))
    select(x, score, idx, inv, act="tanh")                                                    -> x[idx] * act(score[idx])
    sort_pool(x, segs=None, batch=None, *, k)                                                 -> [B, k * F]

A batch is cut into contiguous segments of rows, by `segs` (a list of segment sizes as in knn_graph / fps: no read-back, and equal
segments take their pointer tables from the cache of points.py) or by `batch` (a non-decreasing int64 vector of graph ids, as PyG
batches are; its sizes are read back once; an unsorted vector raises ValueError).  With neither, the rows are one segment.

segment_topk orders the rows of every segment by SCORE DESCENDING, TIES TO THE SMALLER ROW INDEX (-0.0 equals +0.0, every NaN ranks
after -inf, NaNs among themselves by index: the contract of dgll_hip_segment_sort) and keeps the first ceil(ratio * size) of them
(`ratio` in (0, 1]) or the first min(k, size) (`k`).  score is [N] or [N, 1], float32 or bfloat16, and is not differentiated.  idx
holds global row ids, segment after segment, and carries idx.seg_sizes, the rows kept per segment as a Python list, so that the next
layer needs no read-back.  inv (return_inverse) is int32 [N]: the position in idx of a kept row, -1 for every other row.

select is the scaled gather out[j] = x[idx[j]] * act(score[idx[j]]), act one of "none" (a pure gather; score may be None),
"identity", "tanh", "sigmoid", the multiplier in fp32; differentiable in x and score through ONE streaming pass over the rows of x
that reads inv (no scatter-add, no memset, no atomics: two runs give the same bits).  A negative idx[j] gives a row of zeros.

sort_pool is SortPooling's read-out (PyG's global_sort_pool): the rows of every graph ordered by their LAST channel, the first k kept,
graphs of fewer than k rows padded with zero rows by the same gather launch, flattened to [B, k * F].  The gradient reaches x through
the gather only.  There is no CPU implementation: a CPU tensor raises.
"""
import itertools
import math

import torch

from . import _lib
from .ops import _dtype_code, _require_cuda, _row_major, alloc_features, epv
from .points import _Samples, _equal_tables

TILE = _lib.SEGSORT_TILE            # a segment of up to this many rows is sorted by one workgroup; longer ones through a scratch array
ACTS = {"none": _lib.POOL_ACT_NONE, "identity": _lib.POOL_ACT_IDENTITY, "tanh": _lib.POOL_ACT_TANH, "sigmoid": _lib.POOL_ACT_SIGMOID}


def keep_counts(sizes, ratio=None, k=None):
    """rows kept of segments of `sizes`: ceil(ratio * size) each, or min(k, size) each"""
    if (ratio is None) == (k is None):
        raise ValueError("segment_topk: give exactly one of ratio and k")
    if k is not None:
        if int(k) != k or int(k) < 1:
            raise ValueError("segment_topk: k must be an integer >= 1, got %r" % (k,))
        return [min(int(k), s) for s in sizes]
    if not 0.0 < float(ratio) <= 1.0:
        raise ValueError("segment_topk: ratio must be in (0, 1], got %r" % (ratio,))
    return [min(s, int(math.ceil(float(ratio) * s))) for s in sizes]


def segment_sizes(what, n, segs=None, batch=None):
    """the segment sizes, as a Python list, of n rows cut by `segs` or by `batch` (module docstring)"""
    if segs is not None and batch is not None:
        raise ValueError("%s: give segs or batch, not both" % what)
    if batch is not None:
        if not isinstance(batch, torch.Tensor) or batch.dim() != 1 or batch.dtype != torch.int64 or batch.numel() != n:
            raise ValueError("%s: batch must be an int64 vector with one graph id per row (%d)" % (what, n))
        if n == 0:
            return []
        bad = (batch[1:] < batch[:-1]).any() | (batch[0] < 0)
        got = torch.cat([torch.bincount(batch.clamp(min=0)), bad.to(torch.int64).view(1)]).tolist()     # the one read-back
        if got[-1]:
            raise ValueError("%s: batch must be non-decreasing graph ids >= 0 (sort the batch, or give segs)" % what)
        return got[:-1]
    if segs is None:
        return [n]
    if isinstance(segs, torch.Tensor):
        if segs.is_floating_point() or segs.dim() != 1:
            raise ValueError("%s: segs must be a 1-D integer tensor or a sequence of segment sizes" % what)
        segs = segs.tolist()
    sizes = [int(s) for s in segs]
    if any(s < 0 for s in sizes) or sum(sizes) != n:
        raise ValueError("%s: the segment sizes must be >= 0 and sum to the number of rows %d, got a sum of %d" % (what, n, sum(sizes)))
    return sizes


def _tables(sizes, counts, device):
    """(seg_ptr, out_ptr) int64 [S + 1] on the device: equal segments from the cache of points.py (no upload), others as ONE upload"""
    if len(set(sizes)) == 1 and len(set(counts)) == 1:
        return _equal_tables(len(sizes), sizes[0], counts[0], device)
    both = torch.tensor([0, *itertools.accumulate(sizes), 0, *itertools.accumulate(counts)], dtype=torch.int64).to(device)
    return both[:len(sizes) + 1], both[len(sizes) + 1:]


def _sorted_rows(score, sizes, counts, want_inv):
    """(idx int64 [sum(counts)], inv int32 [N] or None) of one dgll_hip_segment_sort launch; counts[s] > sizes[s] pads with -1"""
    n, dev, n_out = score.numel(), score.device, sum(counts)
    idx = torch.empty(n_out, dtype=torch.int64, device=dev)
    inv = torch.empty(n, dtype=torch.int32, device=dev) if want_inv else None
    if n_out == 0 or n == 0:
        if inv is not None:
            inv.fill_(-1)
        return idx.fill_(-1), inv
    seg_ptr, out_ptr = _tables(sizes, counts, dev)
    max_seg = max(sizes)
    scratch = torch.empty(2 * n, dtype=torch.int64, device=dev) if max_seg > TILE else None
    _lib.launch("dgll_hip_segment_sort", dev, score.data_ptr(), _dtype_code(score), n, seg_ptr.data_ptr(), len(sizes), max_seg,
                out_ptr.data_ptr(), idx.data_ptr(), _lib.ptr(inv), n_out, _lib.ptr(scratch), tag=lambda: ("segment_sort", max_seg, n))
    return idx, inv


def _score_vector(what, score):
    if not isinstance(score, torch.Tensor) or not (score.dim() == 1 or (score.dim() == 2 and score.shape[1] == 1)):
        raise ValueError("%s: score must be a tensor [N] or [N, 1]" % what)
    _dtype_code(score)
    return score.detach().reshape(-1).contiguous()


def segment_topk(score, segs=None, batch=None, *, ratio=None, k=None, return_inverse=False):
    """int64 row ids of the best rows of every segment, best first (module docstring); with return_inverse also int32 inv [N]."""
    score = _score_vector("segment_topk", score)
    keep_counts([], ratio, k)           # the argument errors come first, whatever the device
    _require_cuda(score, batch)
    sizes = segment_sizes("segment_topk", score.numel(), segs, batch)
    counts = keep_counts(sizes, ratio, k)
    idx, inv = _sorted_rows(score, sizes, counts, return_inverse)
    idx = idx.as_subclass(_Samples)
    idx.seg_sizes = counts
    return (idx, inv) if return_inverse else idx


def _act_code(act):
    try:
        return ACTS["none" if act is None else act]
    except KeyError:
        raise ValueError("select: act must be one of %s, got %r" % (sorted(ACTS), act))


def select_raw(x, score, idx, act, out=None):
    """out[j] = x[idx[j]] * act(score[idx[j]]) with no autograd; x [n, F] on a unit column stride, score [n] contiguous or None.
    out: a buffer [len(idx), F] of x's dtype to write into (every row of it is written)."""
    n, F, n_out = x.shape[0], x.shape[1], idx.numel()
    if out is None:
        out = alloc_features(n_out, F, x.dtype, x.device, pad_to=epv(x.dtype))
    if n_out:
        _lib.launch("dgll_hip_pool_select", x.device, x.data_ptr(), x.stride(0), _dtype_code(x), n, F, _lib.ptr(score),
                    _lib.F32 if score is None else _dtype_code(score), act, idx.data_ptr(), n_out, out.data_ptr(), out.stride(0),
                    tag=lambda: ("pool_select", F, str(x.dtype), n_out))
    return out


def select_bwd_raw(x, score, inv, g, n_out, act, want_x=True, want_score=True, grad_x=None, grad_score=None):
    """(grad_x [n, F] of x's dtype or None, grad_score fp32 [n] or None) from g [n_out, F]; every row of both is written.
    grad_x / grad_score: buffers to write into."""
    n, F, dev = x.shape[0], x.shape[1], x.device
    if want_x and grad_x is None:
        grad_x = alloc_features(n, F, x.dtype, dev, pad_to=epv(x.dtype))
    if want_score and grad_score is None:
        grad_score = torch.empty(n, dtype=torch.float32, device=dev)
    if n and (want_x or want_score):
        _lib.launch("dgll_hip_pool_select_bwd", dev, x.data_ptr(), x.stride(0), _dtype_code(x), n, F, _lib.ptr(score),
                    _lib.F32 if score is None else _dtype_code(score), act, inv.data_ptr(), g.data_ptr() if n_out else None, _lib.pitch(g),
                    n_out, _lib.ptr(grad_x) if want_x else None, _lib.pitch(grad_x), _lib.ptr(grad_score) if want_score else None,
                    tag=lambda: ("pool_select_bwd", F, str(x.dtype), n))
    return (grad_x if want_x else None), (grad_score if want_score else None)


class _Select(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, score, idx, inv, act):
        xr = _row_major(x.detach())
        sr = None if score is None else score.detach().reshape(-1).contiguous()
        ctx.act, ctx.n_out, ctx.score_shape = act, idx.numel(), None if score is None else score.shape
        ctx.save_for_backward(xr, sr, inv)
        return select_raw(xr, sr, idx, act)

    @staticmethod
    def backward(ctx, g):
        xr, sr, inv = ctx.saved_tensors
        want_x, want_s = ctx.needs_input_grad[0], sr is not None and ctx.needs_input_grad[1] and ctx.act != _lib.POOL_ACT_NONE
        gx, gs = select_bwd_raw(xr, sr, inv, _row_major(g.to(xr.dtype)), ctx.n_out, ctx.act, want_x, want_s)
        if gs is not None:
            gs = gs.to(sr.dtype).view(ctx.score_shape)
        elif sr is not None and ctx.needs_input_grad[1]:
            gs = torch.zeros(ctx.score_shape, dtype=sr.dtype, device=sr.device)     # act "none": the score reaches nothing
        return gx, gs, None, None, None


def select(x, score, idx, inv, act="tanh"):
    """x[idx] * act(score[idx]) as [len(idx), F] of x's dtype, differentiable in x and score (module docstring).  idx and inv as
    segment_topk(..., return_inverse=True) returned them for the n rows of x."""
    code = _act_code(act)
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("select: x must be a matrix [n, F] with F >= 1")
    _dtype_code(x)
    if score is None:
        if code != _lib.POOL_ACT_NONE:
            raise ValueError("select: act %r needs a score" % (act,))
    else:
        _dtype_code(score)
        if score.numel() != x.shape[0]:
            raise ValueError("select: score has %d entries for %d rows of x" % (score.numel(), x.shape[0]))
    _require_cuda(x, score, idx, inv)
    if idx.dtype != torch.int64 or idx.dim() != 1 or inv is None or inv.dtype != torch.int32 or inv.shape != (x.shape[0],):
        raise ValueError("select: idx must be int64 [n_out] and inv int32 [n], as segment_topk(..., return_inverse=True) returns them")
    return _Select.apply(x, score, idx.as_subclass(torch.Tensor).contiguous(), inv.contiguous(), code)


def sort_pool(x, segs=None, batch=None, *, k):
    """[B, k * F]: the k rows of every graph with the largest last channel, in that order, zero rows behind a short graph."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("sort_pool: x must be a matrix [n, F] with F >= 1")
    if int(k) != k or int(k) < 1:
        raise ValueError("sort_pool: k must be an integer >= 1, got %r" % (k,))
    _dtype_code(x)
    _require_cuda(x, batch)
    sizes = segment_sizes("sort_pool", x.shape[0], segs, batch)
    idx, inv = _sorted_rows(x.detach()[:, -1].contiguous(), sizes, [int(k)] * len(sizes), True)
    return select(x, None, idx, inv, act="none").reshape(len(sizes), int(k) * x.shape[1])
