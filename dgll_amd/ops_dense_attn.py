"""Dense attention inside every graph of a batch (the global half of a GraphGPS / graph-transformer block): csrc/seg_attn.hip.

    segment_attention(q, k, v, heads, segs=None, batch=None, scale=None) -> out [N, heads * D]

The N rows are cut into contiguous segments by `segs` (a list of segment sizes: no read-back, and equal segments take their tables
from the cache of points.py) or by `batch` (a non-decreasing int64 vector of graph ids, as PyG batches are; its sizes are read back
once), exactly as in ops_pool; with neither, the rows are one segment.  Per segment s and head h of width D:

    S = scale Q_s,h K_s,h^T      P = softmax over the keys of the segment      out_s,h = P V_s,h

Every row attends to every row of its own segment and to no other.  An empty segment costs nothing; in a segment of one row, out
equals v.  This is what PyG does with to_dense_batch + torch.nn.MultiheadAttention, without the padded [B, max_n, C] batch, and what
sparse_attention does on a complete graph per segment, without the sum of n_s^2 column indices.

q, k, v [N, heads * D] are fp32 or bf16 on the GPU (fp32 accumulation), on a unit column stride; rows on a 16-byte pitch are read in
place (three column slices of one [N, 3 * heads * D] projection), anything else is copied once.  D must be a whole number of 16-byte
vectors (4 fp32 / 8 bf16 columns -- the layers pad their heads) and at most 128.  scale defaults to D ** -0.5; a layer that pads
its heads passes the scale of the TRUE head width.  `k is v` is allowed (autograd adds the two gradients).

One autograd node over three MFMA passes behind dgll_hip_segment_attn_pass: the forward (online softmax; leaves lse [N, heads]), a
pass over query tiles (grad_q, delta [N, heads]) and one over key tiles (grad_k and grad_v; skipped when neither is needed).  No
[n, n] array exists, nothing is read back, no float atomics: reruns give the same bits and the step can be captured.  There is no
CPU implementation here: a CPU tensor raises.
"""
import ctypes as C

import torch

from . import _lib
from .ops import _dtype_code, _require_cuda, alloc_features, as_rows16, epv
from .ops_attn import _same_buffer
from .ops_pool import _tables, segment_sizes

TILE = _lib.SEG_ATTN_TILE           # rows of a work item: one wavefront per (segment, tile, head)
MAX_D = _lib.SEG_ATTN_MAX_D


def _launch(kind, tables, n_segs, heads, D, scale, q, k, v, out, out2=None, grad_out=None, o=None, lse=None, delta=None):
    d = _lib.SegAttnDesc()
    d.pass_, d.dtype = kind, _dtype_code(q)
    d.seg_ptr, d.tile_ptr, d.n_rows, d.n_segs = tables[0].data_ptr(), tables[1].data_ptr(), q.shape[0], n_segs
    d.heads, d.D, d.scale = heads, D, scale
    d.q, d.ld_q, d.k, d.ld_k, d.v, d.ld_v = q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0)
    d.grad_out, d.ld_grad_out, d.o, d.ld_o = _lib.ptr(grad_out), _lib.pitch(grad_out), _lib.ptr(o), _lib.pitch(o)
    d.out, d.ld_out, d.out2, d.ld_out2 = out.data_ptr(), out.stride(0), _lib.ptr(out2), _lib.pitch(out2)
    d.lse, d.delta = _lib.ptr(lse), _lib.ptr(delta)
    _lib.launch("dgll_hip_segment_attn_pass", q.device, C.byref(d),
                tag=lambda: ("seg_attn_" + ("fwd", "rows", "cols")[kind], heads, D, str(q.dtype), q.shape[0]))


def segment_tables(sizes, device):
    """(seg_ptr, tile_ptr) int64 [S + 1] on the device: the row and the 32-row-tile prefix of segments of `sizes` (one upload)"""
    return _tables(sizes, [-(-s // TILE) for s in sizes], device)


def segment_attention_forward_raw(tables, n_segs, q, k, v, heads, scale):
    """(out, lse) with no autograd; q / k / v as as_rows16 leaves them"""
    n, D = q.shape[0], q.shape[1] // heads
    out = alloc_features(n, heads * D, q.dtype, q.device, pad_to=epv(q.dtype))
    lse = torch.empty((n, heads), dtype=torch.float32, device=q.device)
    _launch(_lib.SEG_ATTN_FORWARD, tables, n_segs, heads, D, scale, q, k, v, out, lse=lse)
    return out, lse


def segment_attention_backward_raw(tables, n_segs, q, k, v, out, lse, g, heads, scale, need_kv=True):
    """(grad_q, grad_k or None, grad_v or None) from the output gradient g (rows on a 16-byte pitch)"""
    n, D, vec = q.shape[0], q.shape[1] // heads, epv(q.dtype)
    dq = alloc_features(n, heads * D, q.dtype, q.device, pad_to=vec)
    delta = torch.empty((n, heads), dtype=torch.float32, device=q.device)
    _launch(_lib.SEG_ATTN_ROWS, tables, n_segs, heads, D, scale, q, k, v, dq, grad_out=g, o=out, lse=lse, delta=delta)
    dk = dv = None
    if need_kv:
        dk = alloc_features(n, heads * D, q.dtype, q.device, pad_to=vec)
        dv = alloc_features(n, heads * D, q.dtype, q.device, pad_to=vec)
        _launch(_lib.SEG_ATTN_COLS, tables, n_segs, heads, D, scale, q, k, v, dk, out2=dv, grad_out=g, lse=lse, delta=delta)
    return dq, dk, dv


class _SegmentAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, tables, n_segs, heads, scale):
        qr, kr = as_rows16(q.detach()), as_rows16(k.detach())
        vr = kr if _same_buffer(k, v) else as_rows16(v.detach())
        out, lse = segment_attention_forward_raw(tables, n_segs, qr, kr, vr, heads, scale)
        ctx.tables, ctx.n_segs, ctx.heads, ctx.scale = tables, n_segs, heads, scale
        ctx.save_for_backward(qr, kr, vr, out, lse)
        return out

    @staticmethod
    def backward(ctx, g):
        qr, kr, vr, out, lse = ctx.saved_tensors
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        if not (need_q or need_k or need_v):
            return (None,) * 7
        dq, dk, dv = segment_attention_backward_raw(ctx.tables, ctx.n_segs, qr, kr, vr, out, lse, as_rows16(g.to(qr.dtype)), ctx.heads,
                                                    ctx.scale, need_kv=need_k or need_v)
        return (dq if need_q else None), (dk if need_k else None), (dv if need_v else None), None, None, None, None


def segment_attention(q, k, v, heads, segs=None, batch=None, scale=None):
    """out[i, h] = sum over the rows j of i's segment of softmax_j(scale <q[i, h], k[j, h]>) v[j, h]; see the module text."""
    _dtype_code(q)
    heads = int(heads)
    if q.dim() != 2 or k.shape != q.shape or v.shape != q.shape or q.dtype != k.dtype or q.dtype != v.dtype:
        raise ValueError("segment_attention: q, k and v must be matrices [N, heads * D] of one shape and dtype")
    if heads < 1 or q.shape[1] % heads:
        raise ValueError("segment_attention: heads = %d does not divide the %d columns" % (heads, q.shape[1]))
    n, D, vec = q.shape[0], q.shape[1] // heads, epv(q.dtype)
    if D == 0 or D % vec:
        raise ValueError("segment_attention: D = %d is not a whole number of 16-byte vectors (%d columns of %s); the layers pad "
                         "their heads" % (D, vec, q.dtype))
    if D > MAX_D:
        raise ValueError("segment_attention: D = %d, a head may span at most %d columns" % (D, MAX_D))
    sizes = segment_sizes("segment_attention", n, segs, batch)       # the argument errors come first, whatever the device
    _require_cuda(q, k, v, batch)
    scale = float(D) ** -0.5 if scale is None else float(scale)
    if n == 0:
        return q.new_zeros((0, heads * D)) + 0 * (q.sum() + k.sum() + v.sum())
    return _SegmentAttn.apply(q, k, v, segment_tables(sizes, q.device), len(sizes), heads, scale)
