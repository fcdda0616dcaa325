"""Sparse scaled dot-product attention (DGL's DotGatConv, PyG's TransformerConv, graph-transformer blocks): csrc/sparse_attn.hip.

    sparse_attention(graph, q, k, v, heads, scale=None) -> out [n_dst, heads * D]

Per head h of width D, over the entries j of row i of `graph` (a CSRGraph, n_dst rows gathering from n_src columns; rectangular
blocks allowed; edge values are ignored, duplicate entries are separate edges):

    s_ij = scale <q[i, h], k[j, h]>      alpha = softmax_j s_ij      out[i, h] = sum_j alpha_ij v[j, h]

An empty row gives 0.  q [n_dst, heads * D], k and v [n_src, heads * D] are fp32 or bf16 on the GPU (fp32 accumulation); D must be a
whole number of 16-byte vectors (4 fp32 / 8 bf16 columns -- the layers pad their heads) and a head must fit a wavefront's lanes
(D <= 256 fp32, 512 bf16).  scale defaults to D ** -0.5; a layer that pads its heads passes the scale of the TRUE head width.
`k is v` (DotGatConv) is detected: each source row is then loaded once per edge and autograd adds the two gradients.

One autograd node over three gather passes, all behind dgll_hip_sparse_attn_pass: the forward (online softmax; leaves lse
[n_dst, heads]), and for the backward a pass over the rows of A (grad_q, {lse, delta} per row) and one over the rows of A^T (grad_k
and grad_v; graph.transpose(), the cached structure), skipped when neither k nor v needs a gradient.  Nothing is stored per edge,
nothing is read back, no float atomics: reruns give the same bits and the step can be captured.  There is no CPU implementation
here: a CPU tensor raises.
"""
import ctypes as C

import torch

from . import _lib
from .graph import CSRGraph
from .ops import _dtype_code, epv, _require_cuda, alloc_features, as_rows16

LONG_ROW = _lib.ATTN_LONG_ROW       # rows with more entries are swept by a whole workgroup
_MAX_VECTORS = 64                   # a head fits a wavefront's lanes: D / EPV <= 64


def _launch(kind, graph, heads, D, scale, shared, q, k, v, out, out2=None, grad_out=None, lse=None, lse_delta=None):
    d = _lib.AttnDesc()
    d.pass_, d.dtype = kind, _dtype_code(q)
    d.rowptr, d.col, d.n_rows, d.n_cols = graph.rowptr.data_ptr(), graph.col.data_ptr(), graph.n_rows, graph.n_cols
    d.heads, d.D, d.scale, d.kv_shared = heads, D, scale, int(shared)
    d.q, d.ld_q, d.k, d.ld_k, d.v, d.ld_v = q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0)
    d.grad_out, d.ld_grad_out = _lib.ptr(grad_out), _lib.pitch(grad_out)
    d.out, d.ld_out, d.out2, d.ld_out2 = out.data_ptr(), out.stride(0), _lib.ptr(out2), _lib.pitch(out2)
    d.lse, d.lse_delta = _lib.ptr(lse), _lib.ptr(lse_delta)
    _lib.launch("dgll_hip_sparse_attn_pass", q.device, C.byref(d),
                tag=lambda: ("attn_" + ("fwd", "rows", "cols")[kind], heads, D, str(q.dtype), graph.nnz))


def _same_buffer(a, b):
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


def sparse_attention_forward_raw(graph, q, k, v, heads, scale):
    """(out, lse) with no autograd; q / k / v as as_rows16 leaves them (k and v the same tensor: one gather per edge)."""
    D = q.shape[1] // heads
    out = alloc_features(graph.n_rows, heads * D, q.dtype, q.device, pad_to=epv(q.dtype))
    lse = torch.empty((graph.n_rows, heads), dtype=torch.float32, device=q.device)
    _launch(_lib.ATTN_FORWARD, graph, heads, D, scale, _same_buffer(k, v), q, k, v, out, lse=lse)
    return out, lse


def sparse_attention_backward_raw(graph, q, k, v, heads, scale, lse, g, need_kv=True):
    """(grad_q, grad_k or None, grad_v or None) from the output gradient g (rows on a 16-byte pitch)."""
    D = q.shape[1] // heads
    vec = epv(q.dtype)
    shared = _same_buffer(k, v)
    dq = alloc_features(graph.n_rows, heads * D, q.dtype, q.device, pad_to=vec)
    lse_delta = torch.empty((graph.n_rows, 2 * heads), dtype=torch.float32, device=q.device)
    _launch(_lib.ATTN_ROWS, graph, heads, D, scale, shared, q, k, v, dq, grad_out=g, lse=lse, lse_delta=lse_delta)
    dk = dv = None
    if need_kv:
        gt, _ = graph.transpose()
        dk = alloc_features(graph.n_cols, heads * D, q.dtype, q.device, pad_to=vec)
        dv = alloc_features(graph.n_cols, heads * D, q.dtype, q.device, pad_to=vec)
        _launch(_lib.ATTN_COLS, gt, heads, D, scale, shared, q, k, v, dk, out2=dv, grad_out=g, lse_delta=lse_delta)
    return dq, dk, dv


class _SparseAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, graph, heads, scale):
        shared = _same_buffer(k, v)
        qr, kr = as_rows16(q.detach()), as_rows16(k.detach())
        vr = kr if shared else as_rows16(v.detach())
        out, lse = sparse_attention_forward_raw(graph, qr, kr, vr, heads, scale)
        ctx.graph, ctx.heads, ctx.scale = graph, heads, scale
        ctx.save_for_backward(qr, kr, vr, lse)
        return out

    @staticmethod
    def backward(ctx, g):
        qr, kr, vr, lse = ctx.saved_tensors
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        if not (need_q or need_k or need_v):
            return None, None, None, None, None, None
        if g.dtype != qr.dtype:
            g = g.to(qr.dtype)
        dq, dk, dv = sparse_attention_backward_raw(ctx.graph, qr, kr, vr, ctx.heads, ctx.scale, lse, as_rows16(g), need_kv=need_k or need_v)
        return (dq if need_q else None), (dk if need_k else None), (dv if need_v else None), None, None, None


def sparse_attention(graph, q, k, v, heads, scale=None):
    """out[i, h] = sum_j softmax_j(scale <q[i, h], k[j, h]>) v[j, h]; see the module text."""
    if not isinstance(graph, CSRGraph):
        raise TypeError("sparse_attention expects a CSRGraph (use dgll_amd.graph.as_csr_graph for torch sparse tensors)")
    _require_cuda(q, k, v, graph.rowptr)
    _dtype_code(q)
    heads = int(heads)
    if q.dim() != 2 or k.dim() != 2 or v.dim() != 2 or q.dtype != k.dtype or q.dtype != v.dtype or q.shape[1] != k.shape[1] \
            or q.shape[1] != v.shape[1]:
        raise ValueError("q [n_dst, heads * D], k and v [n_src, heads * D] must be matrices of one dtype and width")
    if q.shape[0] != graph.n_rows or k.shape[0] != graph.n_cols or v.shape[0] != graph.n_cols:
        raise ValueError("q has %d rows, k %d and v %d, but the graph gathers %d sources into %d destinations"
                         % (q.shape[0], k.shape[0], v.shape[0], graph.n_cols, graph.n_rows))
    if heads < 1 or q.shape[1] % heads:
        raise ValueError("heads = %d does not divide the %d columns" % (heads, q.shape[1]))
    D = q.shape[1] // heads
    vec = epv(q.dtype)
    if D == 0 or D % vec:
        raise ValueError("D = %d is not a whole number of 16-byte vectors (%d columns of %s); the layers pad their heads"
                         % (D, vec, q.dtype))
    if D // vec > _MAX_VECTORS:
        raise ValueError("D = %d: a head may span at most %d columns of %s (64 16-byte vectors)" % (D, _MAX_VECTORS * vec, q.dtype))
    scale = float(D) ** -0.5 if scale is None else float(scale)
    if graph.n_rows == 0 or graph.nnz == 0:         # nothing to gather: zeros, with zero gradients
        return q.new_zeros((graph.n_rows, heads * D)) + 0 * (q.sum() + k.sum() + v.sum())
    return _SparseAttn.apply(q, k, v, graph, heads, scale)
