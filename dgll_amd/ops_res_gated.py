"""Gated aggregation with nothing stored per edge (PyG's ResGatedGraphConv underneath): csrc/res_gated.hip.

    res_gated_sum(graph, k, q, v, reduce="sum") -> out [n_dst, F]        k [n_dst, F]; q, v [n_src, F]; one dtype

`graph` is a CSRGraph (n_dst rows gathering from n_src columns; rectangular blocks allowed; edge values are ignored).  Entry e of
row i is the edge j = col[e] -> i; duplicate entries are separate edges.  For every column independently:

    s = sigmoid(k[i] + q[j])        out[i] = sum_e s v[j]        (reduce="mean": divided by the row's entry count)

A row without entries gives 0.  The gate needs two node rows and nothing else, so every pass recomputes it -- the same fp32 function
of the same stored k and q -- and no [nnz, F] array exists, in the forward or in the backward: the memory of a training step is
O((n_dst + n_src) F).  This is the gated layer that trains on graphs whose per-edge arrays (ops_gated: c, ehat and their gradients)
do not fit.

ONE autograd node, three passes of one entry point (dgll_hip_res_gated_pass), and it saves k, q and v only: FORWARD over A; for the
backward ROWS over A (grad_k) when k needs a gradient, and COLS over A^T (graph.transpose()[0], the cached structure; an ordinary
gather, its permutation is not used) for grad_q and grad_v when q or v does -- only the requested one is summed.  reduce="mean":
the forward sets the descriptor's `mean`; the backward divides the output gradient by the entry counts once (one [n_dst, F] torch
multiply with graph.inv_degrees(), cached, to be built outside a capture) and runs the same two passes.  No float atomics (reruns
give the same bits), nothing allocated by a pass, synchronised or read back (the step can be captured), fp32 accumulation.  There is
no CPU implementation here: a CPU tensor raises (the layer has a host path of its own).

Not built: a normalised form (/ (sum of gates + eps)), ROWS fused into COLS, the partitioned (multi-GPU) path.
"""
import ctypes as C

import torch

from . import _lib
from .graph import CSRGraph
from .ops import _dtype_code, epv, _require_cuda, alloc_features, as_rows16

LONG_ROW = _lib.RES_GATED_LONG_ROW      # rows with more entries are swept by a whole workgroup
_TAGS = ("res_gated_forward", "res_gated_rows", "res_gated_cols")


def _launch(kind, gr, ref, mean=False, **mats):
    """One pass over `gr` (A, or A^T); `ref` gives the dtype and the width; mats: descriptor field -> matrix or None."""
    d = _lib.ResGatedDesc()
    d.pass_, d.dtype = kind, _dtype_code(ref)
    d.rowptr, d.col = gr.rowptr.data_ptr(), gr.col.data_ptr()
    d.n_rows, d.n_cols, d.F, d.mean = gr.n_rows, gr.n_cols, ref.shape[1], int(bool(mean))
    for name, t in mats.items():
        setattr(d, name, _lib.ptr(t))
        setattr(d, "ld_" + name, _lib.pitch(t))
    _lib.launch("dgll_hip_res_gated_pass", gr.rowptr.device, C.byref(d), tag=lambda: (_TAGS[kind], d.F, gr.nnz))


def _like(rows, ref):
    return alloc_features(rows, ref.shape[1], ref.dtype, ref.device, pad_to=epv(ref.dtype))


# ---- raw passes (no autograd, no checks): what the autograd node, tools/resgated_bench.py and the tests call ---------------------------
# Matrices with rows on a 16-byte pitch.
def forward_raw(graph, k, q, v, mean=False):
    """out [n_dst, F]"""
    out = _like(graph.n_rows, k)
    _launch(_lib.RES_GATED_FORWARD, graph, k, mean, k=k, q=q, v=v, out=out)
    return out


def rows_raw(graph, k, q, v, g):
    """grad_k [n_dst, F] for the output gradient g (of a mean: already divided by the entry counts)"""
    gk = _like(graph.n_rows, k)
    _launch(_lib.RES_GATED_ROWS, graph, k, k=k, q=q, v=v, grad_out=g, grad_k=gk)
    return gk


def cols_raw(graph, k, q, v, g, need_q=True, need_v=True):
    """(grad_q, grad_v) [n_src, F] over graph.transpose()[0].  An output that is not needed is None; v is passed on only for grad_q."""
    gt = graph.transpose()[0]
    gq = _like(gt.n_rows, q) if need_q else None
    gv = _like(gt.n_rows, q) if need_v else None
    _launch(_lib.RES_GATED_COLS, gt, q, k=k, q=q, v=v if need_q else None, grad_out=g, grad_q=gq, grad_v=gv)
    return gq, gv


class _ResGatedSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, k, q, v, graph, mean):
        kr, qr, vr = (as_rows16(t.detach()) for t in (k, q, v))
        out = forward_raw(graph, kr, qr, vr, mean)
        ctx.graph, ctx.mean = graph, mean
        if any(ctx.needs_input_grad[:3]):
            ctx.save_for_backward(kr, qr, vr)
        return out

    @staticmethod
    def backward(ctx, g):
        need_k, need_q, need_v = ctx.needs_input_grad[:3]
        if not (need_k or need_q or need_v):
            return None, None, None, None, None
        kr, qr, vr = ctx.saved_tensors
        if ctx.mean:                                # d out_i = g_i / deg_i: one node-sized multiply, then the passes of the sum
            gr = torch.mul(g, ctx.graph.inv_degrees().unsqueeze(1), out=_like(g.shape[0], kr))
        else:
            gr = as_rows16(g)
        gk = rows_raw(ctx.graph, kr, qr, vr, gr) if need_k else None
        gq, gv = cols_raw(ctx.graph, kr, qr, vr, gr, need_q, need_v) if need_q or need_v else (None, None)
        return gk, gq, gv, None, None


def res_gated_sum(graph, k, q, v, reduce="sum"):
    """out [n_dst, F]: out[i] the sigmoid(k[i] + q[col_e])-gated sum (or mean) of v[col_e] over the entries e of row i (module
    docstring)."""
    if not isinstance(graph, CSRGraph):
        raise TypeError("res_gated_sum expects a CSRGraph (use dgll_amd.graph.as_csr_graph for torch sparse tensors)")
    if reduce not in ("sum", "mean"):
        raise ValueError("res_gated_sum: reduce must be 'sum' or 'mean', got %r" % (reduce,))
    for t in (k, q, v):
        _dtype_code(t)
    if not (k.dtype == q.dtype == v.dtype):
        raise TypeError("res_gated_sum: k, q and v must have one dtype, got %s, %s and %s" % (k.dtype, q.dtype, v.dtype))
    if k.dim() != 2 or k.shape[0] != graph.n_rows:
        raise ValueError("res_gated_sum: k must be a matrix of %d rows (the destinations), got %s" % (graph.n_rows, tuple(k.shape)))
    for name, t in (("q", q), ("v", v)):
        if t.dim() != 2 or t.shape[0] != graph.n_cols:
            raise ValueError("res_gated_sum: %s must be a matrix of %d rows (the sources), got %s" % (name, graph.n_cols, tuple(t.shape)))
    F, vec = k.shape[1], epv(k.dtype)
    for name, t in (("q", q), ("v", v)):
        if t.shape[1] != F:
            raise ValueError("res_gated_sum: %s has %d columns and k %d: the three operands share one width (project them first, as "
                             "nn.ResGatedGraphConv does)" % (name, t.shape[1], F))
    if F == 0 or F % vec:
        raise ValueError("res_gated_sum: the width %d is not a whole number of 16-byte vectors (%d columns of %s); the layers pad "
                         "their widths with zero columns" % (F, vec, k.dtype))
    _require_cuda(k, q, v, graph.rowptr)
    if graph.n_rows == 0 or graph.nnz == 0:         # nothing to gather: zeros, with zero gradients
        return k.new_zeros((graph.n_rows, F)) + 0 * (k.sum() + q.sum() + v.sum())
    return _ResGatedSum.apply(k, q, v, graph, reduce == "mean")
