"""Edge-gated aggregation with edge outputs (DGL's GatedGCNConv underneath): csrc/gated.hip.

    gated_sum(graph, a, b, c, v, eps=1e-6) -> (out [n_dst, F], ehat [nnz, F])        a [n_dst, F]; b, v [n_src, F]; c [nnz, F]; one dtype

`graph` is a CSRGraph (n_dst rows gathering from n_src columns; rectangular blocks allowed; edge values are ignored).  Entry k of
row i is the edge j = col[k] -> i and c[k] its row, in the graph's entry order (ops_ef.edge_graph_from_coo); duplicate entries are
separate edges.  For every column independently:

    ehat[k] = c[k] + a[i] + b[j]        sig[k] = sigmoid(ehat[k])        out[i] = (sum_k sig[k] v[j]) / (sum_k sig[k] + eps)

A row without entries gives 0.  ehat is rounded to the storage dtype when stored, and every pass -- the forward included -- takes the
sigmoid of that stored value: forward and backward see the same gate, and no [nnz, F] array exists apart from c, ehat and their
gradients.  Both outputs carry gradients (ehat is the next layer's edge input).

ONE autograd node with two outputs, three passes of one entry point (dgll_hip_gated_pass): FORWARD over A, which also leaves the
fp32 row state (1 / S_i and the unrounded out_i, two [n_dst, F] arrays); for the backward ROWS over A (t[k] -> grad_c, its row sums ->
grad_a, and w_i = g_i / S_i) when any of a, b, c needs a gradient, and COLS over A^T (graph.transpose(), the cached structure; t and
ehat read through its perm) for grad_b and grad_v when b or v does.  When only v needs a gradient ROWS runs without its sweep and
just leaves w.  A gradient nobody asked for is neither computed nor returned.  No float atomics (reruns give the same bits),
nothing allocated by a pass, synchronised or read back (the step can be captured), fp32 accumulation.  There is no CPU
implementation here: a CPU tensor raises (the layer has a host path of its own).

Not built: ehat written in place over c, a fused projection of c, the partitioned (multi-GPU) path.  The variant without edge
features (PyG's ResGatedGraphConv: the gate from two node rows alone, nothing stored per edge) is ops_res_gated.
"""
import ctypes as C

import torch

from . import _lib
from .graph import CSRGraph
from .ops import _dtype_code, epv, _require_cuda, alloc_features, as_rows16

LONG_ROW = _lib.GATED_LONG_ROW      # rows with more entries are swept by a whole workgroup
_TAGS = ("gated_forward", "gated_rows", "gated_cols")


def _launch(kind, gr, perm, nnz, eps, ref, **mats):
    """One pass over `gr` (A, or A^T with its perm); `ref` gives the dtype and the width; mats: descriptor field -> matrix or None."""
    d = _lib.GatedDesc()
    d.pass_, d.dtype = kind, _dtype_code(ref)
    d.rowptr, d.col, d.perm = gr.rowptr.data_ptr(), gr.col.data_ptr(), _lib.ptr(perm)
    d.n_rows, d.n_cols, d.nnz, d.F, d.eps = gr.n_rows, gr.n_cols, nnz, ref.shape[1], eps
    for name, t in mats.items():
        setattr(d, name, _lib.ptr(t))
        setattr(d, "ld_" + name, _lib.pitch(t))
    _lib.launch("dgll_hip_gated_pass", gr.rowptr.device, C.byref(d), tag=lambda: (_TAGS[kind], d.F, nnz))


def _like(rows, ref, dtype=None):
    return alloc_features(rows, ref.shape[1], dtype or ref.dtype, ref.device, pad_to=epv(dtype or ref.dtype))


# ---- raw passes (no autograd, no checks): what the autograd node, tools/gated_bench.py and the tests call -------------------------------
# Matrices with rows on a 16-byte pitch.
def forward_raw(graph, a, b, c, v, eps=1e-6):
    """(out, ehat, inv_s, out32): the two results and the fp32 row state the backward reads."""
    out, ehat = _like(graph.n_rows, a), _like(graph.nnz, a)
    inv_s, out32 = _like(graph.n_rows, a, torch.float32), _like(graph.n_rows, a, torch.float32)
    _launch(_lib.GATED_FORWARD, graph, None, graph.nnz, eps, a, a=a, b=b, c=c, v=v, out=out, ehat=ehat, inv_s=inv_s, out32=out32)
    return out, ehat, inv_s, out32


def rows_raw(graph, v, ehat, inv_s, out32, g, ge=None, eps=1e-6, sweep=True, want_w=True):
    """(grad_c [nnz, F], grad_a [n_dst, F], w [n_dst, F]); ge: the gradient through ehat or None (passed as NULL, not as zeros).
    sweep=False: only w is formed (grad_c and grad_a are None); want_w=False: w is None."""
    gc = _like(graph.nnz, g) if sweep else None
    ga = _like(graph.n_rows, g) if sweep else None
    w = _like(graph.n_rows, g) if want_w else None
    _launch(_lib.GATED_ROWS, graph, None, graph.nnz, eps, g, v=v if sweep else None, ehat=ehat if sweep else None, inv_s=inv_s,
            out32=out32, grad_out=g, grad_ehat=ge if sweep else None, grad_c=gc, grad_a=ga, w=w)
    return gc, ga, w


def cols_raw(graph, t, ehat, w, need_b=True, need_v=True, eps=1e-6):
    """(grad_b, grad_v) [n_src, F] over graph.transpose(); t: the grad_c of rows_raw.  An output that is not needed is None, and
    what only it reads is not passed on."""
    gt, perm = graph.transpose()
    ref = t if need_b else w
    gb = _like(gt.n_rows, ref) if need_b else None
    gv = _like(gt.n_rows, ref) if need_v else None
    _launch(_lib.GATED_COLS, gt, perm, graph.nnz, eps, ref, grad_c=t if need_b else None, ehat=ehat if need_v else None,
            w=w if need_v else None, grad_b=gb, grad_v=gv)
    return gb, gv


class _GatedSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, c, v, graph, eps):
        ar, br, cr, vr = (as_rows16(t.detach()) for t in (a, b, c, v))
        out, ehat, inv_s, out32 = forward_raw(graph, ar, br, cr, vr, eps)
        ctx.graph, ctx.eps = graph, eps
        ctx.set_materialize_grads(False)            # a missing gradient of ehat stays None: the rows pass takes NULL
        if any(ctx.needs_input_grad[:4]):
            ctx.save_for_backward(vr, ehat, inv_s, out32)
        return out, ehat

    @staticmethod
    def backward(ctx, g, ge):
        need_a, need_b, need_c, need_v = ctx.needs_input_grad[:4]
        if not (need_a or need_b or need_c or need_v) or (g is None and ge is None):
            return None, None, None, None, None, None
        vr, ehat, inv_s, out32 = ctx.saved_tensors
        gr = as_rows16(g) if g is not None else torch.zeros_like(out32, dtype=ehat.dtype)
        ger = as_rows16(ge) if ge is not None else None
        sweep, cols = need_a or need_b or need_c, need_b or need_v
        gc, ga, w = rows_raw(ctx.graph, vr, ehat, inv_s, out32, gr, ger, ctx.eps, sweep=sweep, want_w=need_v)
        gb, gv = cols_raw(ctx.graph, gc, ehat, w, need_b, need_v, ctx.eps) if cols else (None, None)
        return ga if need_a else None, gb, gc if need_c else None, gv, None, None


def gated_sum(graph, a, b, c, v, eps=1e-6):
    """(out [n_dst, F], ehat [nnz, F]): ehat[k] = c[k] + a[i] + b[col_k], out[i] the sigmoid(ehat)-gated mean of v[col_k] over the
    entries k of row i (module docstring)."""
    if not isinstance(graph, CSRGraph):
        raise TypeError("gated_sum expects a CSRGraph (use dgll_amd.graph.as_csr_graph for torch sparse tensors)")
    for t in (a, b, c, v):
        _dtype_code(t)
    if not (a.dtype == b.dtype == c.dtype == v.dtype):
        raise TypeError("gated_sum: a, b, c and v must have one dtype, got %s, %s, %s and %s" % (a.dtype, b.dtype, c.dtype, v.dtype))
    if a.dim() != 2 or a.shape[0] != graph.n_rows:
        raise ValueError("gated_sum: a must be a matrix of %d rows (the destinations), got %s" % (graph.n_rows, tuple(a.shape)))
    for name, t in (("b", b), ("v", v)):
        if t.dim() != 2 or t.shape[0] != graph.n_cols:
            raise ValueError("gated_sum: %s must be a matrix of %d rows (the sources), got %s" % (name, graph.n_cols, tuple(t.shape)))
    if c.dim() != 2 or c.shape[0] != graph.nnz:
        raise ValueError("gated_sum: c must be [nnz, F] with nnz = %d, got %s" % (graph.nnz, tuple(c.shape)))
    F, vec = a.shape[1], epv(a.dtype)
    for name, t in (("b", b), ("c", c), ("v", v)):
        if t.shape[1] != F:
            raise ValueError("gated_sum: %s has %d columns and a %d: the four operands share one width (project them first, as "
                             "nn.GatedGCNConv does)" % (name, t.shape[1], F))
    if F == 0 or F % vec:
        raise ValueError("gated_sum: the width %d is not a whole number of 16-byte vectors (%d columns of %s); the layers pad "
                         "their widths with zero columns" % (F, vec, a.dtype))
    eps = float(eps)
    if not eps > 0.0:
        raise ValueError("gated_sum: eps must be positive (it is the denominator of a row without entries), got %r" % (eps,))
    _require_cuda(a, b, c, v, graph.rowptr)
    if graph.n_rows == 0 or graph.nnz == 0:         # nothing to gather: zeros, with zero gradients
        zero = 0 * (a.sum() + b.sum() + c.sum() + v.sum())
        return a.new_zeros((graph.n_rows, F)) + zero, c.new_zeros((graph.nnz, F)) + zero
    return _GatedSum.apply(a, b, c, v, graph, eps)
