"""The learnable per-column soft reductions of DeeperGCN (PyG's SoftmaxAggregation and PowerMeanAggregation, what GENConv aggregates
with): csrc/soft_agg.hip.

    softmax_aggregate(graph, x, e=None, t=1.0, semi_grad=False, eps=1e-7)  -> out [n_dst, F]
    powermean_aggregate(graph, x, e=None, p=1.0, eps=1e-7)                 -> out [n_dst, F]

`graph` is a CSRGraph (n_dst rows gathering from n_src columns; rectangular blocks allowed; edge values are ignored).  Entry k of
row i is the edge j = col[k] -> i; duplicate entries are separate edges.  x [n_src, F], e [nnz, F] in the graph's entry order (or
None), one dtype.  For every column independently:

    m_k = relu(x[j] + e[k]) + eps
    softmax:     out_i = sum_k softmax_k(t m_k) m_k                      (t = 0 is the mean; semi_grad: the weights are constants of
                                                                         the backward, and t gets no gradient)
    power-mean:  out_i = (mean_k min(m_k, 100)^p)^(1/p)                  (p = 1 is the mean of the clamped messages)

A row without entries gives 0.  `t` / `p` are a Python float, or a one-element floating tensor / Parameter on the device, which gets
a gradient.  The value reaches the kernels as a pointer to one fp32 in device memory and is never read on the host: no .item(), no
synchronisation, so a step can be captured, and a captured step follows a `t` changed in place.  PyG's PowerMeanAggregation skips
the clamp and the powers when p == 1 exactly; here the formula above always holds -- the two differ only for messages above 100.
powermean_aggregate refuses eps <= 0 and a float p == 0 (a zero message has no power mean; a tensor p is not inspected).

ONE autograd node per op, three passes of one entry point (dgll_hip_soft_agg_pass), and it saves x, e, out and the fp32 row
statistics ([n_dst, 2 F]: softmax {lse | out}, power {out | S}) only: FORWARD over A; for the backward ROWS over A (grad_e, one
store per entry, and the scalar gradient: one fp32 partial per workgroup, summed in workgroup order) only when e, t or p needs a
gradient, and COLS over A^T (graph.transpose(), the cached structure, e read through its perm) for grad_x when x does.  Nothing of
the size of the edge list is allocated but grad_e itself.  No float atomics (reruns give the same bits, the scalar gradient
included), nothing allocated by a pass, synchronised or read back, fp32 accumulation.  There is no CPU implementation here: a CPU
tensor raises (nn.GENConv has a host path of its own).

Not built: one t / p per column (PyG's channels > 1), a fused edge projection, the partitioned (multi-GPU) path.
"""
import ctypes as C

import torch

from . import _lib
from .graph import CSRGraph
from .ops import _dtype_code, epv, _require_cuda, alloc_features, as_rows16

LONG_ROW = _lib.SOFT_AGG_LONG_ROW       # rows with more entries are swept by a whole workgroup
SOFTMAX, POWER = _lib.SOFT_AGG_SOFTMAX, _lib.SOFT_AGG_POWER
PARTIALS = 512                          # workgroups (per column block) of a ROWS pass that sums a scalar gradient, at the most
_TAGS = ("soft_agg_forward", "soft_agg_rows", "soft_agg_cols")


def _launch(kind, mode, gr, ref, theta, eps, semi=False, perm=None, nnz=0, n_partials=0, **mats):
    """One pass over `gr` (A, or A^T with its perm); `ref` gives the dtype and the width; theta: fp32 [1] on the device; mats:
    descriptor field -> matrix or None (partials and grad_theta: flat fp32 buffers)."""
    d = _lib.SoftAggDesc()
    d.pass_, d.dtype, d.mode, d.semi_grad = kind, _dtype_code(ref), mode, int(bool(semi))
    d.rowptr, d.col, d.perm = gr.rowptr.data_ptr(), gr.col.data_ptr(), _lib.ptr(perm)
    d.n_rows, d.n_cols, d.nnz, d.F, d.eps = gr.n_rows, gr.n_cols, nnz, ref.shape[1], eps
    d.theta, d.n_partials = theta.data_ptr(), n_partials
    for name, t in mats.items():
        setattr(d, name, _lib.ptr(t))
        if name not in ("partials", "grad_theta"):
            setattr(d, "ld_" + name, _lib.pitch(t))
    _lib.launch("dgll_hip_soft_agg_pass", gr.rowptr.device, C.byref(d), tag=lambda: (_TAGS[kind], d.F, gr.nnz))


def _like(rows, ref):
    return alloc_features(rows, ref.shape[1], ref.dtype, ref.device, pad_to=epv(ref.dtype))


# ---- raw passes (no autograd, no checks): what the autograd node, tools/softagg_bench.py and the tests call ------------------------------
# Matrices with rows on a 16-byte pitch; theta: fp32 [1] on the device.
def forward_raw(graph, mode, x, e, theta, eps):
    """(out [n_dst, F], stats fp32 [n_dst, 2 F])"""
    out = _like(graph.n_rows, x)
    stats = torch.empty((graph.n_rows, 2 * x.shape[1]), dtype=torch.float32, device=x.device)
    _launch(_lib.SOFT_AGG_FORWARD, mode, graph, x, theta, eps, nnz=graph.nnz, x=x, e=e, out=out, stats=stats)
    return out, stats


def rows_raw(graph, mode, x, e, theta, eps, stats, g, semi=False, need_e=True, need_theta=True):
    """(grad_e [nnz, F], grad_theta fp32 [1]) for the output gradient g.  An output that is not needed is None."""
    ge = _like(graph.nnz, x) if need_e else None
    gth = parts = None
    if need_theta:
        blocks = (x.shape[1] // epv(x.dtype) + 63) // 64
        parts = torch.empty(PARTIALS * blocks, dtype=torch.float32, device=x.device)
        gth = torch.empty(1, dtype=torch.float32, device=x.device)
    _launch(_lib.SOFT_AGG_ROWS, mode, graph, x, theta, eps, semi, nnz=graph.nnz, n_partials=PARTIALS if need_theta else 0,
            x=x, e=e, stats=stats, grad_out=g, grad_e=ge, partials=parts, grad_theta=gth)
    return ge, gth


def cols_raw(graph, mode, x, e, theta, eps, stats, g, semi=False):
    """grad_x [n_src, F] over graph.transpose()."""
    gt, perm = graph.transpose()
    gx = _like(gt.n_rows, x)
    _launch(_lib.SOFT_AGG_COLS, mode, gt, x, theta, eps, semi, perm=perm if e is not None else None, nnz=graph.nnz,
            x=x, e=e, stats=stats, grad_out=g, grad_x=gx)
    return gx


class _SoftAgg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, e, theta, graph, mode, semi, eps):
        xr = as_rows16(x.detach())
        er = None if e is None else as_rows16(e.detach())
        th = theta.detach().reshape(1)
        if th.dtype != torch.float32:
            th = th.float()
        out, stats = forward_raw(graph, mode, xr, er, th, eps)
        ctx.graph, ctx.mode, ctx.semi, ctx.eps = graph, mode, semi, eps
        ctx.theta_like = theta
        if any(ctx.needs_input_grad[:3]):
            ctx.save_for_backward(xr, er, th, out, stats)
        return out

    @staticmethod
    def backward(ctx, g):
        need_x, need_e, need_th = ctx.needs_input_grad[:3]
        need_th = need_th and not ctx.semi
        if not (need_x or need_e or need_th):
            return (None,) * 7
        xr, er, th, _, stats = ctx.saved_tensors
        gr = as_rows16(g)
        ge = gth = gx = None
        if need_e or need_th:
            ge, gth = rows_raw(ctx.graph, ctx.mode, xr, er, th, ctx.eps, stats, gr, ctx.semi, need_e, need_th)
            if gth is not None:
                gth = gth.to(ctx.theta_like.dtype).reshape(ctx.theta_like.shape)
        if need_x:
            gx = cols_raw(ctx.graph, ctx.mode, xr, er, th, ctx.eps, stats, gr, ctx.semi)
        return gx, ge, gth, None, None, None, None


def _aggregate(name, letter, graph, x, e, theta, mode, semi, eps):
    if not isinstance(graph, CSRGraph):
        raise TypeError("%s expects a CSRGraph (use dgll_amd.graph.as_csr_graph for torch sparse tensors)" % name)
    _dtype_code(x)
    if e is not None and e.dtype != x.dtype:
        raise TypeError("%s: x and e must have one dtype, got %s and %s" % (name, x.dtype, e.dtype))
    if x.dim() != 2 or x.shape[0] != graph.n_cols:
        raise ValueError("%s: x must be a matrix of %d rows (the sources), got %s" % (name, graph.n_cols, tuple(x.shape)))
    F, vec = x.shape[1], epv(x.dtype)
    if e is not None:
        if e.dim() != 2 or e.shape[0] != graph.nnz:
            raise ValueError("%s: e must be [nnz, F] with nnz = %d, got %s" % (name, graph.nnz, tuple(e.shape)))
        if e.shape[1] != F:
            raise ValueError("%s: e has %d columns and x %d: edge features of another width than the node features' are not built "
                             "(project them first, as nn.GENConv does)" % (name, e.shape[1], F))
    if F == 0 or F % vec:
        raise ValueError("%s: the width %d is not a whole number of 16-byte vectors (%d columns of %s); the layers pad their widths "
                         "with zero columns" % (name, F, vec, x.dtype))
    if not eps >= 0.0:
        raise ValueError("%s: eps must be >= 0, got %r" % (name, eps))
    if isinstance(theta, torch.Tensor):
        if theta.numel() != 1 or not theta.is_floating_point():
            raise ValueError("%s: %s must be a float or a one-element floating tensor (one %s per column is not built), got %s %s"
                             % (name, letter, letter, theta.dtype, tuple(theta.shape)))
        _require_cuda(x, e, graph.rowptr, theta)
    else:
        _require_cuda(x, e, graph.rowptr)
        theta = torch.full((1,), float(theta), dtype=torch.float32, device=x.device)
    if graph.n_rows == 0 or graph.nnz == 0:         # nothing to gather: zeros, with zero gradients
        zero = x.sum() + theta.sum().to(x.dtype) + (0 if e is None else e.sum())
        return x.new_zeros((graph.n_rows, F)) + 0 * zero
    return _SoftAgg.apply(x, e, theta, graph, mode, bool(semi), float(eps))


def softmax_aggregate(graph, x, e=None, t=1.0, semi_grad=False, eps=1e-7):
    """out [n_dst, F]: per column, the softmax(t m)-weighted sum of the messages m = relu(x[col_k] + e[k]) + eps over the entries k
    of row i (module docstring)."""
    return _aggregate("softmax_aggregate", "t", graph, x, e, t, SOFTMAX, semi_grad, eps)


def powermean_aggregate(graph, x, e=None, p=1.0, eps=1e-7):
    """out [n_dst, F]: per column, the power mean (mean_k min(m_k, 100)^p)^(1/p) of the messages m = relu(x[col_k] + e[k]) + eps over
    the entries k of row i (module docstring)."""
    if not eps > 0.0:
        raise ValueError("powermean_aggregate: eps must be > 0 (a zero message has no power mean), got %r" % (eps,))
    if not isinstance(p, torch.Tensor) and float(p) == 0.0:
        raise ValueError("powermean_aggregate: p must not be 0 (the geometric mean is not built)")
    return _aggregate("powermean_aggregate", "p", graph, x, e, p, POWER, False, eps)
