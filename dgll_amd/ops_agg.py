"""Several reductions of a neighbourhood from one gather (PNA, DGL's PNAConv): csrc/multi_agg.hip.

    multi_aggregate(graph, x_src, y_dst=None, aggregators=("mean", "max", "min", "std"),
                    scalers=("identity", "amplification", "attenuation"), delta=1.0)
        -> [n_dst, len(scalers) * len(aggregators) * F] of x_src.dtype
    pna_delta(graph) -> float          mean over the rows of log(D_i + 1), the usual choice of delta

`graph` is a CSRGraph (n_dst rows gathering from n_src columns; rectangular blocks allowed; edge values are ignored, duplicate
entries are separate edges).  Over the D_i entries j of row i, with x = x_src [n_src, F] and y = y_dst [n_dst, F] (None: 0):

    mean  mean_j x[j] + y[i]        sum  sum_j x[j] + D_i y[i]        max / min  max_j x[j] + y[i] / min_j x[j] + y[i]
    var   relu(mean_j x[j]^2 - (mean_j x[j])^2)                       std  sqrt(var + 1e-30)            (y does not enter these two)

which are the reductions of the per-edge message x[j] + y[i] -- PNA's message M(cat(h_j, h_i)) is linear and splits so
(nn.PNAConv) -- without a per-edge tensor.  Block (s * len(aggregators) + a) of the output is scaler_s(i) * aggregator_a(i), DGL's
concatenation order, with identity 1, amplification log(D_i + 1) / delta, attenuation delta / log(D_i + 1).  A row without entries
gives zeros in every block.

One autograd node, three passes of one entry point (dgll_hip_multi_agg_pass): FORWARD over A (saves the rows' mean / variance and
the arg-max / arg-min source rows only when a gradient is needed and the chosen aggregators use them), then ROWS (element-wise:
scalers folded, per-row coefficients, grad_y) and COLS over A^T (graph.transpose(), the cached structure).  Gradients nobody needs
are not computed.  The variance is accumulated about the row's first entry (a row of equal entries gives exactly var = 0) and its
gradient is exactly 0 where var <= 0 (torch's relu'(0) = 0).  Ties of max / min go to the smallest source id among the entries
attaining the extreme; torch gives the gradient to an unspecified one of them, so the gradients differ from torch's on ties only.
No atomics (reruns give the same bits), nothing allocated by a pass, synchronised or read back (the step can be captured), fp32
accumulation.  There is no CPU implementation here: a CPU tensor raises (nn.PNAConv has a host path of its own).

Not built: the moment aggregators ("moment3" .. "moment5"), per-edge features, the partitioned (multi-GPU) path.
"""
import ctypes as C

import torch

from . import _lib
from .graph import CSRGraph
from .ops import _dtype_code, epv, _require_cuda, as_rows16

LONG_ROW = _lib.MAGG_LONG_ROW       # rows with more entries are swept by a whole workgroup
AGGREGATORS = {"mean": _lib.MAGG_MEAN, "sum": _lib.MAGG_SUM, "max": _lib.MAGG_MAX, "min": _lib.MAGG_MIN, "var": _lib.MAGG_VAR,
               "std": _lib.MAGG_STD}
SCALERS = {"identity": _lib.MAGG_IDENTITY, "amplification": _lib.MAGG_AMPLIFICATION, "attenuation": _lib.MAGG_ATTENUATION}
_NOT_BUILT = ("moment3", "moment4", "moment5")
_TAGS = ("magg_forward", "magg_rows", "magg_cols")
_USE_STATS, _USE_ARG = (_lib.MAGG_VAR, _lib.MAGG_STD), (_lib.MAGG_MAX, _lib.MAGG_MIN)


def _desc(kind, graph, F, dtype, aggs, scalers, delta):
    d = _lib.MultiAggDesc()
    d.pass_, d.dtype = kind, dtype
    d.rowptr, d.col, d.n_rows, d.n_cols, d.F = graph.rowptr.data_ptr(), graph.col.data_ptr(), graph.n_rows, graph.n_cols, F
    d.n_agg, d.n_scaler, d.delta = len(aggs), len(scalers), delta
    for i, c in enumerate(aggs):
        d.agg[i] = c
    for i, c in enumerate(scalers):
        d.scaler[i] = c
    return d


def _launch(d, graph):
    _lib.launch("dgll_hip_multi_agg_pass", graph.rowptr.device, C.byref(d), tag=lambda: (_TAGS[d.pass_], d.F, d.n_agg * d.n_scaler, graph.nnz))


# ---- raw passes (no autograd, no checks): what the autograd node and tools/pna_bench.py call; aggs / scalers are code tuples --------
def forward_raw(graph, x, y, aggs, scalers, delta, want_stats=False, want_arg=False):
    """(out, stats or None, arg or None); x, y with rows on a 16-byte pitch."""
    F = x.shape[1]
    out = torch.empty((graph.n_rows, len(aggs) * len(scalers) * F), dtype=x.dtype, device=x.device)
    stats = torch.empty((graph.n_rows, 2 * F), dtype=torch.float32, device=x.device) if want_stats else None
    arg = torch.empty((graph.n_rows, 2 * F), dtype=torch.int32, device=x.device) if want_arg else None
    d = _desc(_lib.MAGG_FORWARD, graph, F, _dtype_code(x), aggs, scalers, delta)
    d.x, d.ld_x, d.y, d.ld_y, d.out, d.ld_out = x.data_ptr(), x.stride(0), _lib.ptr(y), _lib.pitch(y), out.data_ptr(), out.stride(0)
    d.stats, d.ld_stats, d.arg, d.ld_arg = _lib.ptr(stats), _lib.pitch(stats), _lib.ptr(arg), _lib.pitch(arg)
    _launch(d, graph)
    return out, stats, arg


def rows_raw(graph, grad_out, stats, aggs, scalers, delta, want_coef=True, want_grad_y=True):
    """(coef fp32 [n_rows, 5 F] or None, grad_y [n_rows, F] or None) from the gradient of forward_raw's output."""
    F = grad_out.shape[1] // (len(aggs) * len(scalers))
    coef = torch.empty((graph.n_rows, 5 * F), dtype=torch.float32, device=grad_out.device) if want_coef else None
    gy = torch.empty((graph.n_rows, F), dtype=grad_out.dtype, device=grad_out.device) if want_grad_y else None
    d = _desc(_lib.MAGG_ROWS, graph, F, _dtype_code(grad_out), aggs, scalers, delta)
    d.grad_out, d.ld_grad_out, d.stats, d.ld_stats = grad_out.data_ptr(), grad_out.stride(0), _lib.ptr(stats), _lib.pitch(stats)
    d.coef, d.ld_coef, d.grad_y, d.ld_grad_y = _lib.ptr(coef), _lib.pitch(coef), _lib.ptr(gy), _lib.pitch(gy)
    _launch(d, graph)
    return coef, gy


def cols_raw(graph, x, coef, arg, aggs, scalers, delta):
    """grad_x [n_src, F] over graph.transpose(); coef and arg are those of graph's rows."""
    gt, _ = graph.transpose()
    gx = torch.empty((gt.n_rows, x.shape[1]), dtype=x.dtype, device=x.device)
    d = _desc(_lib.MAGG_COLS, gt, x.shape[1], _dtype_code(x), aggs, scalers, delta)
    d.x, d.ld_x, d.coef, d.ld_coef, d.arg, d.ld_arg = x.data_ptr(), x.stride(0), coef.data_ptr(), coef.stride(0), _lib.ptr(arg), _lib.pitch(arg)
    d.grad_x, d.ld_grad_x = gx.data_ptr(), gx.stride(0)
    _launch(d, gt)
    return gx


class _MultiAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, graph, aggs, scalers, delta):
        xr = as_rows16(x.detach())
        yr = None if y is None else as_rows16(y.detach())
        need_x, need_y = ctx.needs_input_grad[0], y is not None and ctx.needs_input_grad[1]
        out, stats, arg = forward_raw(graph, xr, yr, aggs, scalers, delta,
                                      want_stats=need_x and any(c in _USE_STATS for c in aggs),
                                      want_arg=need_x and any(c in _USE_ARG for c in aggs))
        ctx.graph, ctx.aggs, ctx.scalers, ctx.delta, ctx.need = graph, aggs, scalers, delta, (need_x, need_y)
        ctx.save_for_backward(*(t for t in (xr if need_x else None, stats, arg) if t is not None))
        ctx.has = (need_x, stats is not None, arg is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        need_x, need_y = ctx.need
        if not (need_x or need_y):
            return None, None, None, None, None, None
        saved = list(ctx.saved_tensors)
        xr, stats, arg = (saved.pop(0) if h else None for h in ctx.has)
        gr = as_rows16(g if xr is None or g.dtype == xr.dtype else g.to(xr.dtype))
        coef, gy = rows_raw(ctx.graph, gr, stats, ctx.aggs, ctx.scalers, ctx.delta, want_coef=need_x, want_grad_y=need_y)
        gx = cols_raw(ctx.graph, xr, coef, arg, ctx.aggs, ctx.scalers, ctx.delta) if need_x else None
        return gx, gy, None, None, None, None


def _codes(names, table, what):
    if isinstance(names, str):
        names = (names,)
    names = tuple(names)
    for n in names:
        if n in _NOT_BUILT:
            raise NotImplementedError("multi_aggregate: the moment aggregators (%s) are not built; built: %s" % (n, ", ".join(AGGREGATORS)))
        if n not in table:
            raise ValueError("multi_aggregate: unknown %s %r; known: %s" % (what, n, ", ".join(table)))
    if not names or len(set(names)) != len(names):
        raise ValueError("multi_aggregate: %ss must be a non-empty list without repeats, got %r" % (what, names))
    return tuple(table[n] for n in names)


def _matrix(t, rows, name):
    _dtype_code(t)
    if t.dim() != 2 or t.shape[0] != rows:
        raise ValueError("multi_aggregate: %s must be a matrix of %d rows, got %s" % (name, rows, tuple(t.shape)))
    F, vec = t.shape[1], epv(t.dtype)
    if F == 0 or F % vec:
        raise ValueError("multi_aggregate: the width %d of %s is not a whole number of 16-byte vectors (%d columns of %s); the layers "
                         "pad their widths with zero columns" % (F, name, vec, t.dtype))


def multi_aggregate(graph, x_src, y_dst=None, aggregators=("mean", "max", "min", "std"),
                    scalers=("identity", "amplification", "attenuation"), delta=1.0):
    """[n_dst, len(scalers) * len(aggregators) * F]: block (s * len(aggregators) + a) = scaler_s * aggregator_a of the messages
    x_src[j] + y_dst[i] over the entries of row i (module docstring)."""
    if not isinstance(graph, CSRGraph):
        raise TypeError("multi_aggregate expects a CSRGraph (use dgll_amd.graph.as_csr_graph for torch sparse tensors)")
    aggs, scs = _codes(aggregators, AGGREGATORS, "aggregator"), _codes(scalers, SCALERS, "scaler")
    delta = float(delta)
    if not delta > 0.0 or delta == float("inf"):
        raise ValueError("multi_aggregate: delta must be a positive number, got %r" % delta)
    _matrix(x_src, graph.n_cols, "x_src")
    if y_dst is not None:
        _matrix(y_dst, graph.n_rows, "y_dst")
        if y_dst.dtype != x_src.dtype or y_dst.shape[1] != x_src.shape[1]:
            raise ValueError("multi_aggregate: x_src and y_dst must be matrices of one dtype and width")
    _require_cuda(x_src, y_dst, graph.rowptr)
    if graph.n_rows == 0 or graph.nnz == 0:     # nothing to gather: zeros, with zero gradients
        zero = x_src.sum() if y_dst is None else x_src.sum() + y_dst.sum()
        return x_src.new_zeros((graph.n_rows, len(aggs) * len(scs) * x_src.shape[1])) + 0 * zero
    return _MultiAggregate.apply(x_src, y_dst, graph, aggs, scs, delta)


def pna_delta(graph):
    """mean over the rows of log(D_i + 1): PNA's delta, computed once per training graph (reads one number back)."""
    if not isinstance(graph, CSRGraph):
        raise TypeError("pna_delta expects a CSRGraph")
    if graph.n_rows == 0:
        return 1.0
    return float(torch.log(graph.degrees().to(torch.float64) + 1.0).mean())
