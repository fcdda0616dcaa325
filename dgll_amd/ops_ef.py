"""Edge-feature aggregation (DGL's GINEConv and CFConv underneath): csrc/edge_feat.hip.

    u_op_e_sum(graph, x, e, op="add", act=None, reduce="sum")     x [n_src, F], e [nnz, F] of one dtype -> [n_dst, F] of that dtype
    u_add_e_sum(graph, x, e, act=None, reduce="sum")              sum_k act(x[col_k] + e[k])
    u_mul_e_sum_full(graph, x, e, reduce="sum")                   sum_k x[col_k] * e[k]   (ops_mp.u_mul_e_sum takes one scalar per head)
    edge_graph_from_coo(src, dst, edge_feat, n_dst=None, n_src=None) -> (CSRGraph, edge_feat in entry order, order)

`graph` is a CSRGraph (n_dst rows gathering from n_src columns; rectangular blocks allowed; edge values are ignored).  Entry k of
row i is the edge j = col[k] -> i and e[k] its feature row, in the graph's entry order; duplicate entries are separate edges with
their own rows.  op "add" | "mul"; act None | "relu" (with "add" only); reduce "sum" | "mean" (the sum over the row's entries
divided by their number; an empty row gives zeros either way).

One autograd node, three passes of one entry point (dgll_hip_edge_feat_pass): FORWARD over A; for the backward COLS over A^T
(graph.transpose(), the cached structure, e read through its perm) for grad_x and EDGE over A for grad_e, each only when that
gradient is wanted.  relu's gate is never stored: every pass recomputes it as the same fp32 sum of the same stored operands.
What this costs is what a per-edge operand of width F costs: e is a real [nnz, F] array (and grad_e another), read once per pass.
No float atomics (reruns give the same bits, unlike index_add), nothing allocated by a pass, synchronised or read back (the step
can be captured), fp32 accumulation.  There is no CPU implementation here: a CPU tensor raises (the layers have a host path of
their own).

Not built: max / min over the messages, edge features of another width than the node features' (project them first: nn.GINE
does; ops_efp.u_op_proj_e_sum fuses a projection of up to 16 attribute columns into the kernel, so that e is never an array),
the partitioned (multi-GPU) path.
"""
import ctypes as C

import torch

from . import _lib
from .graph import CSRGraph
from .ops import _dtype_code, epv, _require_cuda, alloc_features, as_rows16

LONG_ROW = _lib.EF_LONG_ROW         # rows with more entries are swept by a whole workgroup
_TAGS = ("ef_forward", "ef_cols", "ef_edge")
_OPS = {("add", None): _lib.EF_ADD, ("add", "relu"): _lib.EF_ADD_RELU, ("mul", None): _lib.EF_MUL}


def _launch(kind, op, gr, perm, nnz, scale, ref, x=None, e=None, g=None, out=None, gx=None, ge=None):
    """One pass over `gr` (A, or A^T with its perm); `ref` gives the dtype and the width."""
    d = _lib.EdgeFeatDesc()
    d.pass_, d.dtype, d.op = kind, _dtype_code(ref), op
    d.rowptr, d.col, d.perm = gr.rowptr.data_ptr(), gr.col.data_ptr(), _lib.ptr(perm)
    d.n_rows, d.n_cols, d.nnz, d.F, d.scale = gr.n_rows, gr.n_cols, nnz, ref.shape[1], _lib.ptr(scale)
    d.x, d.ld_x, d.e, d.ld_e, d.grad_out, d.ld_grad_out = _lib.ptr(x), _lib.pitch(x), _lib.ptr(e), _lib.pitch(e), _lib.ptr(g), _lib.pitch(g)
    d.out, d.ld_out, d.grad_x, d.ld_grad_x = _lib.ptr(out), _lib.pitch(out), _lib.ptr(gx), _lib.pitch(gx)
    d.grad_e, d.ld_grad_e = _lib.ptr(ge), _lib.pitch(ge)
    _lib.launch("dgll_hip_edge_feat_pass", gr.rowptr.device, C.byref(d), tag=lambda: (_TAGS[kind], op, d.F, nnz))


def mean_scale(graph):
    """fp32 [n_dst]: 1 / D_i, 0 for a row without entries; cached on the graph."""
    if getattr(graph, "_ef_mean_scale", None) is None:
        deg = graph.degrees().to(torch.float32)
        graph._ef_mean_scale = torch.where(deg > 0, 1.0 / deg.clamp(min=1.0), torch.zeros_like(deg)).contiguous()
    return graph._ef_mean_scale


# ---- raw passes (no autograd, no checks): what the autograd node, tools/edge_feat_bench.py and the tests call ---------------------------
# x, e, g: matrices with rows on a 16-byte pitch; op: an _lib.EF_* code; scale: fp32 [n_dst] or None.  Operands the (pass, op) does
# not read are not passed on, whatever the caller gave.
def forward_raw(graph, x, e, op, scale=None):
    out = alloc_features(graph.n_rows, x.shape[1], x.dtype, x.device, pad_to=epv(x.dtype))
    _launch(_lib.EF_FORWARD, op, graph, None, graph.nnz, scale, x, x=x, e=e, out=out)
    return out


def cols_raw(graph, x, e, g, op, scale=None):
    """grad_x [n_src, F] over graph.transpose()."""
    gt, perm = graph.transpose()
    gx = alloc_features(gt.n_rows, g.shape[1], g.dtype, g.device, pad_to=epv(g.dtype))
    read_e = op != _lib.EF_ADD
    _launch(_lib.EF_COLS, op, gt, perm if read_e else None, graph.nnz, scale, g, x=x if op == _lib.EF_ADD_RELU else None,
            e=e if read_e else None, g=g, gx=gx)
    return gx


def edge_raw(graph, x, e, g, op, scale=None, out=None):
    """grad_e [nnz, F] in the graph's entry order (out: a [nnz, F] buffer of any 16-byte pitch to write instead of a new one)."""
    ge = alloc_features(graph.nnz, g.shape[1], g.dtype, g.device, pad_to=epv(g.dtype)) if out is None else out
    _launch(_lib.EF_EDGE, op, graph, None, graph.nnz, scale, g, x=x if op != _lib.EF_ADD else None,
            e=e if op == _lib.EF_ADD_RELU else None, g=g, ge=ge)
    return ge


class _UOpESum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, e, graph, op, scale):
        xr, er = as_rows16(x.detach()), as_rows16(e.detach())
        need_x, need_e = ctx.needs_input_grad[:2]
        ctx.graph, ctx.op, ctx.scale = graph, op, scale
        # the backward of "add" reads neither operand, that of "mul" one of them per gradient
        keep_x = (need_x and op == _lib.EF_ADD_RELU) or (need_e and op != _lib.EF_ADD)
        keep_e = (need_x and op != _lib.EF_ADD) or (need_e and op == _lib.EF_ADD_RELU)
        ctx.has = (keep_x, keep_e)
        ctx.save_for_backward(*(t for t, k in ((xr, keep_x), (er, keep_e)) if k))
        return forward_raw(graph, xr, er, op, scale)

    @staticmethod
    def backward(ctx, g):
        need_x, need_e = ctx.needs_input_grad[:2]
        if not (need_x or need_e):
            return None, None, None, None, None
        saved = list(ctx.saved_tensors)
        xr, er = (saved.pop(0) if h else None for h in ctx.has)
        gr = as_rows16(g)
        gx = cols_raw(ctx.graph, xr, er, gr, ctx.op, ctx.scale) if need_x else None
        ge = edge_raw(ctx.graph, xr, er, gr, ctx.op, ctx.scale) if need_e else None
        return gx, ge, None, None, None


def u_op_e_sum(graph, x, e, op="add", act=None, reduce="sum"):
    """out[i] = reduce over the entries k of row i of act(x[col_k] op e[k]) (module docstring)."""
    if not isinstance(graph, CSRGraph):
        raise TypeError("u_op_e_sum expects a CSRGraph (use dgll_amd.graph.as_csr_graph for torch sparse tensors)")
    if op not in ("add", "mul"):
        raise ValueError("u_op_e_sum: op must be 'add' or 'mul', got %r" % (op,))
    if act not in (None, "relu"):
        raise ValueError("u_op_e_sum: act must be None or 'relu', got %r" % (act,))
    if (op, act) not in _OPS:
        raise ValueError("u_op_e_sum: act='relu' goes with op='add' only (relu(x * e) is not built)")
    if reduce not in ("sum", "mean"):
        raise ValueError("u_op_e_sum: reduce must be 'sum' or 'mean', got %r (max / min over the messages are not built)" % (reduce,))
    _dtype_code(x)
    _dtype_code(e)
    if x.dtype != e.dtype:
        raise TypeError("u_op_e_sum: x and e must have one dtype, got %s and %s" % (x.dtype, e.dtype))
    if x.dim() != 2 or x.shape[0] != graph.n_cols:
        raise ValueError("u_op_e_sum: x must be a matrix of %d rows, got %s" % (graph.n_cols, tuple(x.shape)))
    if e.dim() != 2 or e.shape[0] != graph.nnz:
        raise ValueError("u_op_e_sum: e must be [nnz, F] with nnz = %d, got %s" % (graph.nnz, tuple(e.shape)))
    if e.shape[1] != x.shape[1]:
        raise ValueError("u_op_e_sum: e has %d columns and x %d: edge features of another width than the node features' are not "
                         "built (project them first, as nn.GINE does)" % (e.shape[1], x.shape[1]))
    F, vec = x.shape[1], epv(x.dtype)
    if F == 0 or F % vec:
        raise ValueError("u_op_e_sum: the width %d is not a whole number of 16-byte vectors (%d columns of %s); the layers pad "
                         "their widths with zero columns" % (F, vec, x.dtype))
    _require_cuda(x, e, graph.rowptr)
    if graph.n_rows == 0 or graph.nnz == 0:     # nothing to gather: zeros, with zero gradients
        return x.new_zeros((graph.n_rows, F)) + 0 * (x.sum() + e.sum())
    return _UOpESum.apply(x, e, graph, _OPS[(op, act)], mean_scale(graph) if reduce == "mean" else None)


def u_add_e_sum(graph, x, e, act=None, reduce="sum"):
    return u_op_e_sum(graph, x, e, "add", act, reduce)


def u_mul_e_sum_full(graph, x, e, reduce="sum"):
    return u_op_e_sum(graph, x, e, "mul", None, reduce)


def edge_graph_from_coo(src, dst, edge_feat, n_dst=None, n_src=None):
    """(CSRGraph, edge_feat in the graph's entry order, order) from COO pairs: a stable sort by (dst, src).  Nothing is coalesced:
    parallel edges stay separate entries with their own feature rows, in their order of appearance, as in DGL.  order: entry k of the
    graph is edge order[k] of the input, so that other per-edge data can follow (data[order])."""
    src, dst = src.reshape(-1).to(torch.int64), dst.reshape(-1).to(torch.int64)
    if src.numel() != dst.numel() or edge_feat.dim() != 2 or edge_feat.shape[0] != src.numel():
        raise ValueError("src, dst and the rows of edge_feat must have one entry per edge")
    n_src = int(n_src) if n_src is not None else (int(src.max()) + 1 if src.numel() else 0)
    n_dst = int(n_dst) if n_dst is not None else (int(dst.max()) + 1 if dst.numel() else 0)
    if n_src >= 2 ** 31:
        raise ValueError("column ids must fit int32")
    if src.numel() and (int(src.min()) < 0 or int(src.max()) >= n_src or int(dst.min()) < 0 or int(dst.max()) >= n_dst):
        raise ValueError("src / dst out of range for a %d x %d graph" % (n_dst, n_src))
    order = torch.sort(dst * max(n_src, 1) + src, stable=True)[1]
    counts = torch.bincount(dst, minlength=n_dst) if dst.numel() else torch.zeros(n_dst, dtype=torch.int64, device=dst.device)
    rowptr = torch.zeros(n_dst + 1, dtype=torch.int64, device=dst.device)
    torch.cumsum(counts, 0, out=rowptr[1:])
    graph = CSRGraph(rowptr, src[order].to(torch.int32), None, n_dst, n_src)
    return graph, edge_feat[order.to(edge_feat.device)], order
