"""Edge-feature aggregation with the edge projection fused into the kernel (PyG's GINEConv(nn, edge_dim=) underneath):
csrc/edge_proj.hip.

    u_op_proj_e_sum(graph, x, a, weight, bias=None, op="add", act=None, reduce="sum")  -> [n_dst, F] of x's dtype
        x [n_src, F], a [nnz, De] of one dtype (De <= 16); weight [F, De] as torch.nn.Linear stores it, bias [F] or None

ops_ef.u_op_e_sum with e[k] = bias + a[k] @ weight.T, where e is never an array: each pass forms e_k per entry in registers, in
fp32, from the raw attributes a[k] (De values), by one device function (from bias, d ascending, one fused multiply-add per term), so
the relu of the forward and the gates of the backward see the same bits.  The per-edge memory of the whole op is a [nnz, De] (and
grad_a [nnz, De], only when a requires a gradient); nothing of [nnz, F] exists in the forward or the backward.  graph, op, act and
reduce are u_op_e_sum's (a CSRGraph, entry k of row i the edge col[k] -> i with the attribute row a[k], in the graph's entry order).

One autograd node; four passes of one entry point (dgll_hip_edge_proj_pass), each run only when a gradient that needs it is wanted:
FORWARD over A; COLS over A^T for grad_x (a read through the transpose's perm; for op "add" without relu grad_x reads neither x nor e
and is ops_ef's COLS pass as it is); PARAM over A for grad_weight and grad_bias: min(tiles, EFP_MAX_PARTIALS) workgroups take the
row tiles grid-stride, every lane keeps its (De + 1) sums per column over all of them, the workgroup merges its lane groups through
LDS in group order and writes one fp32 slab [De + 1, F], and the slabs are summed in slab order (torch.sum(0)): no float atomics, a
scratch that does not grow with nnz; DOTS over A for grad_a (De dot products over a row's lanes per entry).  The node saves x and a
only, and only when a wanted gradient reads them; weight and bias reach the kernels as fp32 [De, F] and [F] copies.  Gradients come
back in each input's own dtype and layout.  Nothing is allocated, synchronised or read back by a pass; fp32 accumulation.  There is
no CPU implementation here: a CPU tensor raises (nn.GINEConv has a host path of its own).

Not built: De > 16, max / min over the messages, a filter network that ends in a nonlinearity (CFConv's), MFMA for the
[entries, De] x [De, F] product, the partitioned (multi-GPU) path.
"""
import ctypes as C

import torch

from . import _lib, ops_ef
from .graph import CSRGraph
from .ops import _dtype_code, epv, _require_cuda, alloc_features, as_rows16
from .ops_ef import _OPS, mean_scale

LONG_ROW = _lib.EFP_LONG_ROW        # rows with more entries are swept by a whole workgroup
MAX_DE = _lib.EFP_MAX_DE
_TAGS = ("efp_forward", "efp_cols", "efp_param", "efp_dots")


def geometry(n_rows, width, dtype):
    """(tiles, col_blocks) of a pass over n_rows rows of `width` columns, as csrc/row_tiles.hpp's make_flat_geometry lays them out."""
    vpr = width // epv(dtype)
    lpr = 8
    while lpr < min(vpr, 64):
        lpr <<= 1
    groups = 4 * (64 // lpr)
    return -(-n_rows // groups), -(-vpr // lpr)


def _launch(kind, op, gr, perm, nnz, scale, ref, De, wt, b, x=None, a=None, g=None, out=None, gx=None, ga=None, part=None,
            slabs=None, partials=0):
    """One pass over `gr` (A, or A^T with its perm); `ref` gives the dtype and the width."""
    d = _lib.EdgeProjDesc()
    d.pass_, d.dtype, d.op, d.De = kind, _dtype_code(ref), op, De
    d.rowptr, d.col, d.perm = gr.rowptr.data_ptr(), gr.col.data_ptr(), _lib.ptr(perm)
    d.n_rows, d.n_cols, d.nnz, d.F, d.scale = gr.n_rows, gr.n_cols, nnz, ref.shape[1], _lib.ptr(scale)
    d.x, d.ld_x, d.a, d.ld_a, d.grad_out, d.ld_grad_out = _lib.ptr(x), _lib.pitch(x), _lib.ptr(a), _lib.pitch(a), _lib.ptr(g), _lib.pitch(g)
    d.weight, d.bias = _lib.ptr(wt), _lib.ptr(b)
    d.out, d.ld_out, d.grad_x, d.ld_grad_x = _lib.ptr(out), _lib.pitch(out), _lib.ptr(gx), _lib.pitch(gx)
    d.grad_a, d.ld_grad_a, d.dots_part, d.slabs, d.partials = _lib.ptr(ga), _lib.pitch(ga), _lib.ptr(part), _lib.ptr(slabs), partials
    _lib.launch("dgll_hip_edge_proj_pass", gr.rowptr.device, C.byref(d), tag=lambda: (_TAGS[kind], op, d.F, De, nnz))


def kernel_weights(weight, bias):
    """(weight as fp32 [De, F] contiguous, bias as fp32 [F] or None): what the passes read."""
    wt = weight.detach().to(torch.float32).t().contiguous()
    return wt, None if bias is None else bias.detach().to(torch.float32).contiguous()


# ---- raw passes (no autograd, no checks): what the autograd node, tools/edge_proj_bench.py and the tests call ---------------------------
# x, a, g: matrices with rows on a 16-byte pitch (a: [nnz, De], whatever its pitch holds past De); wt, b: kernel_weights(); op: an
# _lib.EF_* code; scale: fp32 [n_dst] or None.  Operands the (pass, op) does not read are not passed on, whatever the caller gave.
def forward_raw(graph, x, a, wt, b, op, scale=None):
    out = alloc_features(graph.n_rows, x.shape[1], x.dtype, x.device, pad_to=epv(x.dtype))
    _launch(_lib.EFP_FORWARD, op, graph, None, graph.nnz, scale, x, wt.shape[0], wt, b, x=x, a=a, out=out)
    return out


def cols_raw(graph, x, a, wt, b, g, op, scale=None):
    """grad_x [n_src, F] over graph.transpose()."""
    if op == _lib.EF_ADD:               # reads neither x nor e: the edge-feature pass as it is
        return ops_ef.cols_raw(graph, None, None, g, op, scale)
    gt, perm = graph.transpose()
    gx = alloc_features(gt.n_rows, g.shape[1], g.dtype, g.device, pad_to=epv(g.dtype))
    _launch(_lib.EFP_COLS, op, gt, perm, graph.nnz, scale, g, wt.shape[0], wt, b, x=x if op == _lib.EF_ADD_RELU else None, a=a, g=g, gx=gx)
    return gx


def param_raw(graph, x, a, wt, b, g, op, scale=None, want_a=False, want_w=True, partials=None):
    """(grad_wt fp32 [De, F], grad_b fp32 [F], grad_a [nnz, De] of g's dtype in the graph's entry order): the first two None without
    want_w, the last None without want_a.  partials: the workgroups (and slabs) of the PARAM pass, min(tiles, EFP_MAX_PARTIALS) when
    None."""
    De, F, relu = wt.shape[0], g.shape[1], op == _lib.EF_ADD_RELU
    tiles, col_blocks = geometry(graph.n_rows, F, g.dtype)
    xs = x if op != _lib.EF_ADD else None
    gw = gb = ga = None
    if want_w:
        partials = min(tiles, _lib.EFP_MAX_PARTIALS) if partials is None else partials
        slabs = torch.empty((partials, De + 1, F), dtype=torch.float32, device=g.device)
        _launch(_lib.EFP_PARAM, op, graph, None, graph.nnz, scale, g, De, wt if relu else None, b if relu else None, x=xs, a=a, g=g,
                slabs=slabs, partials=partials)
        total = slabs.sum(0)
        gw, gb = total[:De], total[De]
    if want_a:
        part = None
        if col_blocks == 1:
            ga = alloc_features(graph.nnz, De, g.dtype, g.device, pad_to=epv(g.dtype))
        else:
            part = torch.empty((col_blocks, graph.nnz, De), dtype=torch.float32, device=g.device)
        _launch(_lib.EFP_DOTS, op, graph, None, graph.nnz, scale, g, De, wt, b if relu else None, x=xs, a=a if relu else None, g=g,
                ga=ga, part=part)
        if part is not None:            # the column blocks' partial dots, in block order
            acc = part[0]
            for blk in range(1, col_blocks):
                acc = acc + part[blk]
            ga = acc.to(g.dtype)
    return gw, gb, ga


class _UOpProjESum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, weight, bias, graph, op, scale):
        xr, ar = as_rows16(x.detach()), as_rows16(a.detach())
        wt, b = kernel_weights(weight, bias)
        need_x, need_a, need_w, need_b = ctx.needs_input_grad[:4]
        need_p = need_w or need_b
        ctx.graph, ctx.op, ctx.scale, ctx.wt, ctx.b = graph, op, scale, wt, b
        ctx.param_dtypes = (weight.dtype, None if bias is None else bias.dtype)
        # "add": grad_x reads nothing and only PARAM reads a; the gate of "add_relu" reads both in every pass; "mul" reads a for
        # grad_x and x for the other three
        keep_x = (need_x and op == _lib.EF_ADD_RELU) or ((need_a or need_p) and op != _lib.EF_ADD)
        keep_a = (need_x and op != _lib.EF_ADD) or need_p or (need_a and op == _lib.EF_ADD_RELU)
        ctx.has = (keep_x, keep_a)
        ctx.save_for_backward(*(t for t, k in ((xr, keep_x), (ar, keep_a)) if k))
        return forward_raw(graph, xr, ar, wt, b, op, scale)

    @staticmethod
    def backward(ctx, g):
        need_x, need_a, need_w, need_b = ctx.needs_input_grad[:4]
        if not (need_x or need_a or need_w or need_b):
            return (None,) * 7
        saved = list(ctx.saved_tensors)
        xr, ar = (saved.pop(0) if h else None for h in ctx.has)
        gr = as_rows16(g)
        gx = cols_raw(ctx.graph, xr, ar, ctx.wt, ctx.b, gr, ctx.op, ctx.scale) if need_x else None
        gw = gb = ga = None
        if need_a or need_w or need_b:
            gw, gb, ga = param_raw(ctx.graph, xr, ar, ctx.wt, ctx.b, gr, ctx.op, ctx.scale, want_a=need_a, want_w=need_w or need_b)
        w_dtype, b_dtype = ctx.param_dtypes
        gw = gw.t().to(w_dtype).contiguous() if need_w else None
        gb = gb.to(b_dtype) if need_b else None
        return gx, ga, gw, gb, None, None, None


def u_op_proj_e_sum(graph, x, a, weight, bias=None, op="add", act=None, reduce="sum"):
    """out[i] = reduce over the entries k of row i of act(x[col_k] op (bias + a[k] @ weight.T)) (module docstring)."""
    if not isinstance(graph, CSRGraph):
        raise TypeError("u_op_proj_e_sum expects a CSRGraph (use dgll_amd.graph.as_csr_graph for torch sparse tensors)")
    if op not in ("add", "mul"):
        raise ValueError("u_op_proj_e_sum: op must be 'add' or 'mul', got %r" % (op,))
    if act not in (None, "relu"):
        raise ValueError("u_op_proj_e_sum: act must be None or 'relu', got %r" % (act,))
    if (op, act) not in _OPS:
        raise ValueError("u_op_proj_e_sum: act='relu' goes with op='add' only (relu(x * e) is not built)")
    if reduce not in ("sum", "mean"):
        raise ValueError("u_op_proj_e_sum: reduce must be 'sum' or 'mean', got %r (max / min over the messages are not built)" % (reduce,))
    _dtype_code(x)
    _dtype_code(a)
    if x.dtype != a.dtype:
        raise TypeError("u_op_proj_e_sum: x and a must have one dtype, got %s and %s" % (x.dtype, a.dtype))
    if x.dim() != 2 or x.shape[0] != graph.n_cols:
        raise ValueError("u_op_proj_e_sum: x must be a matrix of %d rows, got %s" % (graph.n_cols, tuple(x.shape)))
    if a.dim() != 2 or a.shape[0] != graph.nnz:
        raise ValueError("u_op_proj_e_sum: a must be [nnz, De] with nnz = %d, got %s" % (graph.nnz, tuple(a.shape)))
    F, De, vec = x.shape[1], a.shape[1], epv(x.dtype)
    if F == 0 or F % vec:
        raise ValueError("u_op_proj_e_sum: the width %d is not a whole number of 16-byte vectors (%d columns of %s); the layers pad "
                         "their widths with zero columns" % (F, vec, x.dtype))
    if not 1 <= De <= MAX_DE:
        raise ValueError("u_op_proj_e_sum: a has %d columns: the edge attribute width De must be in 1..%d (wider attributes: project "
                         "them first and use ops_ef.u_op_e_sum)" % (De, MAX_DE))
    if not torch.is_tensor(weight) or not weight.is_floating_point() or tuple(weight.shape) != (F, De):
        raise ValueError("u_op_proj_e_sum: weight must be a floating-point [F, De] = [%d, %d] matrix (torch.nn.Linear(De, F).weight), got %s"
                         % (F, De, tuple(weight.shape) if torch.is_tensor(weight) else type(weight).__name__))
    if bias is not None and (not torch.is_tensor(bias) or not bias.is_floating_point() or tuple(bias.shape) != (F,)):
        raise ValueError("u_op_proj_e_sum: bias must be None or a floating-point [F] = [%d] vector, got %s"
                         % (F, tuple(bias.shape) if torch.is_tensor(bias) else type(bias).__name__))
    _require_cuda(x, a, weight, bias, graph.rowptr)
    if graph.n_rows == 0 or graph.nnz == 0:     # nothing to gather: zeros, with zero gradients
        zero = x.sum() + a.sum() + weight.sum().to(x.dtype) + (0 if bias is None else bias.sum().to(x.dtype))
        return x.new_zeros((graph.n_rows, F)) + 0 * zero
    return _UOpProjESum.apply(x, a, weight, bias, graph, _OPS[(op, act)], mean_scale(graph) if reduce == "mean" else None)
