"""GATv2 aggregation ("How Attentive are Graph Attention Networks?"; DGL's GATv2Conv after the two linear maps): csrc/gatv2.hip.

    gatv2_aggregate(graph, xl, xr, attn, heads, negative_slope=0.2) -> out [n_dst, heads * D]

Per head h of width D, over the entries j of row i of `graph` (a CSRGraph, n_dst rows gathering from n_src columns; rectangular
blocks allowed; edge values are ignored, duplicate entries are separate edges):

    z_ij = xl[j, h] + xr[i, h]      e_ij = attn[h] . leaky_relu(z_ij)      alpha = softmax_j e_ij      out[i, h] = sum_j alpha_ij xl[j, h]

An empty row gives 0.  xl [n_src, heads * D] and xr [n_dst, heads * D] are fp32 or bf16 on the GPU (fp32 accumulation), attn is
[heads, D]; D must be a whole number of 16-byte vectors (4 fp32 / 8 bf16 columns -- nn.GATv2Conv pads its heads).  `xr is xl` is
allowed on a square graph (shared weights): autograd adds the two gradients.

One autograd node over three gather passes, all behind dgll_hip_gatv2_pass: the forward (one gather of xl_j per edge serves score and
value; online softmax; leaves lse [n_dst, heads]), and for the backward a pass over the rows of A (grad_xr, {lse, delta} per row, one
grad_attn partial per workgroup, summed in workgroup order by a small second kernel) and one over the rows of A^T (grad_xl;
graph.transpose(), the cached structure).  Nothing is stored per edge, nothing is read back, no float atomics: reruns give the same bits and the step can
be captured.  There is no CPU implementation here: a CPU tensor raises.
"""
import ctypes as C

import torch

from . import _lib
from .graph import CSRGraph
from .ops import _dtype_code, epv, _require_cuda, alloc_features, as_rows16

LONG_ROW = _lib.GATV2_LONG_ROW      # rows with more entries are swept by a whole workgroup
_MAX_PARTIALS = 2048                # workgroups of the rows pass = rows of the grad_attn partials


def _launch(kind, graph, heads, D, slope, xl, xr, attn, out, grad_out=None, lse=None, lse_delta=None, part=None, dattn=None):
    d = _lib.Gatv2Desc()
    d.pass_, d.dtype = kind, _dtype_code(xl)
    d.rowptr, d.col, d.n_rows, d.n_cols = graph.rowptr.data_ptr(), graph.col.data_ptr(), graph.n_rows, graph.n_cols
    d.heads, d.D, d.slope = heads, D, slope
    d.xl, d.ld_xl, d.xr, d.ld_xr, d.attn = xl.data_ptr(), xl.stride(0), xr.data_ptr(), xr.stride(0), attn.data_ptr()
    d.grad_out, d.ld_grad_out = _lib.ptr(grad_out), _lib.pitch(grad_out)
    d.out, d.ld_out = out.data_ptr(), out.stride(0)
    d.lse, d.lse_delta = _lib.ptr(lse), _lib.ptr(lse_delta)
    d.dattn_part, d.dattn_blocks, d.dattn = _lib.ptr(part), 0 if part is None else part.shape[0], _lib.ptr(dattn)
    _lib.launch("dgll_hip_gatv2_pass", xl.device, C.byref(d),
                tag=lambda: ("gatv2_" + ("fwd", "rows", "cols")[kind], heads, D, str(xl.dtype), graph.nnz))


def gatv2_forward_raw(graph, xl, xr, attn, heads, slope):
    """(out, lse) with no autograd; xl / xr as as_rows16 leaves them, attn fp32 [heads, D] contiguous."""
    D = attn.shape[1]
    out = alloc_features(graph.n_rows, heads * D, xl.dtype, xl.device, pad_to=epv(xl.dtype))
    lse = torch.empty((graph.n_rows, heads), dtype=torch.float32, device=xl.device)
    _launch(_lib.GATV2_FORWARD, graph, heads, D, slope, xl, xr, attn, out, lse=lse)
    return out, lse


def gatv2_backward_raw(graph, xl, xr, attn, heads, slope, lse, g, need_xl=True):
    """(grad_xl or None, grad_xr, grad_attn fp32 [heads, D]) from the output gradient g (rows on a 16-byte pitch)."""
    D = attn.shape[1]
    vec = epv(xl.dtype)
    dxr = alloc_features(graph.n_rows, heads * D, xl.dtype, xl.device, pad_to=vec)
    lse_delta = torch.empty((graph.n_rows, 2 * heads), dtype=torch.float32, device=xl.device)
    part = torch.empty((max(1, min(_MAX_PARTIALS, -(-graph.n_rows // 16))), heads * D), dtype=torch.float32, device=xl.device)
    dattn = torch.empty((heads, D), dtype=torch.float32, device=xl.device)      # the partials summed in workgroup order, by the same call
    _launch(_lib.GATV2_ROWS, graph, heads, D, slope, xl, xr, attn, dxr, grad_out=g, lse=lse, lse_delta=lse_delta, part=part, dattn=dattn)
    dxl = None
    if need_xl:
        gt, _ = graph.transpose()
        dxl = alloc_features(graph.n_cols, heads * D, xl.dtype, xl.device, pad_to=vec)
        _launch(_lib.GATV2_TRANSPOSED, gt, heads, D, slope, xl, xr, attn, dxl, grad_out=g, lse_delta=lse_delta)
    return dxl, dxr, dattn


class _Gatv2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xl, xr, attn, graph, heads, slope):
        shared = xr.data_ptr() == xl.data_ptr() and xr.shape == xl.shape and xr.stride() == xl.stride()
        xlr = as_rows16(xl.detach())
        xrr = xlr if shared else as_rows16(xr.detach())
        a32 = attn.detach().to(torch.float32).contiguous()
        out, lse = gatv2_forward_raw(graph, xlr, xrr, a32, heads, slope)
        ctx.graph, ctx.heads, ctx.slope, ctx.attn_dtype = graph, heads, slope, attn.dtype
        ctx.save_for_backward(xlr, xrr, a32, lse)
        return out

    @staticmethod
    def backward(ctx, g):
        xlr, xrr, a32, lse = ctx.saved_tensors
        need_xl, need_xr, need_attn = ctx.needs_input_grad[:3]
        if not (need_xl or need_xr or need_attn):
            return None, None, None, None, None, None
        if g.dtype != xlr.dtype:
            g = g.to(xlr.dtype)
        dxl, dxr, dattn = gatv2_backward_raw(ctx.graph, xlr, xrr, a32, ctx.heads, ctx.slope, lse, as_rows16(g), need_xl=need_xl)
        return dxl, (dxr if need_xr else None), (dattn.to(ctx.attn_dtype) if need_attn else None), None, None, None


def gatv2_aggregate(graph, xl, xr, attn, heads, negative_slope=0.2):
    """out[i, h] = sum_j softmax_j(attn[h] . leaky_relu(xl[j, h] + xr[i, h])) xl[j, h]; see the module text."""
    if not isinstance(graph, CSRGraph):
        raise TypeError("gatv2_aggregate expects a CSRGraph (use dgll_amd.graph.as_csr_graph for torch sparse tensors)")
    _require_cuda(xl, xr, attn, graph.rowptr)
    _dtype_code(xl)
    heads = int(heads)
    if xl.dim() != 2 or xr.dim() != 2 or xl.dtype != xr.dtype or xl.shape[1] != xr.shape[1]:
        raise ValueError("xl [n_src, heads * D] and xr [n_dst, heads * D] must be matrices of one dtype and width")
    if xl.shape[0] != graph.n_cols or xr.shape[0] != graph.n_rows:
        raise ValueError("xl has %d rows and xr %d, but the graph gathers %d sources into %d destinations"
                         % (xl.shape[0], xr.shape[0], graph.n_cols, graph.n_rows))
    if attn.dim() != 2 or heads < 1 or attn.shape[0] != heads or heads * attn.shape[1] != xl.shape[1]:
        raise ValueError("attn must be [heads, D] with heads * D = %d columns" % xl.shape[1])
    D = int(attn.shape[1])
    if D == 0 or D % epv(xl.dtype):
        raise ValueError("D = %d is not a whole number of 16-byte vectors (%d columns of %s); nn.GATv2Conv pads its heads"
                         % (D, epv(xl.dtype), xl.dtype))
    if graph.n_rows == 0 or graph.nnz == 0:         # nothing to gather: zeros, with zero gradients
        return xl.new_zeros((graph.n_rows, heads * D)) + 0 * (xl.sum() + xr.sum() + attn.sum().to(xl.dtype))
    return _Gatv2.apply(xl, xr, attn, graph, heads, float(negative_slope))
