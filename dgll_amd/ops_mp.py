"""Per-edge message passing (DGL's edge_softmax and its generalized SpMM / SDDMM operators): csrc/mp_ops.hip.

    edge_softmax(graph, logits, norm_by="dst")      logits [nnz, H] or [nnz] fp32, in graph's entry order -> same shape
    u_mul_e_sum(graph, x, w, heads=None)            x [n_src, H * D] fp32 / bf16, w [nnz, H] fp32 -> [n_dst, H * D] of x.dtype
    u_dot_v(graph, x_src, y_dst, heads=1)           -> [nnz, H] fp32: <x[col_k, h], y[row_k, h]>
    u_add_v(graph, a_src, b_dst)                    a [n_src, H], b [n_dst, H] fp32 -> [nnz, H]: a[col_k] + b[row_k]
    copy_e_sum(graph, w, norm_by="dst")             [nnz, H] -> [n_dst, H]  ("src": [n_src, H])

`graph` is a CSRGraph (n_dst rows gathering from n_src columns; rectangular blocks allowed; edge values are ignored, duplicate
entries are separate edges); per-edge tensors are fp32 in the graph's entry order (entry k of row i is edge col[k] -> i).  These are
the building blocks UNDER the attention layers: a layer of one's own is a few lines of them (examples/message_passing/train.py
writes GAT that way, nn.AGNNConv is built on them), every gradient is exact autograd, and `edge_softmax` output is what
`get_attention=True` would return.

What it costs: the fused layers (ops_attn.sparse_attention, ops_gatv2, the GAT passes) store NOTHING per edge; here every per-edge
tensor is a real [nnz, H] fp32 array -- 4 * nnz * H bytes each, 3.96 GB at the products size (123.7 M entries) with 8 heads, and an
attention layer holds three or four of them for its backward.  The fused layers stay the fast path; this is the general one.

Each operator is one autograd node, and the family is closed under differentiation: every backward is another pass of the same
entry point, dgll_hip_mp_pass, over A or over A^T (graph.transpose(), the cached structure) with `perm`, so that per-edge data
never leaves A's entry order:

    edge_softmax   EDGE_SOFTMAX_BWD (alpha, grad); norm_by="src": both passes over A^T with perm
    u_mul_e_sum    grad_x = U_MUL_E_SUM over A^T with perm, the output gradient in x's place; grad_w = U_DOT_V(x, grad_out) over A
    u_dot_v        grad_y = U_MUL_E_SUM over A, weights g; grad_x = U_MUL_E_SUM over A^T with perm, y in x's place
    u_add_v        grad_b = E_SUM over A; grad_a = E_SUM over A^T with perm
    copy_e_sum     U_ADD_V with one side NULL

No float atomics (reruns give the same bits, unlike index_add), nothing allocated by a pass, synchronised or read back (the step
can be captured), fp32 accumulation.  Gradients nobody needs are not computed.  There is no CPU implementation here: a CPU tensor
raises.
"""
import ctypes as C

import torch

from . import _lib
from .graph import CSRGraph
from .ops import _dtype_code, epv, _require_cuda, alloc_features, as_rows16

LONG_ROW = _lib.MP_LONG_ROW         # rows with more entries are swept by a whole workgroup
_MAX_VECTORS = 64                   # a head fits a wavefront's lanes: D / EPV <= 64
_TAGS = ("mp_edge_softmax", "mp_edge_softmax_bwd", "mp_e_sum", "mp_u_add_v", "mp_u_mul_e_sum", "mp_u_dot_v")


def _ld(t):
    """row pitch of a per-edge or per-row array (a single row's stride says nothing); 0 for None"""
    return 0 if t is None else max(t.stride(0), t.shape[1])


def _launch(kind, graph, perm, heads, D=0, dtype=_lib.F32, e=None, e2=None, e_out=None, x=None, y=None, out=None):
    """One pass over `graph` (A, or A^T with its perm).  Per-edge arrays [nnz, heads] fp32 contiguous; x / y / out with their pitches."""
    d = _lib.MpDesc()
    d.pass_, d.dtype = kind, dtype
    d.rowptr, d.col, d.perm = graph.rowptr.data_ptr(), graph.col.data_ptr(), _lib.ptr(perm)
    d.n_rows, d.n_cols, d.nnz, d.heads, d.D = graph.n_rows, graph.n_cols, graph.nnz, heads, D
    d.e, d.ld_e, d.e2, d.ld_e2, d.e_out, d.ld_e_out = _lib.ptr(e), _ld(e), _lib.ptr(e2), _ld(e2), _lib.ptr(e_out), _ld(e_out)
    d.x, d.ld_x, d.y, d.ld_y, d.out, d.ld_out = _lib.ptr(x), _ld(x), _lib.ptr(y), _ld(y), _lib.ptr(out), _ld(out)
    _lib.launch("dgll_hip_mp_pass", graph.rowptr.device, C.byref(d), tag=lambda: (_TAGS[kind], heads, D, graph.nnz))


def _over(graph, transposed):
    """(the pass's CSR, perm): A itself, or A^T with the map of its entries to A's."""
    return graph.transpose() if transposed else (graph, None)


def _edge_empty(graph, heads, device):
    return torch.empty((graph.nnz, heads), dtype=torch.float32, device=device)


def _edge32(g):
    """a per-edge or per-row fp32 gradient as the passes read it"""
    return g.to(torch.float32).contiguous()


# ---- raw passes (no autograd, no checks): what the autograd nodes and tools/mp_bench.py call --------------------------------------
def edge_softmax_raw(graph, e, transposed=False):
    gr, perm = _over(graph, transposed)
    out = torch.empty_like(e)
    _launch(_lib.MP_EDGE_SOFTMAX, gr, perm, e.shape[1], e=e, e_out=out)
    return out


def edge_softmax_bwd_raw(graph, alpha, g, transposed=False):
    gr, perm = _over(graph, transposed)
    out = torch.empty_like(alpha)
    _launch(_lib.MP_EDGE_SOFTMAX_BWD, gr, perm, alpha.shape[1], e=alpha, e2=g, e_out=out)
    return out


def e_sum_raw(graph, w, transposed=False):
    gr, perm = _over(graph, transposed)
    out = torch.empty((gr.n_rows, w.shape[1]), dtype=torch.float32, device=w.device)
    _launch(_lib.MP_E_SUM, gr, perm, w.shape[1], e=w, out=out)
    return out


def u_add_v_raw(graph, a, b, heads, transposed=False):
    """e_out[s(k)] = a[col_k] + b[row_k] over the pass's CSR; either side may be None (0)."""
    gr, perm = _over(graph, transposed)
    out = _edge_empty(graph, heads, graph.rowptr.device)
    _launch(_lib.MP_U_ADD_V, gr, perm, heads, e_out=out, x=a, y=b)
    return out


def u_mul_e_sum_raw(graph, x, w, heads, transposed=False):
    """x (rows on a 16-byte pitch) gathered by the pass's CSR, weighted by w [nnz, heads] at the entries' slots."""
    gr, perm = _over(graph, transposed)
    out = alloc_features(gr.n_rows, x.shape[1], x.dtype, x.device, pad_to=epv(x.dtype))
    _launch(_lib.MP_U_MUL_E_SUM, gr, perm, heads, x.shape[1] // heads, _dtype_code(x), e=w, x=x, out=out)
    return out


def u_dot_v_raw(graph, x, y, heads):
    out = _edge_empty(graph, heads, x.device)
    _launch(_lib.MP_U_DOT_V, graph, None, heads, x.shape[1] // heads, _dtype_code(x), e_out=out, x=x, y=y)
    return out


# ---- autograd nodes ----------------------------------------------------------------------------------------------------------------
class _EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, graph, by_src):
        alpha = edge_softmax_raw(graph, e.detach().contiguous(), by_src)
        ctx.graph, ctx.by_src = graph, by_src
        ctx.save_for_backward(alpha)
        return alpha

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        (alpha,) = ctx.saved_tensors
        return edge_softmax_bwd_raw(ctx.graph, alpha, _edge32(g), ctx.by_src), None, None


class _UMulESum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, graph, heads):
        xr, wr = as_rows16(x.detach()), w.detach().contiguous()
        ctx.graph, ctx.heads = graph, heads
        ctx.save_for_backward(xr, wr)
        return u_mul_e_sum_raw(graph, xr, wr, heads)

    @staticmethod
    def backward(ctx, g):
        xr, wr = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[:2]
        if not (need_x or need_w):
            return None, None, None, None
        gr = as_rows16(g if g.dtype == xr.dtype else g.to(xr.dtype))
        gx = u_mul_e_sum_raw(ctx.graph, gr, wr, ctx.heads, transposed=True) if need_x else None
        gw = u_dot_v_raw(ctx.graph, xr, gr, ctx.heads) if need_w else None
        return gx, gw, None, None


class _UDotV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, graph, heads):
        xr, yr = as_rows16(x.detach()), as_rows16(y.detach())
        ctx.graph, ctx.heads = graph, heads
        ctx.save_for_backward(xr, yr)
        return u_dot_v_raw(graph, xr, yr, heads)

    @staticmethod
    def backward(ctx, g):
        xr, yr = ctx.saved_tensors
        need_x, need_y = ctx.needs_input_grad[:2]
        if not (need_x or need_y):
            return None, None, None, None
        g = _edge32(g)
        gx = u_mul_e_sum_raw(ctx.graph, yr, g, ctx.heads, transposed=True) if need_x else None
        gy = u_mul_e_sum_raw(ctx.graph, xr, g, ctx.heads) if need_y else None
        return gx, gy, None, None


class _UAddV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, graph):
        ctx.graph = graph
        return u_add_v_raw(graph, a.detach().contiguous(), b.detach().contiguous(), a.shape[1])

    @staticmethod
    def backward(ctx, g):
        need_a, need_b = ctx.needs_input_grad[:2]
        if not (need_a or need_b):
            return None, None, None
        g = _edge32(g)
        ga = e_sum_raw(ctx.graph, g, transposed=True) if need_a else None
        gb = e_sum_raw(ctx.graph, g) if need_b else None
        return ga, gb, None


class _CopyESum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, graph, by_src):
        ctx.graph, ctx.by_src = graph, by_src
        return e_sum_raw(graph, w.detach().contiguous(), by_src)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        g = _edge32(g)          # the gradient of the pass's own rows, copied to every entry of the row: the row side of U_ADD_V
        return u_add_v_raw(ctx.graph, None, g, g.shape[1], ctx.by_src), None, None


# ---- the public operators ----------------------------------------------------------------------------------------------------------
def _graph_of(graph, name):
    if not isinstance(graph, CSRGraph):
        raise TypeError("%s expects a CSRGraph (use dgll_amd.graph.as_csr_graph for torch sparse tensors)" % name)
    return graph


def _per_edge(graph, t, name, what):
    """t as [nnz, H] and whether it came as [nnz]"""
    if t.dtype != torch.float32:
        raise TypeError("%s: %s is per-edge data and must be float32, got %s" % (name, what, t.dtype))
    flat = t.dim() == 1
    if flat:
        t = t.unsqueeze(1)
    if t.dim() != 2 or t.shape[0] != graph.nnz or t.shape[1] < 1:
        raise ValueError("%s: %s must be [nnz, H] (or [nnz]) with nnz = %d, got %s" % (name, what, graph.nnz, tuple(t.shape)))
    return t, flat


def _norm_by(norm_by, name):
    if norm_by not in ("dst", "src"):
        raise ValueError("%s: norm_by must be 'dst' or 'src', got %r" % (name, norm_by))
    return norm_by == "src"


def _node_matrix(t, rows, heads, name, what):
    """checks t [rows, heads * D] of a kernel dtype; returns D"""
    _dtype_code(t)
    if t.dim() != 2 or t.shape[0] != rows:
        raise ValueError("%s: %s must be a matrix of %d rows, got %s" % (name, what, rows, tuple(t.shape)))
    if heads < 1 or t.shape[1] % heads:
        raise ValueError("%s: heads = %d does not divide the %d columns of %s" % (name, heads, t.shape[1], what))
    D, vec = t.shape[1] // heads, epv(t.dtype)
    if D == 0 or D % vec:
        raise ValueError("%s: D = %d is not a whole number of 16-byte vectors (%d columns of %s); the layers pad their heads"
                         % (name, D, vec, t.dtype))
    if D // vec > _MAX_VECTORS:
        raise ValueError("%s: D = %d: a head may span at most %d columns of %s (64 16-byte vectors)" % (name, D, _MAX_VECTORS * vec, t.dtype))
    return D


def _per_row(t, rows, name, what):
    if t.dtype != torch.float32:
        raise TypeError("%s: %s must be float32, got %s" % (name, what, t.dtype))
    if t.dim() != 2 or t.shape[0] != rows or t.shape[1] < 1:
        raise ValueError("%s: %s must be [%d, H], got %s" % (name, what, rows, tuple(t.shape)))


def _nothing(graph):
    return graph.n_rows == 0 or graph.nnz == 0


def edge_softmax(graph, logits, norm_by="dst"):
    """softmax of logits [nnz, H] (or [nnz]) over the entries of each row (norm_by="dst") or of each column ("src"), max-subtracted.
    An entry of -inf gives 0; a row of -inf alone gives zeros."""
    graph = _graph_of(graph, "edge_softmax")
    e, flat = _per_edge(graph, logits, "edge_softmax", "logits")
    by_src = _norm_by(norm_by, "edge_softmax")
    _require_cuda(logits, graph.rowptr)
    out = e * 0 if _nothing(graph) else _EdgeSoftmax.apply(e, graph, by_src)
    return out.squeeze(1) if flat else out


def u_mul_e_sum(graph, x, w, heads=None):
    """out[i, h] = sum over the entries k of row i of w[k, h] * x[col_k, h]; heads defaults to w's columns."""
    graph = _graph_of(graph, "u_mul_e_sum")
    w, _ = _per_edge(graph, w, "u_mul_e_sum", "w")
    heads = w.shape[1] if heads is None else int(heads)
    if heads != w.shape[1]:
        raise ValueError("u_mul_e_sum: w has %d columns for %d heads" % (w.shape[1], heads))
    _node_matrix(x, graph.n_cols, heads, "u_mul_e_sum", "x")
    _require_cuda(x, w, graph.rowptr)
    if _nothing(graph):         # nothing to gather: zeros, with zero gradients
        return x.new_zeros((graph.n_rows, x.shape[1])) + 0 * (x.sum() + w.sum().to(x.dtype))
    return _UMulESum.apply(x, w, graph, heads)


def u_dot_v(graph, x_src, y_dst, heads=1):
    """[nnz, H] fp32: <x_src[col_k, h], y_dst[row_k, h]> for every entry k, products and sums in fp32."""
    graph = _graph_of(graph, "u_dot_v")
    heads = int(heads)
    _node_matrix(x_src, graph.n_cols, heads, "u_dot_v", "x_src")
    _node_matrix(y_dst, graph.n_rows, heads, "u_dot_v", "y_dst")
    if x_src.dtype != y_dst.dtype or x_src.shape[1] != y_dst.shape[1]:
        raise ValueError("u_dot_v: x_src and y_dst must be matrices of one dtype and width")
    _require_cuda(x_src, y_dst, graph.rowptr)
    if _nothing(graph):
        return torch.zeros((graph.nnz, heads), dtype=torch.float32, device=x_src.device) + 0 * (x_src.sum() + y_dst.sum()).float()
    return _UDotV.apply(x_src, y_dst, graph, heads)


def u_add_v(graph, a_src, b_dst):
    """[nnz, H]: a_src[col_k] + b_dst[row_k] for every entry k."""
    graph = _graph_of(graph, "u_add_v")
    _per_row(a_src, graph.n_cols, "u_add_v", "a_src")
    _per_row(b_dst, graph.n_rows, "u_add_v", "b_dst")
    if a_src.shape[1] != b_dst.shape[1]:
        raise ValueError("u_add_v: a_src has %d columns and b_dst %d" % (a_src.shape[1], b_dst.shape[1]))
    _require_cuda(a_src, b_dst, graph.rowptr)
    if _nothing(graph):
        return a_src.new_zeros((graph.nnz, a_src.shape[1])) + 0 * (a_src.sum() + b_dst.sum())
    return _UAddV.apply(a_src, b_dst, graph)


def copy_e_sum(graph, w, norm_by="dst"):
    """[n_dst, H]: the sum of w over the entries of each row; norm_by="src": [n_src, H], over the entries of each column."""
    graph = _graph_of(graph, "copy_e_sum")
    w, _ = _per_edge(graph, w, "copy_e_sum", "w")
    by_src = _norm_by(norm_by, "copy_e_sum")
    _require_cuda(w, graph.rowptr)
    if _nothing(graph):
        return w.new_zeros((graph.n_cols if by_src else graph.n_rows, w.shape[1])) + 0 * w.sum()
    return _CopyESum.apply(w, graph, by_src)
