"""Typed-edge basis aggregation (R-GCN, DGL's RelGraphConv in its basis form): csrc/typed_spmm.hip.

    typed_spmm(graph, edges, x, coeff) -> Z [n_dst, B * F]

Every entry e = (j -> i) of `graph` (a CSRGraph, n_dst rows gathering from n_src columns; rectangular blocks allowed; duplicate
entries are separate edges, as in DGL) has a type r_e in [0, num_rels) and optionally a factor norm_e -- `edges`, a TypedEdges.  With
the coefficient table coeff fp32 [num_rels, B]:

    Z[i, b, :] = sum_e norm_e coeff[r_e, b] x[j_e, :]                (Z laid out [n_dst, B * F], basis-major blocks of width F)

so that R-GCN's sum_e norm_e x_j W_{r_e} with W_r = sum_b coeff[r, b] V_b is the dense product Z . stack(V_b).  x is fp32 or bf16 on
the GPU (fp32 accumulation); F must be a whole number of 16-byte vectors (4 fp32 / 8 bf16 columns -- the layer pads).

One autograd node over three gather passes, all behind dgll_hip_typed_spmm_pass: EXPAND (the forward: x_j gathered once per edge,
B accumulators), CONTRACT over the rows of A^T (grad x; graph.transpose(), the cached structure; skipped when x needs no gradient)
and, only when coeff needs a gradient, EDGE_DOTS: P[e, b] = <x_j, dZ[i, b, :]>, the one per-edge tensor of the feature, reduced per
type by the existing SpMM over the type-sorted structure (a type with millions of edges is a long row to it):
grad coeff[r, b] = sum_{e: r_e = r} norm_e P[e, b].  No float atomics anywhere: reruns give the same bits and the step can be
captured.  There is no CPU implementation here: a CPU tensor raises.
"""
import ctypes as C

import torch

from . import _lib
from .graph import CSRGraph
from .ops import _dtype_code, epv, _require_cuda, alloc_features, as_rows16, spmm_raw

LONG_ROW = _lib.TYPED_LONG_ROW          # rows with more entries are swept by a whole workgroup
COEFF_LDS = _lib.TYPED_COEFF_LDS        # the kernels stage coeff in LDS up to this many entries (num_rels * B), else read it from global memory
BASIS_BLOCK = _lib.TYPED_BASIS_BLOCK    # bases one launch block accumulates; more bases re-gather x once per block


class TypedEdges:
    """Per-edge data of one CSRGraph, in its CSR entry order: etypes (any integer dtype, kept as int32) in [0, num_rels) and an
    optional norm ([nnz] or [nnz, 1], kept as fp32).  check=True verifies the lengths and the range of the types -- one reduction and
    one read-back, here and nowhere in the step (the kernels clamp a type they address with, so a buffer corrupted later gives a
    wrong number, not a fault).  The A^T-order copies and the type-sorted structure of grad coeff are built on first use and kept."""

    def __init__(self, graph, etypes, num_rels, norm=None, check=True):
        if not isinstance(graph, CSRGraph):
            raise TypeError("TypedEdges expects a CSRGraph")
        num_rels = int(num_rels)
        if num_rels < 1:
            raise ValueError("num_rels must be >= 1, got %d" % num_rels)
        if etypes.is_floating_point() or etypes.dtype == torch.bool:
            raise TypeError("etypes must be an integer tensor, got %s" % etypes.dtype)
        etypes = etypes.reshape(-1)
        if norm is not None:
            norm = norm.reshape(-1) if norm.dim() != 2 or norm.shape[1] == 1 else norm
        if check:
            if etypes.numel() != graph.nnz:
                raise ValueError("etypes has %d entries but the graph has %d" % (etypes.numel(), graph.nnz))
            if norm is not None and (norm.dim() != 1 or norm.numel() != graph.nnz):
                raise ValueError("norm must be [nnz] or [nnz, 1] with nnz = %d, got %s" % (graph.nnz, tuple(norm.shape)))
            if etypes.numel():
                lo, hi = (int(v) for v in torch.stack((etypes.min(), etypes.max())).tolist())
                if lo < 0 or hi >= num_rels:
                    raise ValueError("edge types must lie in [0, %d); found %d .. %d" % (num_rels, lo, hi))
        self.graph = graph
        self.num_rels = num_rels
        self.etypes = etypes.to(device=graph.device, dtype=torch.int32).contiguous()
        self.norm = None if norm is None else norm.detach().to(device=graph.device, dtype=torch.float32).contiguous()
        self._transposed = None
        self._by_type = None

    def transposed(self):
        """(etypes, norm or None) in the entry order of graph.transpose()."""
        if self._transposed is None:
            _, perm = self.graph.transpose()
            self._transposed = (self.etypes[perm].contiguous(), None if self.norm is None else self.norm[perm].contiguous())
        return self._transposed

    def by_type(self):
        """CSRGraph of num_rels rows over nnz columns: row r lists, by a stable sort, the entries of type r; its values are their
        norms (none without a norm).  An SpMM over it sums a per-edge matrix per type."""
        if self._by_type is None:
            order = torch.sort(self.etypes.to(torch.int64), stable=True)[1]
            counts = torch.bincount(self.etypes.to(torch.int64), minlength=self.num_rels)
            rowptr = torch.zeros(self.num_rels + 1, dtype=torch.int64, device=self.graph.device)
            torch.cumsum(counts, 0, out=rowptr[1:])
            val = None if self.norm is None else self.norm[order].contiguous()
            self._by_type = CSRGraph(rowptr, order.to(torch.int32), val, self.num_rels, self.graph.nnz, check=False)
        return self._by_type


def typed_graph_from_coo(src, dst, etypes, norm=None, num_src=None, num_dst=None, num_rels=None):
    """(CSRGraph, TypedEdges) from COO triples: a stable sort by (dst, src) that carries etypes / norm along.  Nothing is coalesced:
    parallel edges of different or equal type stay separate entries, in their order of appearance, as in DGL.  num_rels: the
    number of types, max(etypes) + 1 when not given."""
    src, dst = src.reshape(-1).to(torch.int64), dst.reshape(-1).to(torch.int64)
    etypes = etypes.reshape(-1)
    if not (src.numel() == dst.numel() == etypes.numel()):
        raise ValueError("src, dst and etypes must have one entry per edge")
    n_src = int(num_src) if num_src is not None else (int(src.max()) + 1 if src.numel() else 0)
    n_dst = int(num_dst) if num_dst is not None else (int(dst.max()) + 1 if dst.numel() else 0)
    if n_src >= 2 ** 31:
        raise ValueError("column ids must fit int32")
    if src.numel() and (int(src.min()) < 0 or int(src.max()) >= n_src or int(dst.min()) < 0 or int(dst.max()) >= n_dst):
        raise ValueError("src / dst out of range for a %d x %d graph" % (n_dst, n_src))
    order = torch.sort(dst * max(n_src, 1) + src, stable=True)[1]
    counts = torch.bincount(dst, minlength=n_dst) if dst.numel() else torch.zeros(n_dst, dtype=torch.int64, device=dst.device)
    rowptr = torch.zeros(n_dst + 1, dtype=torch.int64, device=dst.device)
    torch.cumsum(counts, 0, out=rowptr[1:])
    graph = CSRGraph(rowptr, src[order].to(torch.int32), None, n_dst, n_src)
    if norm is not None:
        norm = norm.reshape(-1)[order]
    if num_rels is None:
        num_rels = int(etypes.max()) + 1 if etypes.numel() else 1
    return graph, TypedEdges(graph, etypes[order], num_rels, norm)


def _launch(kind, graph, etype, norm, R, B, F, coeff, x=None, dz=None, out=None, p=None):
    ref = x if x is not None else dz
    d = _lib.TypedDesc()
    d.pass_, d.dtype = kind, _dtype_code(ref)
    d.rowptr, d.col, d.etype, d.norm = graph.rowptr.data_ptr(), graph.col.data_ptr(), _lib.ptr(etype), _lib.ptr(norm)
    d.n_rows, d.n_cols, d.R, d.B, d.F = graph.n_rows, graph.n_cols, R, B, F
    d.coeff = _lib.ptr(coeff)
    d.x, d.ld_x, d.dz, d.ld_dz = _lib.ptr(x), _lib.pitch(x), _lib.ptr(dz), _lib.pitch(dz)
    d.out, d.ld_out, d.p, d.ld_p = _lib.ptr(out), _lib.pitch(out), _lib.ptr(p), _lib.pitch(p)
    _lib.launch("dgll_hip_typed_spmm_pass", ref.device, C.byref(d),
                tag=lambda: ("typed_" + ("expand", "contract", "dots")[kind], F, B, str(ref.dtype), graph.nnz))


def _coeff32(coeff):
    return coeff.detach().to(torch.float32).contiguous()


def typed_spmm_forward_raw(graph, edges, x, coeff, out=None):
    """Z [n_dst, B * F] with no autograd; x as as_rows16 leaves it, coeff fp32 [num_rels, B] contiguous.  out: rows of a caller's
    buffer to write (16-byte pitch)."""
    B, F = coeff.shape[1], x.shape[1]
    z = alloc_features(graph.n_rows, B * F, x.dtype, x.device, pad_to=epv(x.dtype)) if out is None else out
    _launch(_lib.TYPED_EXPAND, graph, edges.etypes, edges.norm, edges.num_rels, B, F, coeff, x=x, out=z)
    return z


def typed_spmm_backward_raw(graph, edges, x, coeff, g, need_x=True, need_coeff=True):
    """(grad_x or None, grad_coeff fp32 [num_rels, B] or None) from the output gradient g [n_dst, B * F] (rows on a 16-byte pitch)."""
    B, F = coeff.shape[1], x.shape[1]
    dx = dc = None
    if need_x:
        gt, _ = graph.transpose()
        t_etypes, t_norm = edges.transposed()
        dx = alloc_features(graph.n_cols, F, x.dtype, x.device, pad_to=epv(x.dtype))
        _launch(_lib.TYPED_CONTRACT, gt, t_etypes, t_norm, edges.num_rels, B, F, coeff, dz=g, out=dx)
    if need_coeff:
        p = torch.empty((graph.nnz, (B + 3) // 4 * 4), dtype=torch.float32, device=x.device)
        _launch(_lib.TYPED_EDGE_DOTS, graph, None, None, edges.num_rels, B, F, None, x=x, dz=g, p=p)
        dc = spmm_raw(edges.by_type(), p)[:, :B]
    return dx, dc


class _TypedSpmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, coeff, graph, edges):
        xr, cf = as_rows16(x.detach()), _coeff32(coeff)
        z = typed_spmm_forward_raw(graph, edges, xr, cf)
        ctx.graph, ctx.edges, ctx.coeff_dtype = graph, edges, coeff.dtype
        ctx.save_for_backward(xr, cf)
        return z

    @staticmethod
    def backward(ctx, g):
        xr, cf = ctx.saved_tensors
        need_x, need_c = ctx.needs_input_grad[:2]
        if not (need_x or need_c):
            return None, None, None, None
        if g.dtype != xr.dtype:
            g = g.to(xr.dtype)
        dx, dc = typed_spmm_backward_raw(ctx.graph, ctx.edges, xr, cf, as_rows16(g), need_x=need_x, need_coeff=need_c)
        if dc is not None and dc.dtype != ctx.coeff_dtype:
            dc = dc.to(ctx.coeff_dtype)
        return dx, dc, None, None


def typed_spmm(graph, edges, x, coeff):
    """Z[i, b, :] = sum_e norm_e coeff[r_e, b] x[j_e, :] as [n_dst, B * F]; see the module text."""
    if not isinstance(graph, CSRGraph):
        raise TypeError("typed_spmm expects a CSRGraph (use dgll_amd.graph.as_csr_graph for torch sparse tensors)")
    if not isinstance(edges, TypedEdges):
        raise TypeError("typed_spmm expects the graph's TypedEdges")
    _require_cuda(x, coeff, graph.rowptr, edges.etypes)
    _dtype_code(x)
    if edges.graph is not graph and (edges.graph.nnz != graph.nnz or edges.graph.rowptr.data_ptr() != graph.rowptr.data_ptr()):
        raise ValueError("edges were built for another graph")
    if x.dim() != 2 or coeff.dim() != 2:
        raise ValueError("x [n_src, F] and coeff [num_rels, B] must be matrices")
    if x.shape[0] != graph.n_cols:
        raise ValueError("x has %d rows but the graph gathers from %d sources" % (x.shape[0], graph.n_cols))
    if coeff.shape[0] != edges.num_rels or coeff.shape[1] < 1:
        raise ValueError("coeff must be [num_rels = %d, B >= 1], got %s" % (edges.num_rels, tuple(coeff.shape)))
    F, B, vec = x.shape[1], coeff.shape[1], epv(x.dtype)
    if F == 0 or F % vec:
        raise ValueError("F = %d is not a whole number of 16-byte vectors (%d columns of %s); the layer pads its input" % (F, vec, x.dtype))
    if graph.n_rows == 0 or graph.nnz == 0:         # nothing to gather: zeros, with zero gradients
        return x.new_zeros((graph.n_rows, B * F)) + 0 * (x.sum() + coeff.sum().to(x.dtype))
    return _TypedSpmm.apply(x, coeff, graph, edges)
