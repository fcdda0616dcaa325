"""Sparse x sparse products on the device (csrc/spgemm.hip): C = A . B with all three matrices CSRGraphs.

    spgemm(a, b, *, values=True, check=True)   -> CSRGraph [a.n_rows, b.n_cols]        (also `a @ b`)
    khop_graph(g, k)                           -> the pattern of A^k
    coarsen(g, cluster, n_clusters=None)       -> S^T A S for a cluster id per node

PRECONDITION: the columns of every row of both operands are strictly increasing, which is what CSRGraph.from_coo(coalesce=True) and
CSRGraph.transpose() produce.  check=True verifies it with a torch expression, once per graph object (the answer is kept on the graph;
that first check reads one flag back), and raises ValueError naming the operand; check=False trusts the caller.

The result has strictly increasing columns in every row, an entry for every (i, j) that some k connects, whatever the values (a sum that
cancels to exactly 0.0 stays: the structure depends on the patterns only), and fp32 values; an operand without values counts as all
ones, so two patterns give path counts.  values=False computes the pattern alone (C.val is None).  No floating-point atomics: two
calls give the same bits.

The structure of C is unknown before the kernels run.  The symbolic launch counts every row and leaves nnz(C) on the device; spgemm
reads these 8 BYTES BACK to allocate col and val.  That is the ONLY host synchronisation of the forward (so the call cannot be captured
into a graph); the numeric launch and both backward launches synchronise nothing.

When a.val or b.val requires grad, C.val comes from a torch.autograd.Function whose backward runs one gather launch per operand that
needs a gradient (dgll_hip_spgemm_bwd; the one for b goes through a.transpose(), which is cached).  An operand without values gets none.
There is no CPU implementation: a CPU graph raises.
"""
import torch

from . import _lib
from .graph import CSRGraph
from .ops import _require_cuda

WAVE_MAX, LDS_MAX = _lib.SPGEMM_WAVE_MAX, _lib.SPGEMM_LDS_MAX
LONG_POOL_BYTES = 64 << 20      # the slots of the long rows (about 4.25 N bytes each) take this much scratch at the most, but one always
LONG_SLOTS_MAX = 256


def _long_slots(M, N):
    per = _lib.lib.dgll_hip_spgemm_scratch_bytes(0, N, 1) - _lib.lib.dgll_hip_spgemm_scratch_bytes(0, N, 0)
    return max(1, min(M, LONG_SLOTS_MAX, LONG_POOL_BYTES // per))


def _columns_increase(g):
    """True when the columns of every row of g are strictly increasing; computed once per graph object"""
    if getattr(g, "_cols_increase", None) is None:
        ok = True
        if g.nnz > 1:
            starts = torch.zeros(g.nnz + 1, dtype=torch.bool, device=g.device)
            starts[g.rowptr] = True                                        # entry e opens a row
            ok = not bool(((g.col[1:] <= g.col[:-1]) & ~starts[1:g.nnz]).any())
        g._cols_increase = ok
    return g._cols_increase


def _product(a, b, a_val, b_val, values, long_slots=None):
    """(rowptr, col, val or None) of A . B: the symbolic launch, the read-back of nnz(C), the numeric launch"""
    M, K, N, dev = a.n_rows, a.n_cols, b.n_cols, a.device
    if M == 0 or K == 0 or N == 0 or a.nnz == 0 or b.nnz == 0:          # an empty product: nothing to launch
        return (torch.zeros(M + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, dtype=torch.float32, device=dev) if values else None)
    rowptr = torch.empty(M + 1, dtype=torch.int64, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    n_bytes = _lib.lib.dgll_hip_spgemm_scratch_bytes(M, N, _long_slots(M, N) if long_slots is None else max(1, int(long_slots)))
    scratch = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    _lib.launch("dgll_hip_spgemm_symbolic", dev, M, K, N, a.rowptr.data_ptr(), a.col.data_ptr(), a.nnz, b.rowptr.data_ptr(),
                b.col.data_ptr(), b.nnz, rowptr.data_ptr(), total.data_ptr(), scratch.data_ptr(), n_bytes,
                tag=lambda: ("spgemm_symbolic", M, a.nnz, b.nnz))
    nnz_c = int(total.item())                                              # the one read-back
    col = torch.empty(max(nnz_c, 0), dtype=torch.int32, device=dev)
    val = torch.empty(max(nnz_c, 0), dtype=torch.float32, device=dev) if values else None
    _lib.launch("dgll_hip_spgemm_numeric", dev, M, K, N, a.rowptr.data_ptr(), a.col.data_ptr(), _lib.ptr(a_val), a.nnz,
                b.rowptr.data_ptr(), b.col.data_ptr(), _lib.ptr(b_val), b.nnz, rowptr.data_ptr(), col.data_ptr() if nnz_c > 0 else None,
                _lib.ptr(val) if nnz_c > 0 else None, nnz_c, scratch.data_ptr(), n_bytes,     # a negative total raises here, with the reason
                tag=lambda: ("spgemm_numeric", M, a.nnz, nnz_c))
    return rowptr, col, val


def _grad(mode, x, y, y_val, n_rows_c, rowptr, col, grad_c):
    """fp32 [x.nnz]: the gradient of x's values (mode A: x = A, y = B; mode B: x = B, y = A^T)"""
    grad = torch.empty(x.nnz, dtype=torch.float32, device=x.device)
    if x.nnz:
        _lib.launch("dgll_hip_spgemm_bwd", x.device, mode, x.n_rows, x.rowptr.data_ptr(), x.col.data_ptr(), x.nnz, y.n_rows,
                    y.rowptr.data_ptr(), y.col.data_ptr() if y.nnz else None, _lib.ptr(y_val), y.nnz, n_rows_c, rowptr.data_ptr(),
                    col.data_ptr() if col.numel() else None, grad_c.data_ptr() if col.numel() else None, col.numel(), grad.data_ptr(),
                    tag=lambda: ("spgemm_bwd", mode, x.nnz))
    return grad


class _Values(torch.autograd.Function):
    """C.val as a function of a.val and b.val; the structure of C leaves through `out`"""

    @staticmethod
    def forward(ctx, a_val, b_val, a, b, out, long_slots):
        av = None if a_val is None else a_val.detach().contiguous()
        bv = None if b_val is None else b_val.detach().contiguous()
        rowptr, col, val = _product(a, b, av, bv, True, long_slots)
        out.extend([rowptr, col])
        ctx.a, ctx.b = a, b
        ctx.save_for_backward(av, bv, rowptr, col)
        return val

    @staticmethod
    def backward(ctx, g):
        av, bv, rowptr, col = ctx.saved_tensors
        a, b = ctx.a, ctx.b
        g = g.to(torch.float32).contiguous()
        ga = gb = None
        if av is not None and ctx.needs_input_grad[0]:
            ga = _grad(_lib.SPGEMM_BWD_A, a, b, bv, a.n_rows, rowptr, col, g)
        if bv is not None and ctx.needs_input_grad[1]:
            at, perm = a.transpose()
            gb = _grad(_lib.SPGEMM_BWD_B, b, at, None if av is None else av[perm], a.n_rows, rowptr, col, g)
        return ga, gb, None, None, None, None


def spgemm(a, b, *, values=True, check=True, long_slots=None):
    """C = A . B as a CSRGraph (module docstring).  long_slots: how many rows of the long class (more than LDS_MAX products) run at
    once, each on about 4.25 * b.n_cols bytes of scratch; None sizes the pool by LONG_POOL_BYTES."""
    if not isinstance(a, CSRGraph) or not isinstance(b, CSRGraph):
        raise TypeError("spgemm: both operands must be CSRGraphs")
    if a.n_cols != b.n_rows:
        raise ValueError("spgemm: a is [%d, %d] and b is [%d, %d]: the inner dimensions differ" % (a.shape + b.shape))
    if a.device != b.device:
        raise ValueError("spgemm: a is on %s and b on %s" % (a.device, b.device))
    if check:
        for name, g in (("a", a), ("b", b)):
            if not _columns_increase(g):
                raise ValueError("spgemm: the columns of every row of operand %s must be strictly increasing "
                                 "(build it with CSRGraph.from_coo(coalesce=True))" % name)
    _require_cuda(a.rowptr, b.rowptr)
    needs_grad = values and torch.is_grad_enabled() and any(v is not None and v.requires_grad for v in (a.val, b.val))
    if needs_grad:
        out = []
        val = _Values.apply(a.val, b.val, a, b, out, long_slots)
        rowptr, col = out
    else:
        rowptr, col, val = _product(a, b, None if a.val is None else a.val.detach(), None if b.val is None else b.val.detach(), values,
                                    long_slots)
    c = CSRGraph(rowptr, col, val, a.n_rows, b.n_cols, check=False)
    c._cols_increase = True
    return c


def khop_graph(g, k):
    """The pattern of A^k (no values): node i reaches node j in exactly k steps.  k - 1 products spgemm(values=False)."""
    if int(k) != k or int(k) < 1:
        raise ValueError("khop_graph: k must be an integer >= 1, got %r" % (k,))
    if g.n_rows != g.n_cols:
        raise ValueError("khop_graph needs a square adjacency, got [%d, %d]" % g.shape)
    hop = CSRGraph(g.rowptr, g.col, None, g.n_rows, g.n_cols, check=False)
    out = hop
    for _ in range(int(k) - 1):
        out = spgemm(out, hop, values=False)
    return out


def coarsen(g, cluster, n_clusters=None):
    """S^T A S [C, C] for `cluster`, an int64 vector with the cluster id in [0, C) of every node: entry (p, q) sums the weights (counts
    the entries, without values) between clusters p and q.  n_clusters None reads max(cluster) + 1 back."""
    if g.n_rows != g.n_cols:
        raise ValueError("coarsen needs a square adjacency, got [%d, %d]" % g.shape)
    if not isinstance(cluster, torch.Tensor) or cluster.dtype != torch.int64 or cluster.shape != (g.n_rows,):
        raise ValueError("coarsen: cluster must be an int64 vector with one cluster id per node (%d)" % g.n_rows)
    _require_cuda(g.rowptr, cluster)
    n = g.n_rows
    C = int(n_clusters) if n_clusters is not None else (int(cluster.max()) + 1 if n else 0)
    s = CSRGraph(torch.arange(n + 1, dtype=torch.int64, device=g.device), cluster.to(torch.int32), None, n, C, check=False)
    return spgemm(spgemm(s.transpose()[0], g), s)
