"""Gaussian-mixture edge weights (MoNet, DGL's GMMConv underneath): csrc/gmm.hip.

    gmm_expand(graph, x, pseudo, mu, inv_sigma, reduce="sum") -> Z [n_dst, K * F] of x's dtype

Every entry e = (j -> i) of `graph` (a CSRGraph, n_dst rows gathering from n_src columns; rectangular blocks allowed; duplicate
entries are separate edges) carries `dim` pseudo-coordinates pseudo[e, :], in the graph's CSR entry order.  With mu and inv_sigma
[K, dim]:

    w_k(e)     = exp(-0.5 * sum_d ((pseudo[e, d] - mu[k, d]) * inv_sigma[k, d])^2)
    Z[i, k, :] = s_i * sum_e w_k(e) x[j_e, :]        s_i = 1 ("sum") or 1 / deg_i ("mean");  Z laid out in kernel-major blocks of width F

so that MoNet's s_i sum_e sum_k w_k(e) x_j W_k is the dense product Z . stack_k(W_k), and no [nnz, K, out] message tensor exists.  x
is fp32 or bf16 on the GPU (fp32 accumulation); F must be a whole number of 16-byte vectors (4 fp32 / 8 bf16 columns -- the layer
pads).  pseudo may be any floating dtype and may require a gradient; it is held as contiguous fp32 inside and its gradient comes back
in its own dtype.  1 <= dim <= MAX_DIM, 1 <= K <= MAX_KERNELS.

One autograd node that saves x, the fp32 pseudo, mu and inv_sigma and nothing else.  Passes, each run only when a wanted gradient
needs it: EXPAND (the forward: x_j gathered once per entry, up to 8 kernels' accumulators per launch block, more kernels re-gather x once per block); CONTRACT over the rows
of A^T for grad x (graph.transpose(), the cached structure; pseudo read through its perm); and, when mu, inv_sigma or pseudo needs a
gradient, ops_typed's EDGE_DOTS pass with one type -- P[e, k] = <x_j, dZ[i, k, :]>, fp32 with K rounded up to 4 columns, the one
per-edge scratch of the backward -- followed by PARAM, which streams P and pseudo, writes grad_pseudo (only when wanted) and one fp32
slab [2, K, dim] per workgroup; the slabs are summed in slab order (torch.sum(0)).  With reduce="mean" the incoming gradient's rows
are multiplied by 1 / deg once before the passes.  The weight is one device function in all three passes (fp32, one exp2): the same
bits everywhere.  No float atomics: reruns give the same bits; nothing is allocated, synchronised or read back by a pass, so a step
can be captured.  There is no CPU implementation here: a CPU tensor raises (nn.GMMConv has a host path of its own).

Not built: a max over the messages, the project-first order (x W_k before the gather; it gathers less only when in > K * out), P
fused away, K > 64, dim > 8, the partitioned (multi-GPU) path.
"""
import ctypes as C

import torch

from . import _lib, ops_typed
from .graph import CSRGraph
from .ops import _dtype_code, epv, _require_cuda, alloc_features, as_rows16
from .ops_ef import mean_scale

MAX_DIM = _lib.GMM_MAX_DIM
MAX_KERNELS = _lib.GMM_MAX_KERNELS
MAX_PARTIALS = _lib.GMM_MAX_PARTIALS
_TAGS = ("gmm_expand", "gmm_contract", "gmm_param")
_PARAM_BLOCK = 256                      # entries a workgroup of PARAM takes per grid stride


def _launch(kind, device, dtype_code, nnz, F, pseudo, mu, inv_sigma, gr=None, perm=None, scale=None, x=None, dz=None, out=None, p=None,
            gp=None, slabs=None, partials=0):
    d = _lib.GmmDesc()
    d.pass_, d.dtype, d.K, d.dim = kind, dtype_code, mu.shape[0], mu.shape[1]
    if gr is not None:
        d.rowptr, d.col, d.n_rows, d.n_cols = gr.rowptr.data_ptr(), gr.col.data_ptr(), gr.n_rows, gr.n_cols
    d.perm, d.nnz, d.F, d.scale = _lib.ptr(perm), nnz, F, _lib.ptr(scale)
    d.pseudo, d.ld_pseudo, d.mu, d.inv_sigma = pseudo.data_ptr(), pseudo.stride(0), mu.data_ptr(), inv_sigma.data_ptr()
    d.x, d.ld_x, d.dz, d.ld_dz, d.out, d.ld_out = _lib.ptr(x), _lib.pitch(x), _lib.ptr(dz), _lib.pitch(dz), _lib.ptr(out), _lib.pitch(out)
    d.p, d.ld_p, d.grad_pseudo, d.ld_grad_pseudo = _lib.ptr(p), _lib.pitch(p), _lib.ptr(gp), _lib.pitch(gp)
    d.slabs, d.partials = _lib.ptr(slabs), partials
    _lib.launch("dgll_hip_gmm_pass", device, C.byref(d), tag=lambda: (_TAGS[kind], F, d.K, d.dim, nnz))


def kernel_params(pseudo, mu, inv_sigma):
    """(pseudo, mu, inv_sigma) as the passes read them: detached, fp32, contiguous."""
    return tuple(t.detach().to(torch.float32).contiguous() for t in (pseudo, mu, inv_sigma))


# ---- raw passes (no autograd, no checks): what the autograd node, tools/gmm_bench.py and the tests call ----------------------------------
# x, g: matrices with rows on a 16-byte pitch; pseudo, mu, inv_sigma: kernel_params(); scale: fp32 [n_dst] or None.
def expand_raw(graph, x, pseudo, mu, inv_sigma, scale=None):
    """Z [n_dst, K * F]."""
    K, F = mu.shape[0], x.shape[1]
    z = alloc_features(graph.n_rows, K * F, x.dtype, x.device, pad_to=epv(x.dtype))
    _launch(_lib.GMM_EXPAND, x.device, _dtype_code(x), graph.nnz, F, pseudo, mu, inv_sigma, gr=graph, scale=scale, x=x, out=z)
    return z


def contract_raw(graph, pseudo, mu, inv_sigma, g):
    """grad_x [n_src, F] over graph.transpose() from g [n_dst, K * F] (already scaled for the mean)."""
    K = mu.shape[0]
    F = g.shape[1] // K
    gt, perm = graph.transpose()
    dx = alloc_features(gt.n_rows, F, g.dtype, g.device, pad_to=epv(g.dtype))
    _launch(_lib.GMM_CONTRACT, g.device, _dtype_code(g), graph.nnz, F, pseudo, mu, inv_sigma, gr=gt, perm=perm, dz=g, out=dx)
    return dx


def edge_dots_raw(graph, x, g, K):
    """P fp32 [nnz, K rounded up to 4]: P[e, k] = <x[j_e], g[i_e, k, :]> -- ops_typed's EDGE_DOTS pass with one edge type (it reads
    neither the types nor the table)."""
    p = torch.empty((graph.nnz, (K + 3) // 4 * 4), dtype=torch.float32, device=x.device)
    ops_typed._launch(_lib.TYPED_EDGE_DOTS, graph, None, None, 1, K, x.shape[1], None, x=x, dz=g, p=p)
    return p


def param_raw(p, pseudo, mu, inv_sigma, want_pseudo=False, partials=None, slabs=None):
    """(grad_mu fp32 [K, dim], grad_inv_sigma fp32 [K, dim], grad_pseudo fp32 [nnz, dim] or None) from P (edge_dots_raw).  partials: the
    workgroups (and slabs) of the pass, min(ceil(nnz / 256), MAX_PARTIALS) when None.  slabs: a caller's fp32 [partials, 2, K, dim]
    buffer to write (every element is written)."""
    K, dim = mu.shape
    nnz = p.shape[0]
    if partials is None:
        partials = max(1, min(-(-nnz // _PARAM_BLOCK), MAX_PARTIALS))
    if slabs is None:
        slabs = torch.empty((partials, 2, K, dim), dtype=torch.float32, device=p.device)
    gp = torch.empty((nnz, dim), dtype=torch.float32, device=p.device) if want_pseudo else None
    _launch(_lib.GMM_PARAM, p.device, _lib.F32, nnz, 0, pseudo, mu, inv_sigma, p=p, gp=gp, slabs=slabs, partials=partials)
    total = slabs.sum(0)
    return total[0], total[1], gp


class _GmmExpand(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pseudo, mu, inv_sigma, graph, scale):
        xr = as_rows16(x.detach())
        ps, m, s = kernel_params(pseudo, mu, inv_sigma)
        ctx.graph, ctx.scale = graph, scale
        ctx.dtypes = (pseudo.dtype, mu.dtype, inv_sigma.dtype)
        ctx.save_for_backward(xr, ps, m, s)
        return expand_raw(graph, xr, ps, m, s, scale)

    @staticmethod
    def backward(ctx, g):
        need_x, need_p, need_m, need_s = ctx.needs_input_grad[:4]
        if not (need_x or need_p or need_m or need_s):
            return (None,) * 6
        xr, ps, m, s = ctx.saved_tensors
        if g.dtype != xr.dtype:
            g = g.to(xr.dtype)
        if ctx.scale is not None:                   # the mean: the rows of the gradient scaled once, node-sized
            g = g * ctx.scale.to(g.dtype).unsqueeze(1)
        gr = as_rows16(g)
        gx = contract_raw(ctx.graph, ps, m, s, gr) if need_x else None
        gp = gm = gs = None
        if need_p or need_m or need_s:
            p = edge_dots_raw(ctx.graph, xr, gr, m.shape[0])
            gm, gs, gp = param_raw(p, ps, m, s, want_pseudo=need_p)
        p_dtype, m_dtype, s_dtype = ctx.dtypes
        return (gx, gp.to(p_dtype) if need_p else None, gm.to(m_dtype) if need_m else None, gs.to(s_dtype) if need_s else None,
                None, None)


def gmm_expand(graph, x, pseudo, mu, inv_sigma, reduce="sum"):
    """Z[i, k, :] = s_i sum_e w_k(e) x[j_e, :] as [n_dst, K * F]; see the module text."""
    if not isinstance(graph, CSRGraph):
        raise TypeError("gmm_expand expects a CSRGraph (use dgll_amd.graph.as_csr_graph for torch sparse tensors)")
    if reduce not in ("sum", "mean"):
        raise ValueError("gmm_expand: reduce must be 'sum' or 'mean', got %r (a max over the messages is not built)" % (reduce,))
    _dtype_code(x)
    if x.dim() != 2 or x.shape[0] != graph.n_cols:
        raise ValueError("gmm_expand: x must be a matrix of %d rows (the sources the graph gathers from), got %s" % (graph.n_cols, tuple(x.shape)))
    F, vec = x.shape[1], epv(x.dtype)
    if F == 0 or F % vec:
        raise ValueError("gmm_expand: the width %d is not a whole number of 16-byte vectors (%d columns of %s); the layers pad "
                         "their widths with zero columns" % (F, vec, x.dtype))
    if not torch.is_tensor(pseudo) or not pseudo.is_floating_point() or pseudo.dim() != 2 or pseudo.shape[0] != graph.nnz:
        raise ValueError("gmm_expand: pseudo must be a floating-point [nnz, dim] matrix with nnz = %d, got %s"
                         % (graph.nnz, tuple(pseudo.shape) if torch.is_tensor(pseudo) else type(pseudo).__name__))
    dim = pseudo.shape[1]
    for name, t in (("mu", mu), ("inv_sigma", inv_sigma)):
        if not torch.is_tensor(t) or not t.is_floating_point() or t.dim() != 2 or t.shape[1] != dim:
            raise ValueError("gmm_expand: %s must be a floating-point [K, dim] matrix with dim = %d (the columns of pseudo), got %s"
                             % (name, dim, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    if mu.shape != inv_sigma.shape:
        raise ValueError("gmm_expand: mu and inv_sigma must have one shape [K, dim], got %s and %s" % (tuple(mu.shape), tuple(inv_sigma.shape)))
    K = mu.shape[0]
    if not 1 <= dim <= MAX_DIM:
        raise ValueError("gmm_expand: pseudo has %d columns: dim must be in 1..%d" % (dim, MAX_DIM))
    if not 1 <= K <= MAX_KERNELS:
        raise ValueError("gmm_expand: mu has %d rows: the number of kernels K must be in 1..%d" % (K, MAX_KERNELS))
    _require_cuda(x, pseudo, mu, inv_sigma, graph.rowptr)
    if graph.n_rows == 0 or graph.nnz == 0:         # nothing to gather: zeros, with zero gradients
        zero = x.sum() + (pseudo.sum() + mu.sum() + inv_sigma.sum()).to(x.dtype)
        return x.new_zeros((graph.n_rows, K * F)) + 0 * zero
    return _GmmExpand.apply(x, pseudo, mu, inv_sigma, graph, mean_scale(graph) if reduce == "mean" else None)
