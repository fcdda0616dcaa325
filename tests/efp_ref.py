"""The oracle of the fused-edge-projection tests: dgll_amd.ops_efp.u_op_proj_e_sum restated in float64, entry by entry, on top of
ef_ref.py.  With a [nnz, De] the raw edge attributes, W [F, De] and b [F] (torch.nn.Linear's layout):

    e[k]      = b + a[k] @ W.T                                   an explicit [nnz, F] float64 array here, never one in the kernel
    out       = ef_ref.forward(x, e)         grad_x, t = ef_ref.gradients(x, e, g)        (t[k] = s_i dm/de g[i] is ef_ref's grad_e)
    grad_a[k] = t[k] @ W        grad_W = t.T @ a        grad_b = sum_k t[k]

The gate.  ef_ref.py's argument that the fp32 gate IS the float64 gate does not carry over: e is now a rounded chain of up to 17
terms in the kernel, so x + e can differ in sign from the exact sum where that is nearly 0.  The tests therefore compare add_relu in
two ways and leave no element out of either: (1) DYADIC inputs (`inputs(..., dyadic=True)`: every value k / 8 with |k| <= 16, exact in
bf16), for which every product and every sum of every pass is exact in fp32 whatever the order, so fp32 results must EQUAL this
reference and bf16 results must equal it rounded once; (2) random inputs whose seed is chosen so that `near_gate` counts no element
with |x + aW + b| <= 2^-19 (|x| + |a||W| + |b|) -- a margin above the (De + 2) 2^-24 that a chain of De + 2 roundings can move the
sum by -- and which the tests assert before they compare.
"""
import torch

import ef_ref

OPS = ef_ref.OPS


def project(a, W, b):
    """e [nnz, F] float64"""
    e = a @ W.t()
    return e if b is None else e + b


def forward(rowptr, col, x, a, W, b, op, reduce="sum"):
    return ef_ref.forward(rowptr, col, x, project(a, W, b), op, reduce)


def gradients(rowptr, col, x, a, W, b, g, op, reduce="sum"):
    """(grad_x [n_src, F], grad_a [nnz, De], grad_W [F, De], grad_b [F]) float64 for the output gradient g [n_dst, F]"""
    gx, t = ef_ref.gradients(rowptr, col, x, project(a, W, b), g, op, reduce)
    return gx, t @ W, t.t() @ a, t.sum(0)


def near_gate(col, x, a, W, b):
    """how many elements of x[col_k] + e[k] are within 2^-19 of 0 relative to the sum of the magnitudes of their terms (float64)"""
    xs = x[col.long()]
    zero = torch.zeros(W.shape[0], dtype=torch.float64)
    s = xs + project(a, W, b)
    size = xs.abs() + a.abs() @ W.abs().t() + (zero if b is None else b.abs())
    return int((s.abs() <= 2.0 ** -19 * size).sum())


def inputs(graph, F, De, dtype, seed, dyadic, bias=True):
    """x [n_src, F], a [nnz, De], go [n_dst, F] of `dtype`; W [F, De], b [F] (or None) fp32.  dyadic: all of them k / 8, |k| <= 16."""
    gen = torch.Generator().manual_seed(seed)
    if dyadic:
        draw = lambda *shape: torch.randint(-16, 17, shape, generator=gen).to(torch.float32) / 8        # noqa: E731
    else:
        draw = lambda *shape: torch.randn(*shape, generator=gen)                                         # noqa: E731
    x, a, go = draw(graph.n_cols, F).to(dtype), draw(graph.nnz, De).to(dtype), draw(graph.n_rows, F).to(dtype)
    W = draw(F, De)
    b = draw(F) if bias else None
    return x, a, go, W, b


def gineconv(sd, rowptr, col, h_src, h_dst, a, apply_func=None):
    """nn.GINEConv(edge_dim=) from its state dict sd (float64): apply_func((1 + eps) h_dst + sum relu(h_src[col] + lin(a)))"""
    out = (1 + sd["eps"]) * h_dst + forward(rowptr, col, h_src, a, sd["lin.weight"], sd["lin.bias"], "add_relu")
    return out if apply_func is None else apply_func(out)
