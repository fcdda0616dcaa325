"""The oracle of the edge-feature tests: dgll_amd.ops_ef.u_op_e_sum, nn.GINEConv and nn.CFConv restated in float64 with EXPLICIT
per-edge messages, row by row.  Entry k of row i is the edge j = col[k] -> i with the feature row e[k]:

    out[i]    = s_i * sum_k m(x[col_k], e[k])            s_i = 1 (sum) or 1 / D_i (mean), an empty row gives 0
    grad_x[j] = sum over the entries k with col_k = j of s_i * dm/dx * g[i]
    grad_e[k] = s_i * dm/de * g[i]

    op          m              dm/dx    dm/de
    add         x + e          1        1
    add_relu    relu(x + e)    gate     gate        gate = (x + e > 0)
    mul         x * e          e        x

The gate of the reference is the sign of the FLOAT64 sum of the two operands as stored (bf16-rounded where the kernel reads bf16),
and no element is excluded from any comparison on its account: a correctly rounded fp32 sum has the sign of the exact sum (rounding
is monotone and 0 is representable, so a positive sum never rounds below 0 nor a negative one above it, and the sum of two floats
is exactly 0 only when the exact sum is), and with inputs of order 1 nothing underflows.  So the kernel's fp32 gate IS this one.
"""
import torch

OPS = ("add", "add_relu", "mul")


def _rows(rowptr):
    rp = [int(v) for v in rowptr]
    return [(i, rp[i], rp[i + 1]) for i in range(len(rp) - 1)]


def messages(col, x, e, op):
    """[nnz, F] float64 (differentiable where x or e require it)"""
    xs = x[col.long()]
    if op == "mul":
        return xs * e
    s = xs + e
    return torch.where(s > 0, s, torch.zeros_like(s)) if op == "add_relu" else s


def forward(rowptr, col, x, e, op, reduce="sum"):
    """out [n_dst, F] float64 from float64 x [n_src, F], e [nnz, F]"""
    m = messages(col, x, e, op)
    rows = []
    for _, b, t in _rows(rowptr):
        if t == b:
            rows.append(torch.zeros(x.shape[1], dtype=torch.float64))
        else:
            r = m[b:t].sum(0)
            rows.append(r / (t - b) if reduce == "mean" else r)
    return torch.stack(rows) if rows else torch.zeros(0, x.shape[1], dtype=torch.float64)


def gradients(rowptr, col, x, e, g, op, reduce="sum"):
    """(grad_x [n_src, F], grad_e [nnz, F]) float64 for the output gradient g [n_dst, F], written out entry by entry"""
    gx, ge = torch.zeros_like(x), torch.zeros_like(e)
    for i, b, t in _rows(rowptr):
        s = 1.0 / (t - b) if reduce == "mean" and t > b else 1.0
        for k in range(b, t):
            j = int(col[k])
            if op == "mul":
                dx, de = e[k], x[j]
            elif op == "add_relu":
                dx = de = (x[j] + e[k] > 0).to(torch.float64)
            else:
                dx = de = torch.ones_like(e[k])
            gx[j] += s * dx * g[i]
            ge[k] = s * de * g[i]
    return gx, ge


def shifted_softplus(v):
    return torch.nn.functional.softplus(v) - torch.log(torch.tensor(2.0, dtype=v.dtype))


def gineconv(sd, rowptr, col, h_src, h_dst, e, apply_func=None):
    """nn.GINEConv from its state dict sd (float64): apply_func((1 + eps) h_dst + sum relu(h_src[col] + e))"""
    out = (1 + sd["eps"]) * h_dst + forward(rowptr, col, h_src, e, "add_relu")
    return out if apply_func is None else apply_func(out)


def cfconv(sd, rowptr, col, h_src, a):
    """nn.CFConv from its state dict sd (float64 tensors; those that require grad receive gradients)"""
    lin = lambda v, name: v @ sd[name + ".weight"].t() + sd[name + ".bias"]      # noqa: E731
    w = shifted_softplus(lin(shifted_softplus(lin(a, "project_edge.0")), "project_edge.2"))
    agg = forward(rowptr, col, lin(h_src, "project_node"), w, "mul")
    return shifted_softplus(lin(agg, "project_out.0"))
