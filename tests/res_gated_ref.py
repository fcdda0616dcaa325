"""The oracle of the ResGated tests: dgll_amd.ops_res_gated.res_gated_sum restated in float64 edge by edge with torch's index ops,
without autograd.  Entry e of row i is the edge j = col[e] -> i.  For every column independently:

    s[e] = sigmoid(k[i] + q[j])        out[i] = sum_e s[e] v[j]        (mean: divided by the row's entry count; no entries: 0)

    grad_k[i] = g[i] sum_e s[e] (1 - s[e]) v[j]        grad_q[j] = v[j] sum over column j of g[i] s[e] (1 - s[e])
    grad_v[j] = sum over column j of g[i] s[e]         (mean: g[i] / the entry count of row i in place of g[i])

Every quantity per edge is a real [nnz, F] float64 array here (that is the point of a restatement: the kernels never form one).  The
gate is smooth and every formula a sum of products: no element is excluded from any comparison.
"""
import torch


def _edges(rowptr, col):
    deg = (rowptr[1:] - rowptr[:-1]).long()
    return torch.repeat_interleave(torch.arange(len(deg)), deg), col.long(), deg


def _scale(deg, mean):
    return 1.0 / deg.clamp(min=1).double().unsqueeze(1) if mean else torch.ones(len(deg), 1, dtype=torch.float64)


def forward(rowptr, col, k, q, v, mean=False):
    """out [n_dst, F] float64"""
    row, j, deg = _edges(rowptr, col)
    s = 1.0 / (1.0 + torch.exp(-(k[row] + q[j])))
    return torch.zeros_like(k).index_add_(0, row, s * v[j]) * _scale(deg, mean)


def gradients(rowptr, col, k, q, v, g, mean=False):
    """(grad_k, grad_q, grad_v) float64 for the output gradient g [n_dst, F]"""
    row, j, deg = _edges(rowptr, col)
    g = g * _scale(deg, mean)
    s = 1.0 / (1.0 + torch.exp(-(k[row] + q[j])))
    ds = s * (1.0 - s)
    gk = g * torch.zeros_like(k).index_add_(0, row, ds * v[j])
    gq = v * torch.zeros_like(q).index_add_(0, j, g[row] * ds)
    gv = torch.zeros_like(v).index_add_(0, j, g[row] * s)
    return gk, gq, gv
