"""The oracle of the gated-aggregation tests: dgll_amd.ops_gated.gated_sum restated in float64 entry by entry, without autograd.
Entry k of row i is the edge j = col[k] -> i.  For every column independently:

    ehat[k] = c[k] + a[i] + b[j]        sig[k] = sigmoid(ehat[k])        S_i = sum_k sig[k] + eps
    out[i]  = (sum_k sig[k] v[j]) / S_i                                   (a row without entries: 0)

    t[k]      = ge[k] + g[i] (v[j] - out[i]) / S_i sig[k] (1 - sig[k])      g = d out, ge = d ehat (None: zeros)
    grad_c[k] = t[k]        grad_a[i] = sum over row i of t[k]        grad_b[j] = sum over column j of t[k]
    grad_v[j] = sum over column j of sig[k] g[i] / S_i

The gate is smooth, so the one-ulp freedom a kernel has in rounding ehat to its storage type moves nothing by more than that ulp:
no element is excluded from any comparison.  `composition` is the same function written with torch's index ops, for autograd to
differentiate (test_gated_host.py holds the two against each other).
"""
import torch


def _rows(rowptr):
    rp = [int(v) for v in rowptr]
    return [(i, rp[i], rp[i + 1]) for i in range(len(rp) - 1)]


def forward(rowptr, col, a, b, c, v, eps=1e-6):
    """(out [n_dst, F], ehat [nnz, F]) float64"""
    out, ehat = torch.zeros_like(a), torch.zeros_like(c)
    for i, lo, hi in _rows(rowptr):
        num, den = torch.zeros_like(a[i]), torch.zeros_like(a[i])
        for k in range(lo, hi):
            j = int(col[k])
            ehat[k] = c[k] + a[i] + b[j]
            sig = 1.0 / (1.0 + torch.exp(-ehat[k]))
            num += sig * v[j]
            den += sig
        out[i] = num / (den + eps)
    return out, ehat


def gradients(rowptr, col, a, b, c, v, eps, g, ge=None):
    """(grad_a, grad_b, grad_c, grad_v) float64 for the output gradients g [n_dst, F] and ge [nnz, F] (None: zeros)"""
    out, ehat = forward(rowptr, col, a, b, c, v, eps)
    ga, gb, gc, gv = torch.zeros_like(a), torch.zeros_like(b), torch.zeros_like(c), torch.zeros_like(v)
    for i, lo, hi in _rows(rowptr):
        sigs = [1.0 / (1.0 + torch.exp(-ehat[k])) for k in range(lo, hi)]
        s_i = sum(sigs, torch.zeros_like(a[i])) + eps
        for k, sig in zip(range(lo, hi), sigs):
            j = int(col[k])
            t = g[i] * (v[j] - out[i]) / s_i * sig * (1.0 - sig)
            if ge is not None:
                t = t + ge[k]
            gc[k] = t
            ga[i] += t
            gb[j] += t
            gv[j] += sig * g[i] / s_i
    return ga, gb, gc, gv


def composition(rowptr, col, a, b, c, v, eps=1e-6):
    """(out, ehat) with index_add_, differentiable"""
    n = len(rowptr) - 1
    row = torch.repeat_interleave(torch.arange(n), (rowptr[1:] - rowptr[:-1]).long())
    j = col.long()
    ehat = c + a[row] + b[j]
    sig = torch.sigmoid(ehat)
    num = torch.zeros_like(a).index_add_(0, row, sig * v[j])
    den = torch.zeros_like(a).index_add_(0, row, sig)
    return num / (den + eps), ehat
