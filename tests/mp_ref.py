"""The oracle of the message-passing tests: the five operators of dgll_amd/ops_mp.py restated with per-edge tensors (repeat_interleave,
index_add_, scatter_reduce(amax)) so that autograd gives the gradients.  It uses nothing of dgll_amd.ops_mp and nothing of the layers'
host path; the tests pass float64.  Every function takes the CSR arrays (rowptr, col) of the graph; per-edge tensors are in its
entry order."""
import torch


def rows_of(rowptr):
    """row [nnz]: the row of every entry."""
    n = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, device=rowptr.device), rowptr[1:] - rowptr[:-1])


def _segment_softmax(seg, n, e):
    """softmax of e [nnz, H] over the entries with the same seg (in [0, n)): max-subtracted; an entry of -inf maps to 0 and a segment
    of -inf alone gives zeros."""
    top = torch.full((n, e.shape[1]), -float("inf"), dtype=e.dtype, device=e.device)
    top = top.scatter_reduce(0, seg.unsqueeze(1).expand_as(e), e.detach(), "amax")
    top = torch.where(torch.isinf(top), torch.zeros_like(top), top)        # a segment of -inf alone: exp(-inf - 0) = 0
    w = torch.exp(e - top[seg])
    den = torch.zeros((n, e.shape[1]), dtype=e.dtype, device=e.device).index_add_(0, seg, w)
    den = torch.where(den > 0, den, torch.ones_like(den))
    return w / den[seg]


def edge_softmax_reference(rowptr, col, n_cols, e, norm_by="dst"):
    """[nnz, H]: softmax over the entries of each row (dst) or of each column (src)."""
    if norm_by == "dst":
        return _segment_softmax(rows_of(rowptr), rowptr.numel() - 1, e)
    return _segment_softmax(col.long(), n_cols, e)


def u_mul_e_sum_reference(rowptr, col, x, w):
    """[n_dst, H, D] from x [n_src, H, D] and w [nnz, H]: out_i = sum_k w_k x[col_k]."""
    row, n = rows_of(rowptr), rowptr.numel() - 1
    return torch.zeros((n,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device).index_add_(0, row, w.unsqueeze(-1) * x[col.long()])


def u_dot_v_reference(rowptr, col, x, y):
    """[nnz, H] from x [n_src, H, D] and y [n_dst, H, D]: <x[col_k], y[row_k]> per head."""
    return (x[col.long()] * y[rows_of(rowptr)]).sum(-1)


def u_add_v_reference(rowptr, col, a, b):
    """[nnz, H] from a [n_src, H] and b [n_dst, H]."""
    return a[col.long()] + b[rows_of(rowptr)]


def copy_e_sum_reference(rowptr, col, n_cols, w, norm_by="dst"):
    """[n_dst, H] (dst) or [n_src, H] (src): the sum of the entries of each row, or of each column."""
    if norm_by == "dst":
        seg, n = rows_of(rowptr), rowptr.numel() - 1
    else:
        seg, n = col.long(), n_cols
    return torch.zeros((n, w.shape[1]), dtype=w.dtype, device=w.device).index_add_(0, seg, w)
