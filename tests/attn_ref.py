"""The oracle of the sparse-attention tests: scaled dot-product attention over the entries of a CSR matrix, restated with per-edge
tensors (index_add, scatter_reduce(amax)) so that autograd gives the gradients.  It uses nothing of dgll_amd.ops_attn and nothing of
the layers' host path; the tests pass float64."""
import torch


def sparse_attention_reference(rowptr, col, q, k, v, scale):
    """out [n_dst, H, D] and the logits s [nnz, H] for q [n_dst, H, D], k and v [n_src, H, D] (any float dtype):
    s_ij = scale <q_i, k_j>,  alpha = softmax over the row's entries (max-subtracted),  out_i = sum_j alpha_ij v_j.
    Duplicate entries are separate edges; an empty row stays 0."""
    n, heads = rowptr.numel() - 1, q.shape[1]
    row = torch.repeat_interleave(torch.arange(n, device=rowptr.device), rowptr[1:] - rowptr[:-1])
    col = col.long()
    s = (q[row] * k[col]).sum(-1) * scale
    top = torch.full((n, heads), -float("inf"), dtype=s.dtype, device=s.device)
    top = top.scatter_reduce(0, row.unsqueeze(1).expand_as(s), s.detach(), "amax")
    w = torch.exp(s - top[row])
    den = torch.zeros((n, heads), dtype=s.dtype, device=s.device).index_add_(0, row, w)
    alpha = w / den[row]
    out = torch.zeros((n,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device).index_add_(0, row, alpha.unsqueeze(-1) * v[col])
    return out, s
