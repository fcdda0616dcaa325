"""float64 restatement, entry by entry, of what csrc/gmm.hip, dgll_amd/ops_gmm.py and nn.GMMConv compute (MoNet / DGL's GMMConv):

    w_k(e)     = exp(-0.5 * sum_d ((pseudo[e, d] - mu[k, d]) * inv_sigma[k, d])^2)
    Z[i, k, :] = s_i sum_{e = (j -> i)} w_k(e) x_j                     s_i = 1 ("sum") or 1 / deg_i ("mean", 0 for an empty row)

and, for an output gradient G [n_dst, K * F] (Gs = s_i G, P[e, k] = <x_j, Gs[i, k, :]>, t = pseudo - mu, s = inv_sigma):

    grad_x[j]           = sum_e sum_k w_k(e) Gs[i_e, k, :]
    grad_mu[k, d]       = sum_e  P w t s^2          grad_inv_sigma[k, d] = -sum_e P w t^2 s          grad_pseudo[e, d] = -sum_k P w t s^2

written with explicit per-entry terms (no autograd), so that the sums over all entries can be examined term by term.  DGL is not
installed here: this file, not a recorded DGL output, is what the kernels and the layer are compared with."""
import torch


def row_index(rowptr):
    n = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])


def row_scale(rowptr, reduce):
    deg = (rowptr[1:] - rowptr[:-1]).double()
    if reduce == "sum":
        return torch.ones_like(deg)
    return torch.where(deg > 0, 1.0 / deg.clamp(min=1.0), torch.zeros_like(deg))


def weights(pseudo, mu, inv_sigma):
    """[nnz, K] float64"""
    t = (pseudo.double().unsqueeze(1) - mu.double().unsqueeze(0)) * inv_sigma.double().unsqueeze(0)
    return torch.exp(-0.5 * (t * t).sum(-1))


def expand(rowptr, col, x, pseudo, mu, inv_sigma, reduce="sum"):
    """Z [n_dst, K * F] float64"""
    n, K, F = rowptr.numel() - 1, mu.shape[0], x.shape[1]
    w, xs, row = weights(pseudo, mu, inv_sigma), x.double()[col.long()], row_index(rowptr)
    z = torch.zeros(n, K, F, dtype=torch.float64)
    for k in range(K):
        z[:, k].index_add_(0, row, w[:, k:k + 1] * xs)
    return (z * row_scale(rowptr, reduce).view(-1, 1, 1)).reshape(n, K * F)


def gradients(rowptr, col, x, pseudo, mu, inv_sigma, g, reduce="sum"):
    """(grad_x [n_src, F], grad_pseudo [nnz, dim], grad_mu [K, dim], grad_inv_sigma [K, dim], terms): float64; terms = (mu_terms,
    sigma_terms), each [nnz, K, dim], the per-entry addends of the two parameter gradients."""
    n, K, F = rowptr.numel() - 1, mu.shape[0], x.shape[1]
    w, xs, row, c = weights(pseudo, mu, inv_sigma), x.double()[col.long()], row_index(rowptr), col.long()
    gs = (g.double() * row_scale(rowptr, reduce).unsqueeze(1)).view(n, K, F)[row]          # [nnz, K, F]
    gx = torch.zeros(x.shape[0], F, dtype=torch.float64).index_add_(0, c, (w.unsqueeze(-1) * gs).sum(1))
    p = (gs * xs.unsqueeze(1)).sum(-1)                                                      # [nnz, K]
    t = pseudo.double().unsqueeze(1) - mu.double().unsqueeze(0)                             # [nnz, K, dim]
    s = inv_sigma.double().unsqueeze(0)
    pw = (p * w).unsqueeze(-1)
    mu_terms = pw * t * s * s
    sigma_terms = -pw * t * t * s
    return gx, -mu_terms.sum(1), mu_terms.sum(0), sigma_terms.sum(0), (mu_terms, sigma_terms)


def edge_dots(rowptr, col, x, g, K, reduce="sum"):
    """P [nnz, K] float64 from the (unscaled) output gradient"""
    n, F = rowptr.numel() - 1, x.shape[1]
    gs = (g.double() * row_scale(rowptr, reduce).unsqueeze(1)).view(n, K, F)[row_index(rowptr)]
    return (gs * x.double()[col.long()].unsqueeze(1)).sum(-1)


def conditioning(terms):
    """max over the elements of sum_e |term| over max over the elements of |sum_e term|: how much larger the addends of a parameter
    gradient are than the gradient the bars are relative to"""
    return (terms.abs().sum(0).max() / terms.sum(0).abs().max()).item()


def layer(rowptr, col, x_src, x_dst, pseudo, mu, inv_sigma, fc_weight, res_weight, bias, reduce, residual):
    """GMMConv's output in float64, in DGL's own order: project x_j to K * out columns, weight per entry, reduce, sum over k."""
    n, K = rowptr.numel() - 1, mu.shape[0]
    out = fc_weight.shape[0] // K
    w, row = weights(pseudo, mu, inv_sigma), row_index(rowptr)
    proj = (x_src.double() @ fc_weight.double().t()).view(-1, K, out)[col.long()]           # [nnz, K, out]
    msg = (w.unsqueeze(-1) * proj).sum(1)
    h = torch.zeros(n, out, dtype=torch.float64).index_add_(0, row, msg) * row_scale(rowptr, reduce).unsqueeze(1)
    if residual:
        h = h + (x_dst.double() if res_weight is None else x_dst.double() @ res_weight.double().t())
    if bias is not None:
        h = h + bias.double()
    return h


def inputs(graph, F, K, dim, dtype, seed):
    """(x [n_src, F], pseudo fp32 [nnz, dim], mu fp32 [K, dim], inv_sigma fp32 [K, dim], g [n_dst, K * F]): pseudo uniform in [-1, 1],
    mu 0.5 N(0, 1), inv_sigma uniform in [0.5, 2], x and g N(0, 1) rounded to `dtype`."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(graph.n_cols, F, generator=gen).to(dtype)
    pseudo = torch.rand(graph.nnz, dim, generator=gen) * 2 - 1
    mu = 0.5 * torch.randn(K, dim, generator=gen)
    inv_sigma = 0.5 + 1.5 * torch.rand(K, dim, generator=gen)
    g = torch.randn(graph.n_rows, K * F, generator=gen).to(dtype)
    return x, pseudo, mu, inv_sigma, g
