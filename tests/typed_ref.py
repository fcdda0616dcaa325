"""float64 restatements of the typed-edge aggregation (dgll_amd/ops_typed.py) and of RelGraphConv, with per-edge tensors and torch
autograd.  Neither touches the code under test: no dgll_amd import, host tensors only.

DGL is not installed here and the project this one was modelled on has no R-GCN, so there are no recorded outputs to compare with:
these functions restate DGL's documented module (dgl.nn.pytorch.conv.RelGraphConv: names, shapes and the order of operations)."""
import torch


def _rows(rowptr):
    rowptr = rowptr.long().cpu()
    n = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1]), n


def typed_spmm_reference(rowptr, col, etype, norm, x, coeff):
    """Z [n_rows, B * F] float64, Z[i, b, :] = sum over the entries e = (j -> i) of row i of norm_e coeff[etype_e, b] x_j.
    Differentiable in x, coeff and norm."""
    row, n = _rows(rowptr)
    x, coeff = x.double(), coeff.double()
    w = coeff[etype.long().cpu()]                                   # [nnz, B]
    if norm is not None:
        w = w * norm.double().reshape(-1, 1)
    xg = x[col.long().cpu()]                                        # [nnz, F]
    blocks = [torch.zeros(n, x.shape[1], dtype=torch.float64).index_add(0, row, w[:, b:b + 1] * xg) for b in range(coeff.shape[1])]
    return torch.cat(blocks, 1)


def edge_dots_reference(rowptr, col, x, dz, B):
    """P [nnz, B] float64: P[e, b] = <x_j, dz[i, b, :]> for e = (j -> i)."""
    row, _ = _rows(rowptr)
    F = x.shape[1]
    return torch.einsum("ef,ebf->eb", x.double()[col.long().cpu()], dz.double()[row].reshape(-1, B, F))


def relgraphconv_reference(rowptr, col, etype, norm, feat, weight, coeff=None, h_bias=None, loop_weight=None, ln_weight=None,
                           ln_bias=None, activation=None, ln_eps=1e-5):
    """The full layer in float64, one relation after another with that relation's own weight matrix (never through Z):
        h_i = sum_r sum_{e = (j -> i), etype_e = r} norm_e x_j W_r,    W_r = sum_b coeff[r, b] weight[b]   (coeff None: W_r = weight[r])
    then layer norm, + h_bias, + feat[:n_dst] loop_weight, activation -- DGL's order.  Arguments are the state-dict tensors."""
    row, n_dst = _rows(rowptr)
    col, etype = col.long().cpu(), etype.long().cpu()
    x, weight = feat.double(), weight.double()
    w_rel = weight if coeff is None else torch.einsum("rb,bio->rio", coeff.double(), weight)
    h = torch.zeros(n_dst, weight.shape[2], dtype=torch.float64)
    for r in range(w_rel.shape[0]):
        sel = (etype == r).nonzero().flatten()
        if sel.numel() == 0:
            continue
        msg = x[col[sel]] @ w_rel[r]
        if norm is not None:
            msg = msg * norm.double().reshape(-1, 1)[sel]
        h = h.index_add(0, row[sel], msg)
    if ln_weight is not None:
        h = torch.nn.functional.layer_norm(h, (h.shape[1],), ln_weight.double(), ln_bias.double(), ln_eps)
    if h_bias is not None:
        h = h + h_bias.double()
    if loop_weight is not None:
        h = h + x[:n_dst] @ loop_weight.double()
    if activation is not None:
        h = activation(h)
    return h
