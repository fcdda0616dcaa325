"""The oracle of the PNA tests: dgll_amd.ops_agg.multi_aggregate and nn.PNAConv restated with EXPLICIT per-edge messages
(x[col_k] + y[row_k]; for the layer M(cat(h_src[col_k], h_dst[row_k]))) reduced per row with torch's segment ops, then scaled; autograd
gives the gradients.  It does not use the decomposition into a source and a destination term, nothing of dgll_amd.ops_agg and nothing of
the layer's host path; the tests pass float64.

The variance is the centred form mean((m - mean)^2), so the reference has no cancellation of its own; the mean is formed about the
row's first message (first + mean(m - first)), so that a row of equal messages has exactly that value as its mean and exactly 0 as its
variance -- otherwise d sqrt(var + 1e-30) = 1e15 would meet the rounding residue of sum / count.  max / min are selected with the
kernel's tie rule (among the entries attaining the extreme the smallest source id, then that entry is gathered), which makes the
gradient routing the kernel's."""
import torch

AGGREGATORS = ("mean", "sum", "max", "min", "var", "std")
SCALERS = ("identity", "amplification", "attenuation")
STD_EPS = 1e-30


def rows_of(rowptr):
    """row [nnz]: the row of every entry."""
    n = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, device=rowptr.device), rowptr[1:] - rowptr[:-1])


def _extreme(msg, row, col, n, largest):
    """(value [n, F], arg [n, F]): the extreme message per row and column, gathered from the entry the tie rule selects; an empty row:
    0 and -1."""
    nnz, F = msg.shape
    if nnz == 0:
        return msg.new_zeros((n, F)), torch.full((n, F), -1, dtype=torch.int64)
    seg = row.unsqueeze(1).expand(nnz, F)
    m = msg.detach()
    ext = torch.full((n, F), -float("inf") if largest else float("inf"), dtype=msg.dtype).scatter_reduce(0, seg, m, "amax" if largest else "amin")
    hit = m == ext[row]
    big = int(col.max()) + 1
    arg = torch.full((n, F), big, dtype=torch.int64).scatter_reduce(0, seg, torch.where(hit, col.unsqueeze(1).expand(nnz, F), big), "amin")
    chosen = hit & (col.unsqueeze(1) == arg[row])                   # the same (source, row) pair stored twice: the first of them
    first = torch.full((n, F), nnz, dtype=torch.int64).scatter_reduce(0, seg, torch.where(chosen, torch.arange(nnz).unsqueeze(1).expand(nnz, F), nnz), "amin")
    empty = first == nnz
    value = msg.gather(0, first.clamp(max=nnz - 1))
    return torch.where(empty, torch.zeros_like(value), value), torch.where(empty, torch.full_like(arg, -1), arg)


def reduce_messages(msg, row, col, n, aggregators, scalers, delta, parts=None):
    """[n, S * A * F] from the per-edge messages msg [nnz, F] of the entries (row_k, col_k).  parts: a dict that receives the rows'
    'mean', 'var', 'argmax', 'argmin'."""
    nnz, F = msg.shape
    deg = torch.bincount(row, minlength=n)
    has = (deg > 0).unsqueeze(1)
    cnt = deg.clamp(min=1).to(msg.dtype).unsqueeze(1)
    start = torch.cumsum(deg, 0) - deg
    zeros = lambda: torch.zeros((n, F), dtype=msg.dtype)            # noqa: E731
    if nnz:
        first = msg[start.clamp(max=nnz - 1)] * has
        mean = first + zeros().index_add_(0, row, msg - first[row]) / cnt
        var = torch.relu(zeros().index_add_(0, row, (msg - mean[row]) ** 2) / cnt)
        total = zeros().index_add_(0, row, msg)
    else:
        mean, var, total = zeros(), zeros(), zeros()
    top, argmax = _extreme(msg, row, col, n, True)
    low, argmin = _extreme(msg, row, col, n, False)
    if parts is not None:
        parts.update(mean=mean.detach(), var=var.detach(), argmax=argmax, argmin=argmin)
    value = {"mean": mean, "sum": total, "max": top, "min": low, "var": var, "std": torch.sqrt(var + STD_EPS)}
    logd = torch.log(cnt + 1.0)
    scale = {"identity": torch.ones_like(logd), "amplification": logd / delta, "attenuation": delta / logd}
    return torch.cat([torch.where(has, scale[s] * value[a], torch.zeros_like(mean)) for s in scalers for a in aggregators], 1)


def multi_aggregate_reference(rowptr, col, x, y=None, aggregators=("mean", "max", "min", "std"),
                              scalers=("identity", "amplification", "attenuation"), delta=1.0, parts=None):
    row, c = rows_of(rowptr), col.long()
    msg = x[c] if y is None else x[c] + y[row]
    return reduce_messages(msg, row, c, rowptr.numel() - 1, aggregators, scalers, delta, parts)


def edge_messages(sd, rowptr, col, h_src, h_dst, num_towers):
    """the per-edge messages of every tower of a PNAConv with the state dict sd: a list of [nnz, Fi]"""
    row, c = rows_of(rowptr), col.long()
    fi = h_src.shape[1] // num_towers
    return [torch.cat([h_src[:, t * fi:(t + 1) * fi][c], h_dst[:, t * fi:(t + 1) * fi][row]], 1) @ sd["towers.%d.M.weight" % t].t()
            + sd["towers.%d.M.bias" % t] for t in range(num_towers)]


def pna_conv_reference(sd, rowptr, col, h_src, h_dst, aggregators, scalers, delta, num_towers=1, residual=True, snorm_n=None,
                       training=True, bn_eps=1e-5):
    """nn.PNAConv (dropout 0) from its state dict sd (float64 tensors; those that require grad receive gradients)."""
    row, c, n = rows_of(rowptr), col.long(), rowptr.numel() - 1
    fi = h_src.shape[1] // num_towers
    outs = []
    for t, msg in enumerate(edge_messages(sd, rowptr, col, h_src, h_dst, num_towers)):
        key = "towers.%d." % t
        h_neigh = reduce_messages(msg, row, c, n, aggregators, scalers, delta)
        h = torch.cat([h_dst[:, t * fi:(t + 1) * fi], h_neigh], 1) @ sd[key + "U.weight"].t() + sd[key + "U.bias"]
        if snorm_n is not None:
            h = h * snorm_n
        if training:
            mu, v = h.mean(0), h.var(0, unbiased=False)
        else:
            mu, v = sd[key + "batchnorm.running_mean"], sd[key + "batchnorm.running_var"]
        outs.append((h - mu) / torch.sqrt(v + bn_eps) * sd[key + "batchnorm.weight"] + sd[key + "batchnorm.bias"])
    h = torch.nn.functional.leaky_relu(torch.cat(outs, 1) @ sd["mixing_layer.0.weight"].t() + sd["mixing_layer.0.bias"])
    return h + h_dst if residual else h


def spread_features(n_src, F, seed):
    """x [n_src, F] float64 whose distinct values stay apart: per column a permutation pi of the sources,
    x[j, f] = (pi(j) + u) * 8 / n_src - 4 with u uniform in [0, 0.5): two sources differ by at least 4 / n_src in every column, so the
    smallest non-zero row variance is at least (2 / n_src)^2, with |x| <= 4."""
    gen = torch.Generator().manual_seed(seed)
    pi = torch.stack([torch.randperm(n_src, generator=gen) for _ in range(F)], 1).double()
    return (pi + 0.5 * torch.rand(n_src, F, generator=gen, dtype=torch.float64)) * 8.0 / n_src - 4.0
