"""float64 reference of the grouped products (dgll_amd.ops_segmm), a loop over the types with torch on the CPU."""
import torch


def grouped_refs(a, b, g, idx):
    """(c, grad_a, grad_b) for c[i] = a[i] . b[idx[i]] and the output gradient g: float64 [M, K], [R, K, N], [M, N]; idx int64 [M].
    A row whose idx is outside [0, R) multiplies nothing: zeros."""
    c, ga, gb = torch.zeros_like(g), torch.zeros_like(a), torch.zeros_like(b)
    for r in range(b.shape[0]):
        m = idx == r
        c[m] = a[m] @ b[r]
        ga[m] = g[m] @ b[r].t()
        gb[r] = a[m].t() @ g[m]
    return c, ga, gb


def segment_ids(seglen):
    return torch.repeat_interleave(torch.arange(len(seglen)), torch.as_tensor(seglen))
