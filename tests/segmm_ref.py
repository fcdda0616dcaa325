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


def gw_slab(m):
    """Rows per slab of the weight gradient: max(512, M / 128) rounded up to 16 (the workspace comment of dgll_amd/ops_segmm.py)."""
    return max(512, -(-(-(-m // 128)) // 16) * 16)


def plan_ref(seglen, m, unit):
    """(segoff, tileptr, partptr), R + 2 entries each, as the header comment of csrc/segment_mm.hip describes the tile list: lengths
    clamped to [0, M], offsets their exclusive prefix sum clamped to [0, M], element R the pseudo segment of the rows behind the last
    segment (segoff[R + 1] = M); tileptr the exclusive prefix of ceil(length / unit) with the total at R + 1; partptr the same prefix
    over the tiles of the segments that have more than one."""
    raw, segoff = 0, []
    for v in list(seglen) + [m]:
        segoff.append(min(raw, m))
        raw += min(max(int(v), 0), m)
    segoff.append(m)
    tileptr, partptr = [0], [0]
    for lo, hi in zip(segoff[:-1], segoff[1:]):
        t = -(-(hi - lo) // unit)
        tileptr.append(tileptr[-1] + t)
        partptr.append(partptr[-1] + (t if t > 1 else 0))
    return segoff, tileptr, partptr
