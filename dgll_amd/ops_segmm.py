"""Grouped dense products, y_i = x_i . W[type_i] over a set of rows (DGL's dgl.ops.segment_mm / gather_mm): csrc/segment_mm.hip.

    segment_mm(a, b, seglen_a) -> c [M, N]      rows [off_r, off_r + seglen_a[r]) of a [M, K] times b[r] of b [R, K, N]
    gather_mm(a, b, idx_b=...)  -> c [M, N]      c[i] = a[i] . b[idx_b[i]], idx_b in any order

bf16 or fp32 operands on the GPU, fp32 accumulation on the matrix cores, output in the dtype of a; b may be an fp32 parameter under
bf16 activations (the pack launch casts it, as dense.wcast allows elsewhere).  Each operator is ONE autograd node whose three
products run on the kernels of this feature: forward, grad_a = segment_mm(g, b^T) (the same kernel, the weights packed from the
other pair of strides: no transposed copy of b) and grad_b[r] = a_r^T . g_r in fp32 (zero for an empty segment; slab partials
summed in slab order).  No float atomics: two runs give the same bits.

Nothing is read back from the device.  A device seglen_a is used as it is: the launch forms the offsets and clamps them to [0, M]; rows
that no segment covers come out as zeros.  A host seglen_a is checked (non-negative, sum == M).  gather_mm sorts the types on the
device (stable torch.sort), takes the segment bounds with searchsorted and hands the sort permutation to the kernels as their row
index: there is no permuted copy of a and no un-permute pass over c.  The packed copy of the weights is bounded: segments are run
in ranges whose packed matrices fit _PACK_BYTES.

Host tensors (the layers' CPU logic, the tests' reference path) take a plain torch loop.
"""
import torch

from . import _lib
from .ops import alloc_features, as_rows16

_PACK_BYTES = 4 << 20          # packed weights alive at a time (one matrix at the least)
_WORKSPACE = {}                # (device, stream) -> uint8 scratch of the weight gradient (slab partials, at most (2 M / slab + 2) K N fp32 with
                               # slab = max(512, M / 128): 33 MiB at M = 2^15 and 66 MiB at M = 2^20 for K = N = 256), grown on demand and kept


def _code(dtype):
    if dtype == torch.float32:
        return _lib.F32
    if dtype == torch.bfloat16:
        return _lib.BF16
    raise TypeError("segment_mm / gather_mm take float32 or bfloat16 matrices, got %s" % dtype)


def _index_arg(t):
    """(pointer, bytes per entry) of an int32 / int64 device vector, (None, 8) for None."""
    return (None, 8) if t is None else (t.data_ptr(), t.element_size())


def _rows16(x):
    return as_rows16(x if x.stride(1) == 1 else x.contiguous())


def _product_raw(a, b, seglen, rows, transpose, out=None):
    """c[rows of segment r] = a[rows of segment r] . (b[r]^T if transpose else b[r]); a rows16, seglen / rows device vectors.
    out: an [M, N] device tensor of a's dtype with contiguous rows on any pitch, written instead of a fresh one."""
    m, k = a.shape
    n = b.shape[1] if transpose else b.shape[2]
    R = b.shape[0]
    dev = a.device
    if out is not None and (out.shape != (m, n) or out.dtype != a.dtype or out.stride(1) != 1 or out.device != dev):
        raise ValueError("out must be a [M, N] device tensor of a's dtype with contiguous rows")
    c = alloc_features(m, n, a.dtype, dev, pad_to=16 // a.element_size()) if out is None else out
    if m == 0 or n == 0:
        return c
    if k == 0 or R == 0:
        return c.zero_()
    code, bcode = _code(a.dtype), _code(b.dtype)
    b = b.detach()
    sr, sk, sn = (b.stride(0), b.stride(2), b.stride(1)) if transpose else b.stride()
    ws = torch.empty(int(_lib.lib.dgll_hip_segment_mm_workspace(R)), dtype=torch.uint8, device=dev)
    (len_ptr, len_bytes), (row_ptr, row_bytes) = _index_arg(seglen), _index_arg(rows)
    first = 1                  # the tile list is formed by the first launch and reused by the further ranges / column blocks
    for n0 in range(0, n, 256):
        nn = min(256, n - n0)
        per = int(_lib.lib.dgll_hip_segment_mm_packed_bytes(1, k, nn, code))
        step = max(1, _PACK_BYTES // per)
        for r0 in range(0, R, step):
            rr = min(step, R - r0)
            packed = torch.empty(rr * per, dtype=torch.uint8, device=dev)
            _lib.launch("dgll_hip_segment_mm_pack", dev, b.data_ptr() + (r0 * sr + n0 * sn) * b.element_size(), bcode, sr, sk, sn, rr, k, nn,
                        code, packed.data_ptr())
            _lib.launch("dgll_hip_segment_mm", dev, a.data_ptr(), a.stride(0), code, packed.data_ptr(), len_ptr, len_bytes, R, row_ptr,
                        row_bytes, c.data_ptr() + n0 * c.element_size(), c.stride(0), m, k, nn, r0, r0 + rr, first, ws.data_ptr(), ws.numel())
            first = 0
            del packed                 # (stream-ordered reuse: the next range's copy may take this one's memory)
    return c


def _gradw_raw(a, g, seglen, rows, R):
    """fp32 [R, K, N]: a_r^T . g_r per segment; a, g rows16 of one dtype."""
    m, k = a.shape
    n = g.shape[1]
    dev = a.device
    gw = torch.empty((R, k, n), dtype=torch.float32, device=dev)
    if R == 0 or k == 0 or n == 0:
        return gw
    code = _code(a.dtype)
    need = int(_lib.lib.dgll_hip_segment_mm_gradw_workspace(m, R, k, min(n, 256)))
    key = (dev.index, _lib.raw_stream(dev))
    ws = _WORKSPACE.get(key)
    if ws is None or ws.numel() < need:
        ws = _WORKSPACE[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    (len_ptr, len_bytes), (row_ptr, row_bytes) = _index_arg(seglen), _index_arg(rows)
    for n0 in range(0, n, 256):
        nn = min(256, n - n0)
        _lib.launch("dgll_hip_segment_mm_gradw", dev, a.data_ptr(), a.stride(0), g.data_ptr() + n0 * g.element_size(), g.stride(0), code,
                    len_ptr, len_bytes, R, row_ptr, row_bytes, gw.data_ptr() + n0 * 4, k * n, n, m, k, nn, ws.data_ptr(), ws.numel())
    return gw


class _GroupedMM(torch.autograd.Function):
    """One node for both operators: seglen (device, int32 / int64) and rows (device row index or None) describe the grouping."""

    @staticmethod
    def forward(ctx, a, b, seglen, rows):
        a16 = _rows16(a)
        ctx.save_for_backward(a16, b, seglen, rows)
        return _product_raw(a16, b, seglen, rows, transpose=False)

    @staticmethod
    def backward(ctx, g):
        a, b, seglen, rows = ctx.saved_tensors
        g = _rows16(g.to(a.dtype))
        ga = _product_raw(g, b, seglen, rows, transpose=True) if ctx.needs_input_grad[0] else None
        gb = _gradw_raw(a, g, seglen, rows, b.shape[0]).to(b.dtype) if ctx.needs_input_grad[1] else None
        return ga, gb, None, None


def _check(a, b):
    if a.dim() != 2 or b.dim() != 3 or a.shape[1] != b.shape[1]:
        raise ValueError("a must be [M, K] and b [R, K, N]; got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if a.device != b.device:
        raise ValueError("a and b must be on one device")
    if a.is_cuda:                    # (host tensors take torch, in any float type)
        _code(a.dtype), _code(b.dtype)


def _int_vector(t, name):
    if t.dim() != 1 or t.is_floating_point() or t.dtype == torch.bool:
        raise TypeError("%s must be a 1-D integer tensor" % name)
    return t.contiguous() if t.dtype in (torch.int32, torch.int64) else t.to(torch.int64)


def segment_mm(a, b, seglen_a):
    """c [M, N]: rows [off_r, off_r + seglen_a[r]) of a [M, K] times b[r] (b [R, K, N]), off the exclusive prefix sum: DGL's contract.
    seglen_a: [R] integers.  On the host it is checked (non-negative, sum == M; ValueError).  On the device it is used as it is, with
    no synchronisation: segments are clamped to the rows there are, and rows that no segment covers are zeros."""
    _check(a, b)
    seglen_a = _int_vector(torch.as_tensor(seglen_a), "seglen_a")
    if seglen_a.numel() != b.shape[0]:
        raise ValueError("seglen_a has %d entries but b holds %d matrices" % (seglen_a.numel(), b.shape[0]))
    if not seglen_a.is_cuda:
        lens = seglen_a.tolist()
        if any(v < 0 for v in lens) or sum(lens) != a.shape[0]:
            raise ValueError("seglen_a must be non-negative and sum to the %d rows of a; got sum %d" % (a.shape[0], sum(lens)))
        if not a.is_cuda:
            out = a.new_zeros((a.shape[0], b.shape[2]))
            off = 0
            for r, n in enumerate(lens):
                out[off:off + n] = torch.mm(a[off:off + n], b[r].to(a.dtype))
                off += n
            return out
        seglen_a = seglen_a.to(a.device)
    elif not a.is_cuda:
        raise ValueError("a device seglen_a needs device operands")
    return _GroupedMM.apply(a, b, seglen_a, None)


def gather_mm(a, b, *, idx_b):
    """c [M, N] with c[i] = a[i] . b[idx_b[i]]; idx_b: [M] integers in [0, R), any order.  On the GPU: a stable device sort of idx_b, the
    segment bounds by searchsorted, and the sort permutation as the kernels' row index -- no host synchronisation, no permuted copy
    of a, no un-permute pass over c.

    UNLIKE DGL, a device idx_b is NOT range-checked: reporting an error would need a read-back, which this call never does (it can
    be captured).  An entry outside [0, R) is clamped into it and its row is multiplied by b[0] or b[R - 1] -- a wrong number, not a
    fault and not an exception.  Check `idx_b.min() >= 0 and idx_b.max() < R` yourself where the types come from outside.  A host
    idx_b (host operands) is indexed by torch, which raises."""
    _check(a, b)
    idx_b = _int_vector(idx_b, "idx_b")
    if idx_b.numel() != a.shape[0]:
        raise ValueError("idx_b has %d entries but a has %d rows" % (idx_b.numel(), a.shape[0]))
    if not a.is_cuda:
        return torch.bmm(a.unsqueeze(1), b[idx_b.long()].to(a.dtype)).squeeze(1)
    R = b.shape[0]
    if R == 0 or a.shape[0] == 0:
        return a.new_zeros((a.shape[0], b.shape[2])) + 0 * (a.sum() + b.sum())      # (empty, but still a node of the autograd graph)
    ids, perm = torch.sort(idx_b.to(a.device).clamp(0, R - 1), stable=True)
    bounds = torch.searchsorted(ids, torch.arange(R + 1, dtype=ids.dtype, device=a.device))
    del ids
    return _GroupedMM.apply(a, b, bounds[1:] - bounds[:-1], perm)
