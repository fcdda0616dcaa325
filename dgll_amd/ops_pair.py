"""Scores of arbitrary node pairs (link prediction's dot-product predictor): dgll_amd/csrc/edge_pred.hip.

    pair_dot(h, batch_or_pairs) -> fp32 [P],  score[p] = <h[src_p], h[dst_p]>

h: [M, F] fp32 or bf16 on the GPU, any row pitch (one copy into 16-byte rows when needed: ops.as_rows16).  batch_or_pairs: a
sampling.edge.PairBatch (its `pairs`, M = len(output_nodes)) or an integer tensor [P, 2] of (src, dst) rows of h (checked against M
once, one device -> host read).  Differentiable in h: grad_h[i] = sum over the pair slots holding i of g[p] * h[other endpoint], a
gather over the pair list's incidence CSR (PairBatch.incidence(): built once per batch, by a sort) in a fixed order with fp32
accumulation, written in h's dtype.  No float atomics: two runs give the same bits.
"""
import torch

from . import _lib
from .ops import _dtype_code, _require_cuda, alloc_features, as_rows16


def pair_dot_raw(h, pairs):
    """score fp32[P] with no autograd; h as as_rows16 leaves it, pairs int32[P, 2] contiguous on h's device."""
    n_pairs = int(pairs.shape[0])
    score = torch.empty(n_pairs, dtype=torch.float32, device=h.device)
    if n_pairs:
        _lib.launch("dgll_hip_pair_dot", h.device, h.data_ptr(), h.stride(0), h.shape[0], h.shape[1], _dtype_code(h), pairs.data_ptr(),
                    n_pairs, score.data_ptr(), tag=lambda: ("pair_dot", h.shape[1], str(h.dtype), n_pairs))
    return score


def pair_dot_bwd_raw(h, incidence, n_pairs, g):
    """grad_h [M, F] of h's dtype (rows on a 16-byte pitch) from the score gradient g fp32[P]."""
    rowptr, pair, other = incidence
    per = 16 // h.element_size()
    grad = alloc_features(h.shape[0], h.shape[1], h.dtype, h.device, pad_to=per)
    if n_pairs == 0:
        return grad.zero_()
    _lib.launch("dgll_hip_pair_dot_bwd", h.device, h.data_ptr(), h.stride(0), h.shape[0], h.shape[1], _dtype_code(h), rowptr.data_ptr(),
                pair.data_ptr(), other.data_ptr(), n_pairs, g.data_ptr(), grad.data_ptr(), grad.stride(0),
                tag=lambda: ("pair_dot_bwd", h.shape[1], str(h.dtype), n_pairs))
    return grad


class _PairDot(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, pairs, incidence):
        hr = as_rows16(h.detach())
        ctx.pairs, ctx.incidence = pairs, incidence
        ctx.save_for_backward(hr)
        return pair_dot_raw(hr, pairs)

    @staticmethod
    def backward(ctx, g):
        (hr,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        inc = ctx.incidence() if callable(ctx.incidence) else ctx.incidence
        return pair_dot_bwd_raw(hr, inc, int(ctx.pairs.shape[0]), g.to(torch.float32).contiguous()), None, None


def pair_dot(h, batch_or_pairs):
    """score[p] = <h[src_p], h[dst_p]> as fp32 [P]; see the module text."""
    from .sampling.edge import PairBatch, incidence_of

    _require_cuda(h)
    if h.dim() != 2 or h.shape[0] == 0 or h.shape[1] == 0:
        raise ValueError("pair_dot expects a non-empty matrix h [M, F]")
    _dtype_code(h)
    if isinstance(batch_or_pairs, PairBatch):
        batch = batch_or_pairs
        if int(batch.output_nodes.numel()) != h.shape[0]:
            raise ValueError("h has %d rows but the batch has %d output nodes" % (h.shape[0], int(batch.output_nodes.numel())))
        pairs, incidence = batch.pairs, batch.incidence            # the bound method: built on first use, in the backward pass
    else:
        pairs = batch_or_pairs
        if not isinstance(pairs, torch.Tensor) or pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.is_floating_point():
            raise ValueError("pairs must be an integer tensor [P, 2] of (src, dst) rows of h")
        _require_cuda(pairs)
        if pairs.numel() and (int(pairs.min()) < 0 or int(pairs.max()) >= h.shape[0]):
            raise ValueError("pairs: a row index outside [0, %d)" % h.shape[0])
        pairs = pairs.to(torch.int32).contiguous()
        m = h.shape[0]
        incidence = lambda: incidence_of(pairs, m)      # noqa: E731
    if pairs.device != h.device:
        raise ValueError("h and the pairs must be on the same device")
    return _PairDot.apply(h, pairs, incidence)
