"""Skip-gram with negative sampling over a batch of walks (dgll_amd/csrc/sgns.hip)."""
import torch

from .. import _lib
from ..graph import CSRGraph

_MASK = 0xFFFFFFFFFFFFFFFF


class NoiseTable:
    """Noise distribution of the negative draws as a fixed-point cumulative table: cdf[i] = round(2^32 * sum_{j <= i} w_j / sum w),
    uint64 bits in an int64 tensor, built in float64 torch; cdf[-1] = 2^32.  A draw is searchsorted(cdf, x, side="right") on one
    32-bit Philox word, so a node of zero weight (cdf[i] == cdf[i - 1]) is never drawn."""

    def __init__(self, weights):
        w = torch.as_tensor(weights).to(torch.float64).reshape(-1)
        if w.numel() == 0 or bool((w < 0).any()) or not bool(torch.isfinite(w).all()) or float(w.sum()) <= 0.0:
            raise ValueError("noise weights must be finite, non-negative and not all zero")
        c = torch.cumsum(w, 0)
        cdf = torch.round(c / c[-1] * 4294967296.0).to(torch.int64)
        # everything from the last node of positive weight on is exactly 2^32 (the tail after it has no mass)
        last = int(torch.nonzero(w > 0).max())
        cdf[last:] = 4294967296
        self.cdf = cdf.contiguous()
        self.n = int(w.numel())

    @classmethod
    def from_graph(cls, g, power=0.75):
        """in-degree^power (word2vec's unigram^0.75 with a node's count = the times it is a walk's next step candidate)."""
        indeg = torch.bincount(g.col.to(torch.int64), minlength=g.n_cols).to(torch.float64)
        if float(indeg.sum()) == 0.0:
            indeg = torch.ones_like(indeg)
        return cls(indeg.pow(power))

    def to(self, device):
        self.cdf = self.cdf.to(device)
        return self

    @property
    def device(self):
        return self.cdf.device


def _check(walks, noise, window, negatives):
    if not isinstance(walks, torch.Tensor) or not walks.is_cuda or not noise.cdf.is_cuda:
        raise RuntimeError("dgll_amd.embedding runs on the GPU only (walks and the noise table must be on the device); there is no CPU fallback")
    if walks.dtype != torch.int32 or walks.dim() != 2:
        raise TypeError("walks must be an int32 [n, L] tensor")
    if int(window) < 1 or int(negatives) < 0:
        raise ValueError("window >= 1 and negatives >= 0")
    return walks.contiguous()


def sgns_negatives(walks, window, negatives, noise, seed, first_walk_index=0):
    """The negatives sgns_step draws: int32 [n, L, 2 window, negatives], -1 where there is no pair.  Slot s of centre j is position
    j + o, o = -window..-1, 1..window."""
    walks = _check(walks, noise, window, negatives)
    n, L = walks.shape
    W, K = int(window), int(negatives)
    out = torch.empty((n, L, 2 * W, K), dtype=torch.int32, device=walks.device)
    if out.numel() == 0:
        return out
    _lib.launch("dgll_hip_sgns_negatives", walks.device, walks.data_ptr(), n, L, W, K, noise.cdf.data_ptr(), noise.n,
                int(first_walk_index) & _MASK, int(seed) & _MASK, out.data_ptr())
    return out


def sgns_step(W_in, W_out, walks, window, negatives, noise, lr, seed, first_walk_index=0):
    """One batch-synchronous SGD step on sum_pairs [-log sigma(u_c.v_t) - sum_k log sigma(-u_c.v_nk)] (a sum, not a mean), in place on
    the fp32 [N, D] tables W_in (centres) and W_out (contexts and negatives); every gradient is taken at the weights as they
    were when the step began.  Returns the loss sum at those weights as a float64 device scalar (no host synchronisation)."""
    walks = _check(walks, noise, window, negatives)
    for t in (W_in, W_out):
        if not t.is_cuda:
            raise RuntimeError("dgll_amd.embedding runs on the GPU only (got a %s table); there is no CPU fallback" % t.device)
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous():
            raise TypeError("the tables must be contiguous fp32 [N, D] tensors")
    if W_in.shape != W_out.shape or W_in.shape[0] != noise.n:
        raise ValueError("W_in, W_out and the noise table must agree on N (and D)")
    n, L = walks.shape
    N, D = W_in.shape
    W, K = int(window), int(negatives)
    dev = walks.device
    loss = torch.zeros((), dtype=torch.float64, device=dev)
    if n == 0:
        return loss
    slots = n * L * 2 * W * (1 + K)
    g = torch.empty(slots, dtype=torch.float32, device=dev)
    tgt = torch.empty(slots, dtype=torch.int32, device=dev)
    delta = torch.empty(n * L * D, dtype=torch.float32, device=dev)
    _lib.launch("dgll_hip_sgns_step", dev, W_in.data_ptr(), W_out.data_ptr(), N, D, walks.data_ptr(), n, L, W, K, noise.cdf.data_ptr(),
                int(first_walk_index) & _MASK, int(seed) & _MASK, float(lr), g.data_ptr(), tgt.data_ptr(), delta.data_ptr(), loss.data_ptr())
    return loss
