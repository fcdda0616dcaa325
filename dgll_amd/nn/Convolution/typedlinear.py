"""TypedLinear: y_i = x_i . W[type_i], a linear map per row type (DGL's dgl.nn.TypedLinear; argument names and state dict as there).

| parameter | shape                                                         | present     |
|-----------|---------------------------------------------------------------|-------------|
| W         | [num_types, in, out] (None), [num_bases, in, out] ("basis")   | always      |
| coeff     | [num_types, num_bases]                                        | basis only  |

Initialisers as DGL's: W uniform in +-1/sqrt(in), coeff Xavier-uniform with the ReLU gain.  regularizer="basis" forms
W_r = sum_b coeff[r, b] W[b] as ONE product [R, B] x [B, in * out] on the dense kernels (dense.linear: differentiable there);
"bdd" is not built.  The typed product itself is ops_segmm: segment_mm when the rows are sorted by type (the segment lengths are taken
on the device, nothing is read back), gather_mm otherwise.  num_types has no upper limit.
"""
import math

import torch

from ... import dense, ops_segmm


class TypedLinear(torch.nn.Module):
    def __init__(self, in_size, out_size, num_types, regularizer=None, num_bases=None):
        super().__init__()
        if regularizer == "bdd":
            raise NotImplementedError('TypedLinear: regularizer="bdd" (block-diagonal decomposition) is not built; use "basis" or None')
        if regularizer not in (None, "basis"):
            raise ValueError('TypedLinear: regularizer must be None, "basis" or "bdd", got %r' % (regularizer,))
        self.in_size, self.out_size, self.num_types = int(in_size), int(out_size), int(num_types)
        self.regularizer = regularizer
        if regularizer == "basis":
            if num_bases is None or int(num_bases) < 1:
                raise ValueError('TypedLinear: regularizer="basis" needs num_bases >= 1')
            self.num_bases = int(num_bases)
            self.W = torch.nn.Parameter(torch.empty(self.num_bases, self.in_size, self.out_size))
            self.coeff = torch.nn.Parameter(torch.empty(self.num_types, self.num_bases))
        else:
            self.num_bases = None
            self.W = torch.nn.Parameter(torch.empty(self.num_types, self.in_size, self.out_size))
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.in_size)
        torch.nn.init.uniform_(self.W, -bound, bound)
        if self.regularizer == "basis":
            torch.nn.init.xavier_uniform_(self.coeff, gain=torch.nn.init.calculate_gain("relu"))

    def get_weight(self):
        """[num_types, in, out]: W itself, or coeff . W for the basis form."""
        if self.regularizer is None:
            return self.W
        flat = dense.linear(self.coeff, self.W.reshape(self.num_bases, self.in_size * self.out_size))
        return flat.reshape(self.num_types, self.in_size, self.out_size)

    def forward(self, x, x_type, sorted_by_type=False):
        """x [M, in], x_type [M] integers in [0, num_types) -> [M, out].  sorted_by_type: x_type is ascending (not checked)."""
        w = self.get_weight()
        if not sorted_by_type:
            return ops_segmm.gather_mm(x, w, idx_b=x_type)
        x_type = x_type.to(x.device)
        bounds = torch.searchsorted(x_type, torch.arange(self.num_types + 1, dtype=x_type.dtype, device=x.device))
        bounds[-1] = x.shape[0]                # every row belongs to a segment whatever the last types say
        seglen = bounds[1:] - bounds[:-1]
        return ops_segmm.segment_mm(x, w, seglen)

    def extra_repr(self):
        return "in_size=%d, out_size=%d, num_types=%d, regularizer=%r, num_bases=%r" % (self.in_size, self.out_size, self.num_types,
                                                                                        self.regularizer, self.num_bases)
