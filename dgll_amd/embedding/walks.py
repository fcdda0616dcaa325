"""random_walks: uniform and node2vec walks over a device CSR (dgll_amd/csrc/walk.hip)."""
import torch

from .. import _lib
from ..graph import CSRGraph

MAX_ATTEMPTS = 1024          # rejection cap of the biased step; capped steps are counted in the info word
_ERRORS = {1: "a start node outside [0, N)", 2: "a column id outside [0, N)"}


def as_walk_graph(g, device=None):
    """Square CSRGraph on the device for a CSRGraph or a DGraph."""
    from ..data.dgraph import DGraph

    if isinstance(g, DGraph):
        g = g.to_csr()
    if not isinstance(g, CSRGraph):
        raise TypeError("g must be a CSRGraph or a DGraph, got %r" % type(g))
    if g.n_rows != g.n_cols:
        raise ValueError("walks need a square adjacency")
    return g if device is None else g.to(device)


def _rows_sorted(g):
    """True when every row's column ids ascend (CSRGraph.from_coo guarantees it); checked once per graph."""
    hit = getattr(g, "_rows_sorted", None)
    if hit is None:
        if g.nnz < 2:
            hit = True
        else:
            key = g.row_index() * g.n_cols + g.col.to(torch.int64)
            hit = bool((key[1:] >= key[:-1]).all())
        g._rows_sorted = hit
    return hit


def random_walks(g, starts, length, p=1.0, q=1.0, seed=0, first_walk_index=0, stream=None, info=None):
    """int32 [n, length] walks from `starts` (int64 device tensor), walks[:, 0] = starts; a node without out-edges ends its walk and
    every later entry is -1.  p = q = 1: uniform steps (DeepWalk); otherwise node2vec's second-order walk by rejection sampling,
    which needs ascending rows.  Walk i is a function of (seed, first_walk_index + i) only -- not of the batch it is drawn in.
    info: int64 [2] device tensor that collects {steps that hit the rejection cap, error bits} (see walk_info); reading it is the
    only host synchronisation, and it is the caller's."""
    if isinstance(g, CSRGraph) and not g.is_cuda:
        raise RuntimeError("dgll_amd.embedding runs on the GPU only (got a %s graph); there is no CPU fallback" % g.device)
    if not isinstance(starts, torch.Tensor) or not starts.is_cuda:
        raise RuntimeError("dgll_amd.embedding runs on the GPU only (starts must be a device tensor); there is no CPU fallback")
    g = as_walk_graph(g, starts.device)
    p, q, length = float(p), float(q), int(length)
    if not (p > 0.0 and q > 0.0):
        raise ValueError("node2vec p and q must be positive")
    if length < 1:
        raise ValueError("walk length must be >= 1")
    if (p != 1.0 or q != 1.0) and not _rows_sorted(g):
        raise ValueError("node2vec walks need a CSR whose rows ascend (CSRGraph.from_coo builds one)")
    if getattr(g, "_deg32", None) is None:
        g._deg32 = g.nnz < 2 ** 32 or int(g.degrees().max()) < 2 ** 32
    if not g._deg32:
        raise ValueError("a row with 2^32 or more entries")
    starts = starts.to(torch.int64).reshape(-1).contiguous()
    n = starts.numel()
    walks = torch.empty((n, length), dtype=torch.int32, device=starts.device)
    if info is None:
        info = torch.zeros(2, dtype=torch.int64, device=starts.device)
    _lib.launch("dgll_hip_random_walk", starts.device, g.rowptr.data_ptr(), g.col.data_ptr(), g.n_rows, starts.data_ptr(), n, length,
                int(first_walk_index) & 0xFFFFFFFFFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF, p, q, MAX_ATTEMPTS, walks.data_ptr(),
                info.data_ptr(), stream=stream)
    return walks


def walk_info(info):
    """Read an info tensor (one blocking copy): the number of steps that hit the rejection cap; raises on error bits."""
    capped, err = info.cpu().tolist()
    if err:
        raise RuntimeError("random walks: " + ", ".join(m for bit, m in _ERRORS.items() if err & bit))
    return capped
