"""random_walks: uniform, node2vec and edge-weighted walks over a device CSR, and the alias tables of the weighted ones
(dgll_amd/csrc/walk.hip)."""
import torch

from .. import _lib
from ..graph import CSRGraph

MAX_ATTEMPTS = 1024          # rejection cap of the biased step; capped steps are counted in the info word
_ERRORS = {1: "a start node outside [0, N)", 2: "a column id outside [0, N)", 4: "an edge weight that is negative, NaN or infinite",
           8: "an alias index outside its row (the table was built for another graph)"}


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


def _rows_fit32(g):
    if getattr(g, "_deg32", None) is None:
        g._deg32 = g.nnz < 2 ** 32 or int(g.degrees().max()) < 2 ** 32
    if not g._deg32:
        raise ValueError("a row with 2^32 or more entries")


class AliasTable:
    """Per-row alias tables of a graph's edge values (dgll_hip_alias_build): `table` int32 [nnz, 2] on the device, the bits of
    {keep threshold T, alias index local to the row} of every edge.  8 bytes per edge; built once per graph (one lane per row)."""

    def __init__(self, table, nnz):
        if table.dtype != torch.int32 or tuple(table.shape) != (int(nnz), 2) or not table.is_contiguous():
            raise ValueError("table must be a contiguous int32 [nnz, 2] tensor")
        self.table, self.nnz = table, int(nnz)

    @classmethod
    def from_graph(cls, g):
        """The table of g.val on g's device, cached on the graph object.  Raises ValueError for a graph without values or with a
        negative, NaN or infinite one (one blocking read of the info word per graph)."""
        g = as_walk_graph(g)
        if g.val is None:
            raise ValueError("weighted walks need edge values (CSRGraph.val is None)")
        if not g.is_cuda:
            raise RuntimeError("dgll_amd.embedding runs on the GPU only (got a %s graph); there is no CPU fallback" % g.device)
        hit = getattr(g, "_alias", None)
        if hit is None:
            _rows_fit32(g)
            table = torch.empty((g.nnz, 2), dtype=torch.int32, device=g.device)
            scratch = torch.empty(3 * g.nnz, dtype=torch.int32, device=g.device)          # 12 bytes per edge
            info = torch.zeros(2, dtype=torch.int64, device=g.device)
            _lib.launch("dgll_hip_alias_build", g.device, g.rowptr.data_ptr(), g.val.data_ptr(), g.n_rows, g.nnz, scratch.data_ptr(),
                        scratch.numel() * 4, table.data_ptr(), info.data_ptr())
            try:
                walk_info(info)
            except RuntimeError as e:
                raise ValueError(str(e)) from None
            hit = g._alias = cls(table, g.nnz)
        return hit

    def numpy(self):
        """(T, alias): two uint32 [nnz] host arrays."""
        t = self.table.cpu().numpy().view("uint32")
        return t[:, 0].copy(), t[:, 1].copy()


def random_walks(g, starts, length, p=1.0, q=1.0, seed=0, first_walk_index=0, stream=None, info=None, weighted=False, alias=None):
    """int32 [n, length] walks from `starts` (int64 device tensor), walks[:, 0] = starts; a node without out-edges ends its walk and
    every later entry is -1.  p = q = 1: uniform steps (DeepWalk); otherwise node2vec's second-order walk by rejection sampling,
    which needs ascending rows.  Walk i is a function of (seed, first_walk_index + i) only -- not of the batch it is drawn in.
    info: int64 [2] device tensor that collects {steps that hit the rejection cap, error bits} (see walk_info); reading it is the
    only host synchronisation, and it is the caller's.
    weighted=True (or alias=an AliasTable of g): every step, the first included, draws the out-edge in proportion to its value
    (times node2vec's bias when p or q != 1); an edge of weight 0 is never taken and a row whose weights sum to 0 is a dead end.
    The table is built on first use and cached on the graph; a graph without values raises ValueError."""
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
    _rows_fit32(g)
    if alias is None and weighted:
        alias = AliasTable.from_graph(g)
    if alias is not None and (not isinstance(alias, AliasTable) or alias.nnz != g.nnz or alias.table.device != g.device):
        raise ValueError("alias must be an AliasTable of this graph, on its device")
    starts = starts.to(torch.int64).reshape(-1).contiguous()
    n = starts.numel()
    walks = torch.empty((n, length), dtype=torch.int32, device=starts.device)
    if info is None:
        info = torch.zeros(2, dtype=torch.int64, device=starts.device)
    tail = (g.n_rows, starts.data_ptr(), n, length, int(first_walk_index) & 0xFFFFFFFFFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF, p, q,
            MAX_ATTEMPTS, walks.data_ptr(), info.data_ptr())
    if alias is None:
        _lib.launch("dgll_hip_random_walk", starts.device, g.rowptr.data_ptr(), g.col.data_ptr(), *tail, stream=stream)
    else:
        _lib.launch("dgll_hip_random_walk_weighted", starts.device, g.rowptr.data_ptr(), g.col.data_ptr(), alias.table.data_ptr(), *tail,
                    stream=stream)
    return walks


def walk_info(info):
    """Read an info tensor (one blocking copy): the number of steps that hit the rejection cap; raises on error bits."""
    capped, err = info.cpu().tolist()
    if err:
        raise RuntimeError("random walks: " + ", ".join(m for bit, m in _ERRORS.items() if err & bit))
    return capped
