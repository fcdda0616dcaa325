"""Subgraph samplers: one induced subgraph per batch, on the device (dgll_amd/csrc/subgraph.hip).

DGL's second family of samplers (ShaDowKHopSampler, SAINTSampler, ClusterGCNSampler) hands a GNN of any depth ONE graph per batch
-- the subgraph induced by the batch's node set -- and the model runs its ordinary full-graph layers on it (fused SAGE / GCN / GAT
over a CSRGraph, no per-layer blocks).  CommunityBatchLoader covers the contiguous-range case; this module induces on any node set.

    node_subgraph(graph, nodes, normalize=None, return_eids=False, workspace=None) -> CSRGraph  |  (CSRGraph, eids)

graph: a square CSRGraph on the device (rows in any order, parallel entries allowed).  nodes: distinct ids in [0, N), any order
(tensor, array or list).  The result has n_rows = n_cols = len(nodes): row i is row nodes[i] of the parent, restricted to the
entries whose column is in `nodes`, IN THE PARENT'S ORDER, the column rewritten to its position in `nodes`.  normalize=None: the
parent's values of the kept entries (no values when the parent has none); "row": 1 / (kept entries of the row).  eids: int64, the
parent's entry index of every kept entry.  workspace: a SubgraphWorkspace of the parent (one 8-byte tag per node, reused from call
to call without clearing); None allocates one for the call.  The kernels run on the CURRENT stream with one blocking device -> host
read (the number of kept entries and the error bits); duplicate or out-of-range nodes and a column id outside [0, N) raise
ValueError.  Two calls give the same bits.

    ShaDowKHopSampler(fanouts, g=None, prob=None, normalize="row", device=None)
        sample(g, seed_nodes) / sample_seeded(g, seed_nodes, seed) -> (input_nodes, output_nodes, subgraph)

wraps NeighborSampler(fanouts, g, prob=prob, norm=None): input_nodes are the nodes its blocks reach (the destinations first, so the
seeds are rows 0 .. len(seed_nodes) - 1 of the subgraph, in order) and subgraph = node_subgraph(sampler.graph, input_nodes).  With
prob= the graph is the neighbour sampler's bound graph (zero-weight entries removed).  Seeding, locking and the stream are
NeighborSampler's.

    SAINTSampler(mode, budget, g=None, normalize="row", device=None)
        sample(g=None, indices=None) / sample_seeded(g, seed) -> (nodes, subgraph), nodes ascending

mode "node": `budget` draws of a node in proportion to its row length (its in-degree in a CSR of in-neighbours), with replacement
-- DGL's multinomial(in_degrees, budget, replacement=True); "edge": `budget` entries drawn uniformly, both endpoints; "walk":
budget = (num_roots, length), num_roots uniform roots and a uniform random walk of `length` steps from each
(dgll_hip_random_walk with p = q = 1, first_walk_index 0 and the same seed; a walk ends at a node without entries).  The node set
is the distinct nodes, ascending.  Draw i uses Philox4x32-10 with key = seed and counter (i, 0, mode): see include/dgll_hip.h.
sample() ignores `indices`, as DGL does, and draws its seed from numpy's global generator.

Out of scope: GraphSAINT's pre-sampled loss / aggregator normalisation (DGL's SAINTSampler has none either), MiniBatchPipeline
integration, heterogeneous graphs, a device transpose of the batch graph (CSRGraph.transpose stays the lazy torch sort).
"""
import threading

import numpy as np
import torch

from .. import _lib
from ..graph import CSRGraph
from .layerwise import _as_device_csr
from .neighbor import NeighborSampler

LONG_ROW = int(_lib.lib.dgll_hip_sg_long_row())
_INFO_WORDS = 8              # subgraph.hip: {count, -, error bits, ...}
_ERRORS = {1: "a node id outside [0, N)", 2: "a column id of the graph outside [0, N)", 4: "a duplicate node"}
_MODES = {"node": 1, "edge": 2, "walk": 3}
_WALK_ATTEMPTS = 1024        # dgll_hip_random_walk's floor; unused when p == q == 1 (attempt 0 is taken)


def _check_normalize(normalize):
    if normalize not in ("row", None):
        raise ValueError("normalize must be 'row' or None")


def _raise_for(err, what):
    if err:
        raise ValueError(what + ": " + ", ".join(m for bit, m in _ERRORS.items() if err & bit))


class SubgraphWorkspace:
    """The persistent per-graph buffer of node_subgraph: one 8-byte tag per node (epoch << 32 | local id; starts zeroed, never
    cleared) and the epoch counter.  One call at a time uses it."""

    def __init__(self, n, device):
        self.n, self.device = int(n), torch.device(device)
        if not 0 < self.n < 2 ** 31:
            raise ValueError("the graph needs between 1 and 2^31 - 1 nodes")
        self.tag = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        self.epoch = 0

    def next_epoch(self):
        self.epoch = self.epoch % 0xFFFFFFFF + 1
        return self.epoch


def _node_tensor(nodes, device):
    if isinstance(nodes, torch.Tensor):
        t = nodes.detach().to(torch.int64)
    else:
        t = torch.as_tensor(np.asarray(nodes, dtype=np.int64))
    return t.reshape(-1).to(device).contiguous()


def node_subgraph(graph, nodes, normalize=None, return_eids=False, workspace=None):
    """The subgraph of `graph` induced by `nodes` with local ids (module docstring)."""
    _check_normalize(normalize)
    if not isinstance(graph, CSRGraph):
        raise TypeError("graph must be a CSRGraph, got %r" % type(graph))
    if graph.n_rows != graph.n_cols:
        raise ValueError("node_subgraph needs a square graph, got %d x %d" % (graph.n_rows, graph.n_cols))
    if not graph.is_cuda:
        raise RuntimeError("node_subgraph runs on the GPU: move the graph to the device (graph.to(device))")
    dev, n = graph.device, graph.n_rows
    ws = SubgraphWorkspace(n, dev) if workspace is None else workspace
    if ws.n != n or ws.device != dev:
        raise ValueError("the workspace belongs to another graph (%d nodes on %s)" % (ws.n, ws.device))
    nodes = _node_tensor(nodes, dev)
    m = int(nodes.numel())
    rowptr = torch.empty(m + 1, dtype=torch.int64, device=dev)
    info = torch.empty(_INFO_WORDS, dtype=torch.int64, device=dev)
    epoch = ws.next_epoch()
    head = (graph.rowptr.data_ptr(), _lib.ptr(graph.col) if graph.nnz else None)
    _lib.launch("dgll_hip_sg_count", dev, *head, n, graph.nnz, nodes.data_ptr() if m else None, m, ws.tag.data_ptr(), epoch, rowptr.data_ptr(),
                info.data_ptr())
    nnz, _, err = info.cpu().tolist()[:3]           # the one blocking read
    _raise_for(err, "node_subgraph")
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    copy_val = normalize is None and graph.val is not None
    val = torch.empty(nnz, dtype=torch.float32, device=dev) if (copy_val or normalize == "row") else None
    eid = torch.empty(nnz, dtype=torch.int64, device=dev) if return_eids else None
    if nnz:
        _lib.launch("dgll_hip_sg_fill", dev, head[0], head[1], graph.val.data_ptr() if copy_val else None, n, graph.nnz, nodes.data_ptr(), m,
                    ws.tag.data_ptr(), epoch, rowptr.data_ptr(), nnz, col.data_ptr(), _lib.ptr(val), _lib.ptr(eid), info.data_ptr())
    sub = CSRGraph(rowptr, col, val, m, m, check=False)
    return (sub, eid) if return_eids else sub


class ShaDowKHopSampler:
    def __init__(self, fanouts, g=None, prob=None, normalize="row", device=None):
        _check_normalize(normalize)
        self.normalize = normalize
        self.sampler = NeighborSampler(fanouts, g, prob=prob, norm=None, device=device)
        self.fanouts = self.sampler.fanouts
        self._workspace = None

    @property
    def graph(self):
        return self.sampler.graph

    def sample(self, g, seed_nodes):
        """(input_nodes, output_nodes, subgraph) under a seed drawn from numpy's global generator."""
        seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
        return self.sample_seeded(g, seed_nodes, seed)

    def sample_seeded(self, g, seed_nodes, seed):
        """sample() under an explicit 64-bit seed: bit-identical output for the same (graph, seed nodes, seed)."""
        input_nodes, output_nodes, _ = self.sampler.sample_seeded(g, seed_nodes, seed)
        s = self.sampler
        with s._lock:                       # the neighbour sampler's lock also guards the tags
            if self._workspace is None:
                self._workspace = SubgraphWorkspace(s.num_nodes, s.device)
            with torch.cuda.device(s.device), torch.cuda.stream(s.stream):
                sub = node_subgraph(s.graph, input_nodes, self.normalize, workspace=self._workspace)
                s.stream.synchronize()
        return input_nodes, output_nodes, sub


class SAINTSampler:
    def __init__(self, mode, budget, g=None, normalize="row", device=None):
        if mode not in _MODES:
            raise ValueError("mode must be 'node', 'edge' or 'walk'")
        _check_normalize(normalize)
        if mode == "walk":
            try:
                roots, length = (int(b) for b in budget)
            except (TypeError, ValueError):
                raise ValueError("mode 'walk' needs budget = (num_roots, length)") from None
            if roots < 1 or length < 1:
                raise ValueError("mode 'walk' needs num_roots >= 1 and length >= 1")
            if roots >= 2 ** 31 or roots * (length + 1) >= 2 ** 31:
                raise ValueError("the walk matrix holds fewer than 2^31 entries")
            self.budget, self.length = roots, length
        else:
            if isinstance(budget, (tuple, list)) or int(budget) != budget:
                raise ValueError("mode %r needs an integer budget" % mode)
            if not 1 <= int(budget) < 2 ** 31:
                raise ValueError("budget must be in [1, 2^31)")
            self.budget, self.length = int(budget), 0
        self.mode, self.normalize = mode, normalize
        self._device_arg = device
        self.graph = None
        self._lock = threading.Lock()
        if g is not None:
            self._bind(g)

    def _bind(self, g):
        if isinstance(g, CSRGraph):             # what needs no device is refused first
            if g.n_rows != g.n_cols:
                raise ValueError("the adjacency must be square")
            if self.mode != "walk" and g.nnz == 0:
                raise ValueError("mode %r draws entries of the graph and it has none" % self.mode)
        device = self._device_arg
        if device is None:
            if isinstance(g, CSRGraph) and g.is_cuda:
                device = g.device
            elif not torch.cuda.is_available():
                raise RuntimeError("SAINTSampler runs on the GPU and none is available: pass a graph on the device or device=")
            else:
                device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("SAINTSampler runs on the GPU: device=%s" % self.device)
        g = _as_device_csr(g, self.device)
        if self.mode != "walk" and g.nnz == 0:
            raise ValueError("mode %r draws entries of the graph and it has none" % self.mode)
        self.graph = g
        self.num_nodes = n = g.n_rows
        self._workspace = SubgraphWorkspace(n, self.device)
        words = (n + 31) // 32
        self._bitmap = torch.zeros(words, dtype=torch.int32, device=self.device)
        self._prefix = torch.zeros(words, dtype=torch.int32, device=self.device)
        self.stream = torch.cuda.Stream(self.device)

    def sample(self, g=None, indices=None):
        """(nodes, subgraph) under a seed drawn from numpy's global generator; `indices` is ignored, as in DGL."""
        seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
        return self.sample_seeded(g, seed)

    def _node_set(self, seed, st):
        g, dev, n = self.graph, self.device, self.num_nodes
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        info = torch.empty(_INFO_WORDS, dtype=torch.int64, device=dev)
        csr = (g.rowptr.data_ptr(), _lib.ptr(g.col) if g.nnz else None)
        if self.mode == "walk":
            roots = torch.empty(self.budget, dtype=torch.int64, device=dev)
            _lib.launch("dgll_hip_sg_draw", dev, *csr, n, g.nnz, _MODES["walk"], self.budget, seed, None, None, roots.data_ptr(), info.data_ptr(),
                        stream=st)
            cols = self.length + 1
            walks = torch.empty((self.budget, cols), dtype=torch.int32, device=dev)
            winfo = torch.zeros(2, dtype=torch.int64, device=dev)
            _lib.launch("dgll_hip_random_walk", dev, *csr, n, roots.data_ptr(), self.budget, cols, 0, seed, 1.0, 1.0, _WALK_ATTEMPTS,
                        walks.data_ptr(), winfo.data_ptr(), stream=st)
            _lib.launch("dgll_hip_sg_walk_nodes", dev, walks.data_ptr(), self.budget * cols, n, self._bitmap.data_ptr(), self._prefix.data_ptr(),
                        info.data_ptr(), stream=st)
            both = torch.cat([info[:3], winfo]).cpu().tolist()          # one blocking read for both
            count, err = both[0], both[2] | (2 if both[4] & 2 else 0)
        else:
            _lib.launch("dgll_hip_sg_draw", dev, *csr, n, g.nnz, _MODES[self.mode], self.budget, seed, self._bitmap.data_ptr(),
                        self._prefix.data_ptr(), None, info.data_ptr(), stream=st)
            count, _, err = info.cpu().tolist()[:3]
        _raise_for(err, "SAINTSampler")
        nodes = torch.empty(count, dtype=torch.int64, device=dev)
        _lib.launch("dgll_hip_sg_compact", dev, n, self._bitmap.data_ptr(), self._prefix.data_ptr(), count, nodes.data_ptr(), stream=st)
        return nodes

    def sample_seeded(self, g, seed):
        """sample() under an explicit 64-bit seed: bit-identical output for the same (graph, seed)."""
        with self._lock:
            if self.graph is None:
                if g is None:
                    raise ValueError("SAINTSampler needs a graph: pass it to the constructor or to sample()")
                self._bind(g)
            with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
                nodes = self._node_set(seed, self.stream)
                sub = node_subgraph(self.graph, nodes, self.normalize, workspace=self._workspace)
                self.stream.synchronize()
        return nodes, sub
