"""Edge-seeded sampling for link prediction, on the device (dgll_amd/csrc/edge_pred.hip) -- DGL's
`as_edge_prediction_sampler(NeighborSampler(...), negative_sampler=Uniform(k) / GlobalUniform(k), exclude=...)`.

    EdgePredictionSampler(block_sampler, negatives=1, filter_existing=False, exclude=None, max_attempts=16)
        .sample(g, edge_ids) / .sample_seeded(g, edge_ids, seed) -> (input_nodes, batch, blocks)

block_sampler: a NeighborSampler; its graph (bound already, or `g` of the first sample()) is the CSR of IN-neighbours: entry e of row
v is the edge col[e] -> v, and the EDGE ID of that edge is the entry index e in [0, nnz).  (A NeighborSampler with prob= and
zero weights samples on its filtered graph, `block_sampler.graph`: the edge ids are that graph's entries.)  edge_ids: int64[B],
duplicates allowed.

Pairs.  Positive i is (u, v) = (col[e], row of e).  Its K = `negatives` negatives are (u, c_k), c_k uniform over all N nodes:
c = mulhi32(word 0 of Philox4x32-10(counter = (e lo, e hi, k | 2^30, attempt), key = seed), N).  A negative depends on (seed, e, k)
only, never on the batch, and the counter domain is apart from the neighbour sampler's, so ONE seed drives both.
filter_existing=False is DGL's `Uniform`: attempt 0 is taken (it may be a real edge, or u itself).  filter_existing=True is DGL's
`GlobalUniform`: a candidate c with an edge u -> c is rejected (binary search of u in row c: the columns of every row must ascend,
checked once when the graph is bound, ValueError otherwise); after `max_attempts` rejections the last candidate is kept and counted
in `batch.capped`.

batch: a PairBatch.  output_nodes int64[M]: the distinct endpoints of all B * (1 + K) pairs in ascending id order -- the seed nodes of
the block sampler, unique by construction.  pairs int32[B * (1 + K), 2]: (local src, local dst) into output_nodes; rows 0 .. B-1 are
the positives in batch order, row B + i * K + k is negative k of positive i.  labels(): fp32 ones then zeros.

blocks: `block_sampler.sample_seeded(None, output_nodes, seed)` of the unmodified NeighborSampler, then the exclusion:
exclude=None      as sampled.
exclude="self"    every block entry a -> b (global ids) with (a, b) a positive pair of the batch is removed: the model cannot read
                  the edge it is asked about off its own input.
exclude="reverse" also entries with (b, a) a positive pair.
The exclusion is by endpoint pair, so parallel entries all go; negatives are never excluded; kept entries keep their order; with
norm="mean" the values become 1 / kept of the row.  A block's n_rows, n_cols and source list do not change: a source that lost all
its edges stays (as a node nobody reads), exactly as DGL samples first and filters afterwards -- the fan-out is NOT refilled.

Seeding, streams, locking: as NeighborSampler.  sample() draws one 64-bit seed from numpy's global generator; the kernels run on
the block sampler's stream and sample() returns after it has finished; a consumer on another stream calls
`batch.record_stream(stream)` and `layerwise.record_stream(blocks, input_nodes, stream)`.  Blocking device -> host reads: one
between the draw and the compaction (M, capped, error bits), the block sampler's one per layer, and one for all blocks' kept counts
when exclude is set.
"""
import threading

import numpy as np
import torch

from .. import _lib
from ..graph import CSRGraph
from .layerwise import record_stream  # noqa: F401  (re-exported for consumers)
from .neighbor import NeighborSampler

_INFO_WORDS = 8              # edge_pred.hip: {distinct endpoints, capped negatives, error bits, ...}
_ERRORS = {1: "an edge id outside [0, nnz)", 2: "a column id of the graph outside [0, N)"}
_EXCLUDE = (None, "self", "reverse")


def incidence_of(pairs, n_nodes):
    """(rowptr int64[n_nodes + 1], pair int32[2P], other int32[2P]) of local pairs int32[P, 2] on their device: row i lists (pair p,
    other endpoint) of every pair slot that holds i, ascending by (p, slot) -- slot 0: i is the src; a pair (i, i) gives two entries.
    One sort of the distinct keys node * 2P + (2p + slot): no order depends on an atomic."""
    flat = pairs.reshape(-1).to(torch.int64)
    n2 = flat.numel()
    if n2 == 0:
        z = torch.zeros(0, dtype=torch.int32, device=pairs.device)
        return torch.zeros(n_nodes + 1, dtype=torch.int64, device=pairs.device), z, z
    slot = torch.arange(n2, dtype=torch.int64, device=pairs.device)
    key, _ = torch.sort(flat * n2 + slot)
    node = torch.div(key, n2, rounding_mode="floor")
    j = key - node * n2
    rowptr = torch.searchsorted(node, torch.arange(n_nodes + 1, dtype=torch.int64, device=pairs.device))
    return rowptr, torch.div(j, 2, rounding_mode="floor").to(torch.int32), flat[j ^ 1].to(torch.int32)


class PairBatch:
    """The pairs of one edge batch: output_nodes int64[M], pairs int32[n_pos + n_neg, 2] local (src, dst), positives first."""

    def __init__(self, output_nodes, pairs, n_pos, n_neg, capped=0):
        self.output_nodes, self.pairs, self.n_pos, self.n_neg, self.capped = output_nodes, pairs, int(n_pos), int(n_neg), int(capped)
        self._incidence = None

    def __len__(self):
        return self.n_pos + self.n_neg

    def labels(self):
        """fp32 [n_pos + n_neg]: ones for the positives, then zeros."""
        y = torch.zeros(len(self), dtype=torch.float32, device=self.pairs.device)
        y[:self.n_pos] = 1.0
        return y

    def incidence(self):
        """incidence_of(pairs, M), built on first use (ops.pair_dot's backward gathers over it)."""
        if self._incidence is None:
            self._incidence = incidence_of(self.pairs, int(self.output_nodes.numel()))
        return self._incidence

    def record_stream(self, stream):
        """Tell the caching allocator that the batch is used on `stream` (call it on the consumer side)."""
        for t in (self.output_nodes, self.pairs) + (self._incidence or ()):
            if t.is_cuda:
                t.record_stream(stream)


def check_sorted_rows(g):
    """ValueError unless the columns of every row of g ascend (parallel entries allowed)."""
    if g.nnz < 2:
        return
    inside = torch.ones(g.nnz, dtype=torch.bool, device=g.device)
    starts = g.rowptr[1:-1]
    inside[starts[starts < g.nnz]] = False                  # the first entry of a row is compared with nothing
    if bool(((g.col[1:] < g.col[:-1]) & inside[1:]).any()):
        raise ValueError("filter_existing=True needs the columns of every row in ascending order (the existence test is a binary search)")


class EdgePredictionSampler:
    def __init__(self, block_sampler, negatives=1, filter_existing=False, exclude=None, max_attempts=16):
        if not isinstance(block_sampler, NeighborSampler):
            raise TypeError("block_sampler must be a NeighborSampler, got %r" % type(block_sampler))
        if int(negatives) != negatives or negatives < 0:
            raise ValueError("negatives must be an integer >= 0")
        if exclude not in _EXCLUDE:
            raise ValueError("exclude must be None, 'self' or 'reverse'")
        if int(max_attempts) != max_attempts or max_attempts < 1:
            raise ValueError("max_attempts must be an integer >= 1")
        self.block_sampler, self.negatives, self.filter_existing = block_sampler, int(negatives), bool(filter_existing)
        self.exclude, self.max_attempts = exclude, int(max_attempts)
        self.graph = None
        self._lock = threading.Lock()
        if block_sampler.graph is not None:
            self._bind(None)

    def _bind(self, g):
        bs = self.block_sampler
        with bs._lock:
            if bs.graph is None:
                if g is None:
                    raise ValueError("EdgePredictionSampler needs a graph: bind the block sampler or pass it to sample()")
                bs._bind(g)                     # RuntimeError without a GPU
        g = bs.graph
        if self.filter_existing:
            check_sorted_rows(g)
        self.graph, self.device, self.num_nodes, self.stream = g, bs.device, bs.num_nodes, bs.stream
        words = (self.num_nodes + 31) // 32
        z = lambda k: torch.zeros(k, dtype=torch.int32, device=self.device)      # noqa: E731
        # persistent per graph: epoch tags (never cleared); per call: the bitmap of endpoints and its popcount prefix
        self._mark, self._bitmap, self._prefix = z(self.num_nodes), z(words), z(words)
        self._epoch = 0

    def sample(self, g, edge_ids):
        """(input_nodes, batch, blocks) under a seed drawn from numpy's global generator."""
        seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
        return self.sample_seeded(g, edge_ids, seed)

    def _pairs(self, eids, seed, st):
        """(PairBatch, global pairs) of the edge ids `eids` (device int64)."""
        dev, g, b, k = self.device, self.graph, int(eids.numel()), self.negatives
        n_pairs = b * (1 + k)
        info = torch.empty(_INFO_WORDS, dtype=torch.int64, device=dev)
        gpairs = torch.empty((n_pairs, 2), dtype=torch.int32, device=dev)
        self._epoch = epoch = self._epoch % 0xFFFFFFFF + 1
        _lib.launch("dgll_hip_ep_draw", dev, g.rowptr.data_ptr(), g.col.data_ptr(), self.num_nodes, g.nnz, eids.data_ptr(), b, k,
                    int(self.filter_existing), self.max_attempts, int(seed) & 0xFFFFFFFFFFFFFFFF, self._mark.data_ptr(), epoch,
                    self._bitmap.data_ptr(), self._prefix.data_ptr(), gpairs.data_ptr(), n_pairs, info.data_ptr(), stream=st)
        m, capped, err = info.cpu().tolist()[:3]            # the one blocking read between the two calls
        if err:
            raise ValueError("edge prediction sampler: " + ", ".join(msg for bit, msg in _ERRORS.items() if err & bit))
        out = torch.empty(m, dtype=torch.int64, device=dev)
        pairs = torch.empty((n_pairs, 2), dtype=torch.int32, device=dev)
        _lib.launch("dgll_hip_ep_compact", dev, self.num_nodes, self._bitmap.data_ptr(), self._prefix.data_ptr(), m, gpairs.data_ptr(),
                    n_pairs, out.data_ptr(), pairs.data_ptr(), stream=st)
        return PairBatch(out, pairs, b, b * k, capped), gpairs

    def _exclude(self, blocks, input_nodes, gpairs, n_pos, st):
        """The blocks without the positive pairs of the batch (and their reverses)."""
        dev, n = self.device, self.num_nodes
        src, dst = gpairs[:n_pos, 0].to(torch.int64), gpairs[:n_pos, 1].to(torch.int64)
        keys = dst * n + src
        if self.exclude == "reverse":
            keys = torch.cat([keys, src * n + dst])
        keys, _ = torch.sort(keys)
        work = [blk for blk in blocks if blk.nnz > 0]
        if not work:
            return blocks
        infos = torch.empty((len(work), _INFO_WORDS), dtype=torch.int64, device=dev)
        rowptrs = []
        for i, blk in enumerate(work):
            rp = torch.empty(blk.n_rows + 1, dtype=torch.int64, device=dev)
            _lib.launch("dgll_hip_ep_exclude_count", dev, blk.rowptr.data_ptr(), blk.col.data_ptr(), blk.n_rows, blk.nnz,
                        input_nodes.data_ptr(), blk.n_cols, n, keys.data_ptr(), keys.numel(), rp.data_ptr(), infos[i].data_ptr(), stream=st)
            rowptrs.append(rp)
        kept = infos[:, 0].cpu().tolist()                   # one blocking read for all blocks
        done = {}
        for blk, rp, nnz in zip(work, rowptrs, kept):
            col = torch.empty(nnz, dtype=torch.int32, device=dev)
            val = torch.empty(nnz, dtype=torch.float32, device=dev) if blk.val is not None else None
            _lib.launch("dgll_hip_ep_exclude_fill", dev, blk.rowptr.data_ptr(), blk.col.data_ptr(), blk.n_rows, blk.nnz,
                        input_nodes.data_ptr(), blk.n_cols, n, keys.data_ptr(), keys.numel(), rp.data_ptr(), nnz,
                        _lib.ptr(col) if nnz else None, _lib.ptr(val) if nnz else None, stream=st)
            done[id(blk)] = CSRGraph(rp, col, val, blk.n_rows, blk.n_cols, check=False)
        return [done.get(id(blk), blk) for blk in blocks]

    def sample_seeded(self, g, edge_ids, seed):
        """sample() under an explicit 64-bit seed: bit-identical output for the same (graph, edge ids, seed)."""
        with self._lock:
            if self.graph is None:
                self._bind(g)
            dev, st = self.device, self.stream
            if isinstance(edge_ids, torch.Tensor) and edge_ids.is_cuda:
                st.wait_stream(torch.cuda.current_stream(edge_ids.device))      # ids still being written by the caller's stream
            with torch.cuda.device(dev), torch.cuda.stream(st):
                if isinstance(edge_ids, torch.Tensor):
                    eids = edge_ids.to(torch.int64)
                else:
                    eids = torch.as_tensor(np.asarray(edge_ids, dtype=np.int64))
                eids = eids.reshape(-1).to(dev).contiguous()
                if eids.numel() == 0:
                    batch = PairBatch(torch.empty(0, dtype=torch.int64, device=dev), torch.empty((0, 2), dtype=torch.int32, device=dev), 0, 0)
                    gpairs = None
                else:
                    batch, gpairs = self._pairs(eids, seed, st)
            # the block sampler takes its own lock and runs on the same stream, behind the compaction
            input_nodes, _, blocks = self.block_sampler.sample_seeded(None, batch.output_nodes, seed)
            if self.exclude is not None and gpairs is not None:
                with torch.cuda.device(dev), torch.cuda.stream(st):
                    blocks = self._exclude(blocks, input_nodes, gpairs, batch.n_pos, st)
                    st.synchronize()
        return input_nodes, batch, blocks
