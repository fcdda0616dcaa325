"""Node-wise neighbour sampler with DGL's block contract, on the device (dgll_amd/csrc/neighbor.hip).

The reference's two headline scripts (`GPU Accelerator/MQGCN.py:114`, `MQGraphSAGE.py:114`) build `NeighborSampler([4, 4])` and
iterate `(input_nodes, output_nodes, blocks)`: fan-out sampling WITHOUT replacement, every hop compacted into a message-flow-graph
block whose source nodes are unique, the destinations first.

    NeighborSampler(fanouts, g=None, replace=False, prob=None, norm="mean", device=None)

fanouts: DGL's order -- fanouts[i] belongs to layer i, the last entry is applied to the seeds first; -1 keeps every neighbour; a
fan-out is at most MAX_FANOUT (64: one kept position per lane of a wavefront).  replace=True is refused (out of scope).  g: a
CSRGraph of IN-neighbours (row v lists the sources of v) or a DGraph, converted once; it may also be passed to the first sample().

sample(g, seed_nodes) / sample_seeded(g, seed_nodes, seed) -> (input_nodes, output_nodes, blocks), blocks outermost first.  Each
block is a CSRGraph with int64 rowptr, int32 LOCAL column ids ascending within a row, n_rows = |dst|, n_cols = |src|:
blocks[i].n_rows == blocks[i + 1].n_cols, blocks[-1].n_rows == len(seed_nodes).  The source nodes of a block are [its destinations
in their order | the new nodes in ascending id order], so `input_nodes[:blocks[0].n_rows]` are blocks[0]'s destinations and
`x[:block.n_rows]` is a layer's self term.  norm="mean": fp32 values 1 / count per row (rows without neighbours have no entries);
norm=None: no values.  A destination of degree d keeps min(d, fanout) DISTINCT entries of its adjacency list, every subset equally
likely (Floyd's algorithm on Philox4x32-10 words; counter = (node, layer, call), key = seed: the draw of a node does not depend
on its batch).  Seed nodes must be unique and lie in [0, N): both are checked on the device and raise.

prob (DGL's argument of the same name): None -- the uniform draw above.  "weight" -- the bound graph's `val`; a tensor or array --
one weight per entry of the graph, in entry order; either is converted to fp32 and checked when the graph is bound (check_weights:
a wrong length, a negative weight, NaN or inf raise ValueError).  An entry of weight 0 is never sampled: a destination keeps
min(number of its positive-weight entries, fanout) distinct entries, every one of them under fanout = -1, and when it has more
than the fan-out the kept set is drawn successively without replacement in proportion to the weights (Plackett-Luce on the set;
the `fanout` smallest exponential race keys -log(u) / w, u from one Philox4x32-10 call per entry with counter =
(node, layer | 2^31, position in the row), key = seed -- again independent of the batch).  Zero weights are handled once, at bind
time: if there is any, `sampler.graph` is the FILTERED graph (zero-weight entries removed, order kept, `val` = the fp32 weights)
and every layer samples on it; otherwise it is the bound graph with the weights as `val`.  The blocks carry no edge weights: their
values are 1 / count as without prob.

Differences from DGL: the new nodes of a block are in ascending id order (DGL: first occurrence); the generator differs, so the
sampled ids are not DGL's.  Parallel edges of the graph are kept as they are (a block row may then repeat a column).

Seeding, streams: as the layer-wise samplers (sampling/layerwise.py) -- sample() draws one 64-bit seed from numpy's global
generator, sample_seeded takes it (use fast_sampler.batch_seed per batch; MiniBatchPipeline(sampler_threads=K) does); the kernels
run on a stream the sampler owns, sample() returns after it has finished, and a consumer on another stream calls
`layerwise.record_stream(blocks, input_nodes, stream)`.  One blocking device -> host read per layer (nnz and the number of new nodes).
"""
import threading

import numpy as np
import torch

from .. import _lib
from ..graph import CSRGraph
from .layerwise import _as_device_csr, record_stream  # noqa: F401  (record_stream: re-exported for consumers)

MAX_FANOUT = int(_lib.lib.dgll_hip_nb_max_fanout())
_INFO_WORDS = 8              # neighbor.hip: {nnz, new nodes, error bits, ...}
_ERRORS = {1: "a seed / destination id outside [0, N)", 2: "a column id of the graph outside [0, N)", 4: "a duplicate seed node",
           8: "an edge weight that is no positive finite number"}


def check_weights(prob, nnz):
    """prob as a flat fp32 tensor (on the device it came from) of one finite weight >= 0 per graph entry, or ValueError.  Needs no GPU."""
    w = prob if isinstance(prob, torch.Tensor) else torch.as_tensor(np.asarray(prob))
    w = w.detach().reshape(-1)
    if w.numel() != int(nnz):
        raise ValueError("prob needs one weight per entry of the graph: got %d weights for %d entries" % (w.numel(), int(nnz)))
    if w.dtype == torch.bool or w.is_complex():
        raise ValueError("prob must hold real numbers")
    w = w.to(torch.float32).contiguous()
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError("prob: every weight must be finite (as fp32) and >= 0")
    return w


def drop_zero_weights(rowptr, col, w):
    """(rowptr, col, w) without the entries of weight 0, order kept; the arguments themselves when there is none (torch, any device)."""
    keep = w > 0
    if bool(keep.all()):
        return rowptr, col, w
    below = torch.zeros(w.numel() + 1, dtype=torch.int64, device=w.device)
    below[1:] = torch.cumsum(keep, 0)
    return below[rowptr], col[keep].contiguous(), w[keep].contiguous()


class NeighborSampler:
    def __init__(self, fanouts, g=None, replace=False, prob=None, norm="mean", device=None):
        if replace:
            raise NotImplementedError("NeighborSampler samples without replacement only (replace=True is not supported)")
        fanouts = [int(f) for f in np.asarray(fanouts).reshape(-1)]
        if not fanouts or any(f != -1 and not 1 <= f <= MAX_FANOUT for f in fanouts):
            raise ValueError("fanouts must be a non-empty list of -1 (every neighbour) or integers in [1, %d]" % MAX_FANOUT)
        if norm not in ("mean", None):
            raise ValueError("norm must be 'mean' or None")
        if isinstance(prob, str) and prob != "weight":
            raise ValueError("prob must be None, 'weight' (the graph's values) or one weight per entry of the graph")
        self.fanouts, self.layers, self.norm, self.prob = fanouts, len(fanouts), norm, prob
        self._device_arg = device
        self.graph = None
        self._lock = threading.Lock()
        if g is not None:
            self._bind(g)

    def _bind(self, g):
        device = self._device_arg
        if device is None:
            if isinstance(g, CSRGraph) and g.is_cuda:
                device = g.device
            elif not torch.cuda.is_available():
                raise RuntimeError("NeighborSampler runs on the GPU and none is available: pass a graph on the device or device=")
            else:
                device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        g = _as_device_csr(g, self.device)
        if self.prob is not None:
            if isinstance(self.prob, str) and g.val is None:
                raise ValueError("prob='weight' needs a graph with values")
            w = check_weights(g.val if isinstance(self.prob, str) else self.prob, g.nnz).to(self.device)
            g = CSRGraph(*drop_zero_weights(g.rowptr, g.col, w), g.n_rows, g.n_cols, check=False)
        self.graph = g
        self.num_nodes = n = g.n_rows
        if not 0 < n < 2 ** 31:
            raise ValueError("the graph needs between 1 and 2^31 - 1 nodes")
        words = (n + 31) // 32
        z = lambda k: torch.zeros(k, dtype=torch.int32, device=self.device)      # noqa: E731
        # persistent per graph: epoch tags (never cleared) and the destinations' local ids; per layer: the bitmap of new nodes
        self._mark, self._local, self._bitmap, self._prefix = z(n), z(n), z(words), z(words)
        self._epoch = 0
        self.stream = torch.cuda.Stream(self.device)

    def sample(self, g, seed_nodes):
        """(input_nodes, output_nodes, blocks) under a seed drawn from numpy's global generator."""
        seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
        return self.sample_seeded(g, seed_nodes, seed)

    def _seed_tensor(self, seed_nodes):
        if isinstance(seed_nodes, torch.Tensor):
            b = seed_nodes.to(torch.int64)
        else:
            b = torch.as_tensor(np.asarray(seed_nodes, dtype=np.int64))
        return b.reshape(-1).to(self.device, non_blocking=False).contiguous()

    def _layer(self, rows, fanout, seed, layer, st):
        """One hop: (source nodes, block) of the destinations `rows`."""
        g, dev, n_dst = self.graph, self.device, int(rows.numel())
        rowptr = torch.zeros(n_dst + 1, dtype=torch.int64, device=dev)
        want_val = self.norm == "mean"
        if n_dst == 0:
            col = torch.empty(0, dtype=torch.int32, device=dev)
            val = torch.empty(0, dtype=torch.float32, device=dev) if want_val else None
            return rows, CSRGraph(rowptr, col, val, 0, 0, check=False)
        info = torch.empty(_INFO_WORDS, dtype=torch.int64, device=dev)
        weighted = self.prob is not None and fanout > 0        # fanout -1 keeps every entry of the (filtered) graph: nothing to weigh
        cap = n_dst * (fanout + 1 if weighted else fanout) if fanout > 0 else 0
        drawn = torch.empty(cap, dtype=torch.int32, device=dev) if cap else None
        self._epoch = epoch = self._epoch % 0xFFFFFFFF + 1
        if weighted:
            _lib.launch("dgll_hip_nb_sample_weighted", dev, g.rowptr.data_ptr(), g.col.data_ptr(), g.val.data_ptr(), self.num_nodes,
                        rows.data_ptr(), n_dst, fanout, int(seed) & 0xFFFFFFFFFFFFFFFF, layer, self._mark.data_ptr(), self._local.data_ptr(),
                        epoch, self._bitmap.data_ptr(), self._prefix.data_ptr(), _lib.ptr(drawn), cap, rowptr.data_ptr(), info.data_ptr(),
                        stream=st)
        else:
            _lib.launch("dgll_hip_nb_sample", dev, g.rowptr.data_ptr(), g.col.data_ptr(), self.num_nodes, rows.data_ptr(), n_dst, fanout,
                        int(seed) & 0xFFFFFFFFFFFFFFFF, layer, self._mark.data_ptr(), self._local.data_ptr(), epoch,
                        self._bitmap.data_ptr(), self._prefix.data_ptr(), _lib.ptr(drawn), cap, rowptr.data_ptr(), info.data_ptr(), stream=st)
        nnz, n_new, err = info.cpu().tolist()[:3]           # the one blocking read of the layer
        if err:
            raise ValueError("neighbour sampler: " + ", ".join(m for bit, m in _ERRORS.items() if err & bit))
        src = torch.empty(n_dst + n_new, dtype=torch.int64, device=dev)
        col = torch.empty(nnz, dtype=torch.int32, device=dev)
        loc = torch.empty(nnz, dtype=torch.int32, device=dev)
        val = torch.empty(nnz, dtype=torch.float32, device=dev) if want_val else None
        _lib.launch("dgll_hip_nb_block", dev, g.rowptr.data_ptr(), g.col.data_ptr(), self.num_nodes, rows.data_ptr(), n_dst, fanout,
                    self._mark.data_ptr(), self._local.data_ptr(), epoch, self._bitmap.data_ptr(), self._prefix.data_ptr(), _lib.ptr(drawn),
                    rowptr.data_ptr(), nnz, n_new, _lib.ptr(loc) if nnz else None, src.data_ptr(), _lib.ptr(col) if nnz else None,
                    _lib.ptr(val) if nnz else None, stream=st)
        return src, CSRGraph(rowptr, col, val, n_dst, n_dst + n_new, check=False)

    def sample_seeded(self, g, seed_nodes, seed, max_threads=1, last_hop_buffer=None, staging=None):
        """sample() under an explicit 64-bit seed: bit-identical output for the same (graph, seed nodes, seed).  max_threads,
        last_hop_buffer and staging are the host sampler's options (MiniBatchPipeline passes them to every sampler): unused here."""
        with self._lock:
            if self.graph is None:
                if g is None:
                    raise ValueError("NeighborSampler needs a graph: pass it to the constructor or to sample()")
                self._bind(g)
            with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
                st = self.stream
                rows = self._seed_tensor(seed_nodes)
                blocks = []
                for layer in range(self.layers - 1, -1, -1):
                    rows, blk = self._layer(rows, self.fanouts[layer], seed, layer, st)
                    blocks.append(blk)
                st.synchronize()
        blocks.reverse()
        return rows, seed_nodes, blocks
