"""Layer-wise importance samplers -- LADIES and FastGCN -- with the per-batch work on the device (dgll_amd/csrc/layerwise.hip).

The reference trains its GCNs on these samplers in 8 of the 10 `GPU Accelerator/MQ*.py` scripts and samples on the host with
scipy (a row slice of the normalised adjacency, `Q.multiply(Q).sum(0)` over all N columns, `np.random.choice(N, s, p)`).  Here
one layer is: column mass of the rows R (fixed-point integer atomics), a draw of s nodes without replacement in draw order
(exponential race keys + radix select), the weights, and the block L[R, S] * w (count, scan, fill) -- with ONE blocking
device -> host read per layer (s and the block's nnz, to size the outputs).

Classes (constructor arguments as in the reference):
    Ladies(fanouts, g, flat=False, HW_row_norm=False)            MQLadies.py:62-89 (LadiesWrs, LadiesFlatWrs: the same algorithm)
    FastGCNSampler(fanouts, g)                                    MQFastGCN.py:60-88
    FastGCNSamplerFlat(fanouts, g, HW_row_norm=False, flat=False, wrs=False)     MQFastGCNFlat.py:62-102
`g` is a CSRGraph of the raw adjacency (any device) or a DGraph (converted once with DGraph.to_csr).

sample(g, batch_nodes) -> (input_nodes, batch_nodes, blocks): blocks outermost first (the reference's `subgs.reverse()`), each a
CSRGraph with int64 rowptr, int32 local column ids ascending within a row, fp32 values, n_rows = |R|, n_cols = |S|, so
blocks[i].n_rows == blocks[i + 1].n_cols and blocks[-1].n_rows == len(batch_nodes); input_nodes are the global ids of the
outermost columns (device int64).  Features are not attached: fetch them (GraphCacheServer.fetch_data, MiniBatchPipeline).

Documented fixes (the reference's behaviour is not reproduced here):
  (a) The reference builds its block from `(indptr, indices, [])` (MQLadies.py:84) and so DROPS the weighted values it has just
      computed; the blocks here carry them -- the estimator the papers define.  `block.with_values(None)` is the unweighted form.
  (b) FastGCN sets `prev_nodes_list = subgs[-1].srcnodes()` (MQFastGCN.py:84, MQFastGCNFlat.py:97): LOCAL ids, so from layer 2 on
      the reference slices the wrong rows.  Here the next rows are the global ids of the sampled set.
  (c) n_cols is always |S|; DGL infers it from max(indices) + 1 and drops trailing columns without edges.
  `HW_row_norm` is accepted and ignored, as in the reference.

Seeding: every sample() draws one 64-bit seed from numpy's global generator, so `np.random.seed(s)` makes a run reproducible --
but the draws are NOT bit-equal to the reference's (a different generator: Philox4x32-10 keyed by (seed, layer), counter = node
id).  sample_seeded(g, batch_nodes, seed) takes the seed explicitly (use it with fast_sampler.batch_seed).  For a given seed the
output is bit-identical across calls, instances and processes (no float atomics; every reduction is integer or in a fixed order).

Streams: the kernels run on a stream the sampler owns, and sample() returns after that stream has finished.  The outputs are
allocated on that stream: a CONSUMER that uses or frees them on another stream waits on the sampler's stream (already done when
sample() returns) and calls `record_stream` on them -- `record_stream(blocks, input_nodes, stream)` below does it -- the rule
GraphCacheServer.fetch_data documents.
"""
import threading

import numpy as np
import torch

from .. import _lib
from .. import prep
from ..graph import CSRGraph

MAX_FANOUT = 4096            # selected sets are ranked and mapped inside one workgroup's bitmap
_INFO_WORDS = 8              # layerwise.hip: {candidates, s, columns, nnz, error bits, ...}
_ERRORS = {1: "a row id outside [0, N)", 2: "a column id outside [0, N)", 4: "more tied winners than the workspace holds",
           8: "a local column id >= 4096"}


def _shift_for(bound):
    """Fixed-point exponent for column masses that can reach `bound`: every mass (and its 64-bit sum) stays below 2^61."""
    bound = float(bound)
    if bound <= 0.0:
        return 60
    return int(max(0, min(60, 61 - int(np.ceil(np.log2(bound))))))


def record_stream(blocks, input_nodes, stream):
    """Tell the caching allocator that the outputs of one sample() are used on `stream` (call it on the consumer side)."""
    for blk in blocks:
        for t in (blk.rowptr, blk.col, blk.val):
            if t is not None:
                t.record_stream(stream)
    if isinstance(input_nodes, torch.Tensor) and input_nodes.is_cuda:
        input_nodes.record_stream(stream)


class Workspace:
    """Persistent per-graph device buffers (length N) -- epoch-tagged markers that are never cleared, the fixed-point column mass,
    the candidate list and the select's scratch -- and the epoch counter.  One sample() at a time uses it."""

    def __init__(self, n, device, max_fanout=MAX_FANOUT):
        z = lambda k, dt: torch.zeros(k, dtype=dt, device=device)      # noqa: E731
        self.n, self.device = int(n), device
        self.marker, self.mark, self.local = z(n, torch.int32), z(n, torch.int32), z(n, torch.int32)
        self.mass, self.cand, self.keys = z(n, torch.int64), z(n, torch.int32), z(n, torch.int64)
        self.ctrl = z(int(_lib.lib.dgll_hip_lw_ctrl_words()), torch.int64)
        self.win_cap = int(max_fanout) + 1024
        self.win_key, self.win_id = z(self.win_cap, torch.int64), z(self.win_cap, torch.int32)
        self.n_reps = z(1, torch.int64)
        self.epoch = 0

    def next_epoch(self):
        self.epoch = self.epoch % 0xFFFFFFFF + 1
        return self.epoch


class ColumnMass:
    """Result of column_mass: the candidate columns (ws.cand[:count], count at `count_ptr` on the device), their fixed-point masses
    (ws.mass), the totals and the fixed-point exponent.  p = q / sum q with q = mass (or sqrt(mass) when flat)."""

    def __init__(self, ws, count, shift, flat, totals):
        self.ws, self.count, self.shift, self.flat, self.totals = ws, count, int(shift), bool(flat), totals

    def n_candidates(self):
        return int(self.count.item())

    def p_of(self, ids, count=None, stream=None):
        """fp64 p of int64 device ids (the first *count of them when count is a device scalar)."""
        out = torch.empty(ids.numel(), dtype=torch.float64, device=ids.device)
        _lib.launch("dgll_hip_lw_column_p", ids.device, ids.data_ptr(), _lib.ptr(count), ids.numel(), self.ws.mass.data_ptr(), self.shift,
                    int(self.flat), self.totals.data_ptr(), out.data_ptr(), stream=stream)
        return out

    def candidates(self):
        return self.ws.cand[:self.n_candidates()].to(torch.int64)

    def p_dense(self):
        """fp64 [N] with p at the candidates and 0 elsewhere (reads the candidate count)."""
        cand = self.candidates()
        p = torch.zeros(self.ws.n, dtype=torch.float64, device=cand.device)
        if cand.numel():
            p[cand] = self.p_of(cand)
        return p


# ---- stages -------------------------------------------------------------------------------------------------------------------
def column_mass(L, rows=None, flat=False, ws=None, info=None, shift=None, stream=None):
    """Per-column mass sum_{i in rows} L_ij^2 of a device CSRGraph (rows: int64 device ids, None = all rows), compacted to the touched
    columns.  No host synchronisation."""
    if ws is None:
        ws = Workspace(L.n_cols, L.device)
    if info is None:
        info = torch.zeros(_INFO_WORDS, dtype=torch.int64, device=L.device)
    n_rows = L.n_rows if rows is None else int(rows.numel())
    if shift is None:
        vmax = 1.0 if L.val is None or L.nnz == 0 else float(L.val.abs().max()) ** 2
        shift = _shift_for(n_rows * vmax)
    totals = torch.empty(2, dtype=torch.int64, device=L.device)
    seg = None if rows is None else torch.empty(n_rows + 1, dtype=torch.int64, device=L.device)
    _lib.launch("dgll_hip_lw_column_mass", L.device, L.rowptr.data_ptr(), L.col.data_ptr(), _lib.ptr(L.val), _lib.ptr(rows), n_rows, ws.n,
                ws.marker.data_ptr(), ws.next_epoch(), ws.mass.data_ptr(), shift, int(flat), ws.cand.data_ptr(), info.data_ptr(),
                totals.data_ptr(), _lib.ptr(seg), stream=stream)
    return ColumnMass(ws, info[0:1], shift, flat, totals)


def mass_from_p(p, ws=None):
    """ColumnMass of given probabilities (fp64 [N] tensor on the device; zeros are not candidates): for drawing from an explicit p."""
    p = p.to(torch.float64)
    ws = Workspace(p.numel(), p.device) if ws is None else ws
    cand = torch.nonzero(p > 0).flatten()
    ws.cand[:cand.numel()] = cand.to(torch.int32)
    ws.mass.copy_(torch.round(p / p.max() * 2.0 ** 40).to(torch.int64))      # the sum below stays exact up to N = 2^22
    info = torch.tensor([cand.numel()], dtype=torch.int64, device=p.device)
    total = int(ws.mass[cand].sum()) if cand.numel() else 0
    totals = torch.tensor([total >> 32, total & 0xFFFFFFFF], dtype=torch.int64, device=p.device)
    return ColumnMass(ws, info, 40, False, totals)


def select(mass, fanout, seed, layer=0, info=None, stream=None):
    """Draw s = min(#{p > 0}, fanout) candidates without replacement with probability p, in draw order: int64 device tensor
    [fanout], valid up to s (info[1] on the device).  No host synchronisation."""
    ws = mass.ws
    fanout = int(fanout)
    if not 1 <= fanout <= ws.win_cap - 1024:
        raise ValueError("fanout must be in [1, %d]" % (ws.win_cap - 1024))
    if info is None:
        info = torch.zeros(_INFO_WORDS, dtype=torch.int64, device=ws.device)
    out = torch.empty(fanout, dtype=torch.int64, device=ws.device)
    _lib.launch("dgll_hip_lw_select", ws.device, ws.cand.data_ptr(), mass.count.data_ptr(), ws.n, ws.mass.data_ptr(), mass.shift,
                int(mass.flat), int(seed) & 0xFFFFFFFFFFFFFFFF, int(layer), fanout, ws.keys.data_ptr(), ws.ctrl.data_ptr(),
                ws.win_key.data_ptr(), ws.win_id.data_ptr(), ws.win_cap, out.data_ptr(), info.data_ptr(), stream=stream)
    return out, info


def union_sorted(ws, a, a_count, b, info, stream=None):
    """sorted unique(a[:*a_count] u b) on the device (FastGCN's np.unique(concatenate(S, batch))); length into info[2]."""
    cap = a.numel() + b.numel()
    reps = torch.empty(cap, dtype=torch.int64, device=ws.device)
    out = torch.empty(cap, dtype=torch.int64, device=ws.device)
    _lib.launch("dgll_hip_lw_union_sorted", ws.device, a.data_ptr(), a_count.data_ptr(), a.numel(), b.data_ptr(), b.numel(), ws.n,
                ws.marker.data_ptr(), ws.next_epoch(), reps.data_ptr(), ws.n_reps.data_ptr(), out.data_ptr(), info.data_ptr(),
                stream=stream)
    return out


def wrs_weights(p, n_total, count=None, stream=None):
    """The reference's estWRS_weights (utils.py:199-213) for probabilities p in draw order, n = n_total (= N, as len(p) there): fp64."""
    return _weights(p, count, None, 0, n_total, 0, stream)


def inverse_weights(p, s, count=None, stream=None):
    """1 / (p_j * s), fp64; s an int or a device int64 scalar."""
    if isinstance(s, torch.Tensor):
        return _weights(p, count, s, 0, 1, 1, stream)
    return _weights(p, count, None, int(s), 1, 1, stream)


def _weights(p, count, snum_dev, snum, n_total, mode, stream):
    p = p.to(torch.float64).contiguous()
    w = torch.empty_like(p)
    _lib.launch("dgll_hip_lw_weights", p.device, p.data_ptr(), _lib.ptr(count), p.numel(), _lib.ptr(snum_dev), snum, int(n_total), mode, w.data_ptr(),
                stream=stream)
    return w


def extract_block(L, rows, cols, weights, ws=None, info=None, count=None, sorted_cols=False, stream=None):
    """CSRGraph L[rows, cols] * weights[local]: n_rows = len(rows), n_cols = number of cols, int32 local ids ascending within a row.
    cols: int64 device ids (the first *count of them when count is a device scalar), distinct; sorted_cols: they ascend (otherwise
    at most 4096).  One blocking read (the column count and the nnz)."""
    if ws is None:
        ws = Workspace(L.n_cols, L.device)
    if info is None:
        info = torch.zeros(_INFO_WORDS, dtype=torch.int64, device=L.device)
    if count is None:
        info[2] = cols.numel()
        count = info[2:3]
    n_rows = int(rows.numel())
    if not sorted_cols and cols.numel() > MAX_FANOUT:
        raise ValueError("unsorted column sets are limited to %d columns" % MAX_FANOUT)
    rowptr = torch.empty(n_rows + 1, dtype=torch.int64, device=L.device)
    seg = bitmap = below = None
    if not sorted_cols:           # flat passes over the entries (hub rows): per-row bitmaps of the kept local ids
        seg = torch.empty(n_rows + 1, dtype=torch.int64, device=L.device)
        bitmap = torch.empty(n_rows * (MAX_FANOUT // 32), dtype=torch.int32, device=L.device)
        below = torch.empty(n_rows * (MAX_FANOUT // 32), dtype=torch.int32, device=L.device)
    epoch = ws.next_epoch()
    _lib.launch("dgll_hip_lw_block_count", L.device, L.rowptr.data_ptr(), L.col.data_ptr(), rows.data_ptr(), n_rows, ws.n, cols.data_ptr(),
                count.data_ptr(), cols.numel(), ws.mark.data_ptr(), ws.local.data_ptr(), epoch, int(sorted_cols), _lib.ptr(seg), _lib.ptr(bitmap),
                _lib.ptr(below), rowptr.data_ptr(), info.data_ptr(), stream=stream)
    h = info.cpu().tolist()           # the one blocking read of the layer
    if h[4]:
        raise RuntimeError("layer-wise sampler: " + ", ".join(m for bit, m in _ERRORS.items() if h[4] & bit))
    m = int(count.item()) if count.data_ptr() != info[2:3].data_ptr() else h[2]
    nnz = h[3]
    col = torch.empty(nnz, dtype=torch.int32, device=L.device)
    val = torch.empty(nnz, dtype=torch.float32, device=L.device)
    w = weights.to(torch.float64).contiguous()
    _lib.launch("dgll_hip_lw_block_fill", L.device, L.rowptr.data_ptr(), L.col.data_ptr(), _lib.ptr(L.val), rows.data_ptr(), n_rows, ws.n,
                ws.mark.data_ptr(), ws.local.data_ptr(), epoch, w.data_ptr(), int(sorted_cols), m, _lib.ptr(seg), _lib.ptr(bitmap), _lib.ptr(below),
                rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), info.data_ptr(), stream=stream)
    return CSRGraph(rowptr, col, val, n_rows, m, check=False), m, h


# ---- samplers -----------------------------------------------------------------------------------------------------------------
def _as_device_csr(g, device):
    from ..data.dgraph import DGraph

    if isinstance(g, DGraph):
        g = g.to_csr()
    if not isinstance(g, CSRGraph):
        raise TypeError("g must be a CSRGraph of the raw adjacency or a DGraph, got %r" % type(g))
    if g.n_rows != g.n_cols:
        raise ValueError("the adjacency must be square")
    return g.to(device)


class LayerwiseSampler:
    """The core of every layer-wise sampler.
    norm: "row" (D^-1 (A + I), LADIES) or "sym" (D^-1/2 (A + I)^T D^-1/2, FastGCN); per_batch: p from the current rows each layer
    (LADIES) or once over all rows (FastGCN); flat: sqrt of the column mass; union: the next set is sorted unique(S u batch)
    (FastGCN); weights: "wrs" (estWRS_weights) or "inverse" (1 / (p s))."""

    def __init__(self, fanouts, g, norm="row", per_batch=True, flat=False, union=False, weights="wrs", device=None):
        fanouts = [int(f) for f in np.asarray(fanouts).reshape(-1)]
        if not fanouts or any(f < 1 or f > MAX_FANOUT for f in fanouts):
            raise ValueError("fanouts must be a non-empty list of integers in [1, %d]" % MAX_FANOUT)
        if norm not in ("row", "sym") or weights not in ("wrs", "inverse"):
            raise ValueError("norm must be 'row' or 'sym', weights 'wrs' or 'inverse'")
        if union and weights != "inverse":
            raise ValueError("the union with the batch goes with the 1 / (p s) weights (MQFastGCN.py:78-80)")
        if device is None:
            device = g.device if isinstance(g, CSRGraph) and g.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.fanouts, self.layers = fanouts, len(fanouts)
        self.norm, self.per_batch, self.flat, self.union, self.weights = norm, bool(per_batch), bool(flat), bool(union), weights
        raw = _as_device_csr(g, self.device)
        self.num_nodes = n = raw.n_rows
        row, col = raw.row_index(), raw.col.to(torch.int64)
        if norm == "row":
            self.lap = prep.normalized_adjacency(row, col, n, val=raw.val, symmetric=False)
        else:
            self.lap = prep.sym_normalized_transpose(row, col, n, val=raw.val)
        self._vmax2 = float(self.lap.val.abs().max()) ** 2 if self.lap.nnz else 1.0
        self.stream = torch.cuda.Stream(self.device)
        self.ws = Workspace(n, self.device)
        self._lock = threading.Lock()
        self.global_mass = None
        if not self.per_batch:        # FastGCN: p over all rows, once (the same kernel with every row)
            # entries of a column of L <= entries of a row of A + I ("sym" is the transpose): bounds every column's mass
            colcount = (int(raw.degrees().max()) if raw.nnz else 0) + 1
            with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
                info = torch.zeros(_INFO_WORDS, dtype=torch.int64, device=self.device)
                self.global_mass = column_mass(self.lap, None, flat=self.flat, ws=self.ws, info=info,
                                               shift=_shift_for(colcount * self._vmax2), stream=self.stream)
                self._global_count = info[0:1].clone()
                self.global_mass.count = self._global_count
            self.stream.synchronize()

    def p_global(self):
        """fp64 [N] p of the FastGCN variants."""
        if self.global_mass is None:
            raise RuntimeError("LADIES samplers compute p per layer (column_mass)")
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            p = self.global_mass.p_dense()
        self.stream.synchronize()
        return p

    def sample(self, g, batch_nodes):
        """(input_nodes, batch_nodes, blocks) under a seed drawn from numpy's global generator."""
        seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
        return self.sample_seeded(g, batch_nodes, seed)

    def _batch_tensor(self, batch_nodes):
        if isinstance(batch_nodes, torch.Tensor):
            b = batch_nodes.to(torch.int64)
        else:
            b = torch.as_tensor(np.asarray(batch_nodes, dtype=np.int64))
        b = b.reshape(-1)
        if b.numel() == 0:
            raise ValueError("empty batch")
        if not b.is_cuda:
            lo, hi = int(b.min()), int(b.max())
            if lo < 0 or hi >= self.num_nodes:
                raise ValueError("batch node ids must lie in [0, %d)" % self.num_nodes)
        return b.to(self.device, non_blocking=False).contiguous()

    def sample_seeded(self, g, batch_nodes, seed):
        """sample() under an explicit 64-bit seed: bit-identical output for the same (graph, batch, seed)."""
        with self._lock, torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            st = self.stream
            batch = self._batch_tensor(batch_nodes)
            rows, blocks, nodes = batch, [], []
            for l, fanout in enumerate(self.fanouts):
                info = torch.zeros(_INFO_WORDS, dtype=torch.int64, device=self.device)
                if self.per_batch:
                    mass = column_mass(self.lap, rows, flat=self.flat, ws=self.ws, info=info,
                                       shift=_shift_for(rows.numel() * self._vmax2), stream=st)
                else:
                    mass = self.global_mass
                drawn, _ = select(mass, fanout, seed, l, info=info, stream=st)
                s_dev = info[1:2]
                if self.union:
                    cols = union_sorted(self.ws, drawn, s_dev, batch, info, stream=st)
                else:
                    cols = drawn
                m_dev = info[2:3]
                p = mass.p_of(cols, count=m_dev, stream=st)
                if self.weights == "wrs":
                    w = _weights(p, m_dev, None, 0, self.num_nodes, 0, st)
                else:
                    w = _weights(p, m_dev, s_dev, 0, 1, 1, st)
                blk, m, _ = extract_block(self.lap, rows, cols, w, ws=self.ws, info=info, count=m_dev, sorted_cols=self.union, stream=st)
                blocks.append(blk)
                rows = cols[:m]
                nodes.append(rows)
            st.synchronize()
        self.last_nodes = nodes           # global ids of every layer's columns, innermost first (for inspection and tests)
        blocks.reverse()
        return rows, batch_nodes, blocks


class Ladies(LayerwiseSampler):
    """MQLadies.py:62-89: p_j = sum_{i in R} L_ij^2 (sqrt with flat), L = D^-1 (A + I); estWRS_weights; the next rows are S."""

    def __init__(self, fanouts, g, flat=False, HW_row_norm=False):
        super().__init__(fanouts, g, norm="row", per_batch=True, flat=flat, union=False, weights="wrs")
        self.HW_row_norm = HW_row_norm      # accepted and ignored, as in the reference


class LadiesWrs(Ladies):
    """MQLadiesWrs.py:62-89: the same algorithm as Ladies."""


class LadiesFlatWrs(Ladies):
    """MQLadiesFlatWrs.py:63-90: the same algorithm as Ladies (flat is an argument)."""


class FastGCNSampler(LayerwiseSampler):
    """MQFastGCN.py:60-88: p = column sums of L o L over all rows, L = D^-1/2 (A + I)^T D^-1/2; per layer s draws from all N, the
    columns are sorted unique(S u batch), weights 1 / (p s); the next rows are the GLOBAL ids of those columns (fix (b))."""

    def __init__(self, fanouts, g):
        super().__init__(fanouts, g, norm="sym", per_batch=False, flat=False, union=True, weights="inverse")


class FastGCNSamplerFlat(LayerwiseSampler):
    """MQFastGCNFlat.py:62-102: FastGCN's p (sqrt with flat), no union with the batch, estWRS_weights with wrs else 1 / (p s)."""

    def __init__(self, fanouts, g, HW_row_norm=False, flat=False, wrs=False):
        super().__init__(fanouts, g, norm="sym", per_batch=False, flat=flat, union=False, weights="wrs" if wrs else "inverse")
        self.HW_row_norm, self.wrs = HW_row_norm, wrs
