"""Multi-GPU execution of the aggregation path: 1-D row partition + halo feature exchange + RaCoM gradient sharing.

One process per GPU (`torch.distributed`, backend "nccl" = RCCL over xGMI on ROCm; "gloo" on CPU for the tests).
The reference has no graph-partition parallelism at all ("Halo / remote-feature exchange:
not present anywhere"); what it does have is data-parallel DDP plus the RaCoM gradient queue
(/root/reference/dgll/GPU Accelerator/MQGCN.py:55-79, buffer_queues.py:74-110, README.md:27-37).  This module
supplies the partitioned full-graph path BASELINE.json's configs 3 and 5 name:

  * `partition_contiguous`: every rank owns a contiguous block of destination rows of A, their CSR rows and their
    feature rows.  The rank's edges are split by COLUMN into two CSRs over the same rows: `local` (neighbours the rank
    owns) and `halo` (remote neighbours, relabelled in owner-rank order so a received message is already in place).
    (Splitting rows into interior/boundary instead gives nothing to overlap: at average degree 45 and a 9 % edge cut
    98 % of the rows have at least one remote neighbour.)
  * `DistAggregate`: one autograd node per layer.  forward = pack send rows -> grouped point-to-point send/recv
    (xGMI is point-to-point: all peers are driven concurrently, not a ring) on a communication stream, overlapped
    with the SpMM over the `local` edges (~90 % of the work); then the SpMM over the `halo` edges accumulates into
    the same rows and applies the mean scale.  backward = the transposed exchange: halo gradients are produced first,
    travel while the local transposed SpMM runs, and are reduced at their owners in a fixed order -- no atomics.
  * `RaCoM`: all parameter gradients flattened into ONE bucket, all-reduced on a dedicated stream, averaged
    (MQGCN.py:63-64: sum / world_size), and applied when ready; `sync_every` = 1 reproduces DDP exactly.
"""
import os
import sys
import threading
import time

import torch
import torch.distributed as dist

from . import ops
from .graph import CSRGraph
from .optim import grad_slot_of
from .ranges import rng


class Partition:
    """This rank's share of a row-partitioned graph (all tensors on one device)."""

    def __init__(self):
        self.rank = self.world = 0
        self.own_begin = self.own_end = 0
        self.n_own = self.n_halo = 0
        self.local = None          # CSRGraph [n_own, n_own]   edges whose source row this rank owns
        self.halo = None           # CSRGraph [n_own, n_halo]  edges whose source row lives on another rank
        self.inv_deg = None        # fp32 [n_own] 1 / full degree (mean aggregation over both halves)
        self.send_idx = None       # [sum(send_counts)] local row ids to pack, grouped by destination rank
        self.send_counts = None    # python list, rows sent to each rank
        self.recv_counts = None    # python list, halo rows received from each rank
        self.send_reduce = None    # CSRGraph [n_own, sum(send_counts)]: owner-side deterministic reduction of returned grads
        self.halo_ids = None       # int64 [n_halo] GLOBAL ids of the halo rows, ascending (== grouped by owner rank)
        self.merged = None         # CSRGraph [n_own, n_own + n_halo]: both halves over ONE column space (own rows first, then
                                   # the halo rows) -- for operands whose halo is already in place (the static input features)
        self.nnz = 0


def _csr_rows(rowptr, col, val, rows):
    """Sub-CSR made of `rows` (int64 indices) in the given order."""
    deg = rowptr[rows + 1] - rowptr[rows]
    new_ptr = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=rowptr.device)
    torch.cumsum(deg, 0, out=new_ptr[1:])
    total = int(new_ptr[-1])
    if total == 0:
        empty = torch.zeros(0, dtype=col.dtype, device=col.device)
        return new_ptr, empty, (None if val is None else val[:0])
    # edge positions: start of each row repeated + offset within the row
    starts = torch.repeat_interleave(rowptr[rows] - new_ptr[:-1], deg)
    pos = starts + torch.arange(total, device=rowptr.device)
    return new_ptr, col[pos], (None if val is None else val[pos])


def _split_block(p, rowptr, col, val, bounds, dev):
    """Fill the Partition's two column halves from this rank's row block (local rowptr, GLOBAL column ids).  Returns the
    sorted global ids of the halo nodes and their owner ranks."""
    world = len(bounds) - 1
    bounds_t = torch.tensor(bounds, dtype=torch.int64, device=dev)
    col = col.to(torch.int64)
    p.nnz = int(col.numel())
    owned = (col >= p.own_begin) & (col < p.own_end)
    halo_ids = torch.unique(col[~owned])                       # sorted by global id == grouped by owner rank
    p.n_halo = int(halo_ids.numel())
    p.halo_ids = halo_ids
    owner = torch.bucketize(halo_ids, bounds_t[1:], right=True)
    p.recv_counts = torch.bincount(owner, minlength=world).tolist()

    deg = rowptr[1:] - rowptr[:-1]
    p.inv_deg = 1.0 / deg.clamp(min=1).to(torch.float32)
    row_of_edge = torch.repeat_interleave(torch.arange(p.n_own, device=dev), deg)

    def sub_csr(mask, local_ids, n_cols):
        cnt = torch.bincount(row_of_edge[mask], minlength=p.n_own)
        ptr = torch.zeros(p.n_own + 1, dtype=torch.int64, device=dev)
        torch.cumsum(cnt, 0, out=ptr[1:])
        return CSRGraph(ptr, local_ids.to(torch.int32), None if val is None else val[mask], p.n_own, n_cols, check=False)

    # boolean masking keeps the row-major edge order, so each half is a valid CSR over the same rows
    p.local = sub_csr(owned, col[owned] - p.own_begin, p.n_own)
    halo_col = torch.searchsorted(halo_ids, col[~owned])
    p.halo = sub_csr(~owned, halo_col, p.n_halo)
    merged_col = col - p.own_begin
    merged_col[~owned] = p.n_own + halo_col
    ptr = torch.zeros(p.n_own + 1, dtype=torch.int64, device=dev)
    torch.cumsum(deg, 0, out=ptr[1:])
    p.merged = CSRGraph(ptr, merged_col.to(torch.int32), val, p.n_own, p.n_own + p.n_halo, check=False)
    return halo_ids, owner


def _finish_send(p, send_lists, dev):
    """send_lists[q]: sorted LOCAL row ids rank q needs from this rank (empty for q == rank)."""
    p.send_counts = [int(t.numel()) for t in send_lists]
    p.send_idx = torch.cat(send_lists) if send_lists else torch.zeros(0, dtype=torch.int64, device=dev)
    # deterministic owner-side reduction of returned halo gradients: row r sums the slots of send_idx equal to r
    n_send = int(p.send_idx.numel())
    if n_send:
        order = torch.argsort(p.send_idx, stable=True)
        cnt = torch.bincount(p.send_idx, minlength=p.n_own)
        sptr = torch.zeros(p.n_own + 1, dtype=torch.int64, device=dev)
        torch.cumsum(cnt, 0, out=sptr[1:])
        p.send_reduce = CSRGraph(sptr, order.to(torch.int32), None, p.n_own, n_send, check=False)
    return p


def partition_contiguous(graph, world, rank, bounds=None):
    """Row-partition `graph` (the SAME full CSRGraph on every rank) into `world` contiguous blocks and build this
    rank's Partition with NO setup communication: every rank derives what its peers need from the full graph.  `bounds`
    (len world+1) overrides the equal-rows split (METIS part boundaries after a relabelling -- partition.bounds_from_book /
    relabel_by_parts -- or an nnz-balanced split).  For graphs too large to hold everywhere use `partition_rows`."""
    n = graph.n_rows
    dev = graph.device
    if bounds is None:
        bounds = [(n * r) // world for r in range(world + 1)]
    p = Partition()
    p.rank, p.world = rank, world
    p.own_begin, p.own_end = bounds[rank], bounds[rank + 1]
    p.n_own = p.own_end - p.own_begin
    rp = graph.rowptr
    e0, e1 = int(rp[p.own_begin]), int(rp[p.own_end])
    val = None if graph.val is None else graph.val[e0:e1]
    _split_block(p, rp[p.own_begin:p.own_end + 1] - e0, graph.col[e0:e1], val, bounds, dev)
    # what each peer needs from me: the unique columns of ITS rows that fall in my range (every rank derives this
    # from the same full graph, so it equals the peer's halo list restricted to my block)
    send = []
    for q in range(world):
        if q == rank:
            send.append(torch.zeros(0, dtype=torch.int64, device=dev))
            continue
        q0, q1 = int(rp[bounds[q]]), int(rp[bounds[q + 1]])
        qc = graph.col[q0:q1].to(torch.int64)
        send.append(torch.unique(qc[(qc >= p.own_begin) & (qc < p.own_end)]) - p.own_begin)
    return _finish_send(p, send, dev)


def partition_rows(rowptr, col, val, bounds, rank, group=None):
    """Build this rank's Partition from ITS OWN ROW BLOCK only: `rowptr` (local, starting at 0) / `col` (GLOBAL ids) / `val`
    are the CSR rows bounds[rank] .. bounds[rank+1] -- what a rank loads from its own part file.  No rank ever holds the
    whole adjacency (RMAT-27 would be ~27 GB of indices per rank otherwise).  The send lists come from ONE exchange: every
    rank tells each owner which of its rows it needs (the halo ids, already unique and sorted), so they are consistent by
    construction -- there is nothing to `verify()`."""
    world = len(bounds) - 1
    dev = rowptr.device
    p = Partition()
    p.rank, p.world = rank, world
    p.own_begin, p.own_end = int(bounds[rank]), int(bounds[rank + 1])
    p.n_own = p.own_end - p.own_begin
    if rowptr.numel() != p.n_own + 1:
        raise ValueError("the row block has %d rows, bounds give %d" % (rowptr.numel() - 1, p.n_own))
    halo_ids, owner = _split_block(p, rowptr - rowptr[0], col, val, list(bounds), dev)
    empty = torch.zeros(0, dtype=torch.int64, device=dev)
    if world == 1:
        return _finish_send(p, [empty], dev)
    staged = dist.get_backend(group) != "nccl"                # gloo moves host tensors
    cdev = torch.device("cpu") if staged else dev
    mine = torch.tensor(p.recv_counts, dtype=torch.int64, device=cdev)
    table = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(table, mine, group=group)                 # table[r][q] = rows r needs from q
    want = [int(table[q][rank]) for q in range(world)]        # rows q needs from me
    need = [halo_ids[owner == q].to(cdev) for q in range(world)]
    got = [torch.empty(want[q], dtype=torch.int64, device=cdev) for q in range(world)]
    opsl = []
    for q in range(world):
        if q == rank:
            continue
        if need[q].numel():
            opsl.append(dist.P2POp(dist.isend, need[q], q, group))
        if want[q]:
            opsl.append(dist.P2POp(dist.irecv, got[q], q, group))
    for r in (dist.batch_isend_irecv(opsl) if opsl else []):
        r.wait()
    send = []
    for q in range(world):
        ids = got[q].to(dev)
        if ids.numel() and (int(ids.min()) < p.own_begin or int(ids.max()) >= p.own_end):
            raise RuntimeError("rank %d asked rank %d for rows it does not own (bounds differ between ranks)" % (q, rank))
        send.append(ids - p.own_begin if q != rank else empty)
    return _finish_send(p, send, dev)


def nnz_balanced_bounds(graph, world):
    """Row boundaries giving every rank about the same number of nonzeros (power-law rows make equal-row splits
    uneven)."""
    targets = torch.arange(1, world, device=graph.device, dtype=torch.int64) * (graph.nnz // world)
    cuts = torch.searchsorted(graph.rowptr, targets).tolist()
    return [0] + cuts + [graph.n_rows]


# ----------------------------------------------------------------------------------------------------------------
class ExchangeWatchdog:
    """First contact with a transport can hang (a grouped send/recv whose peers disagree, an IPC set-up that never completes): the
    host then sits in a synchronize() for ever and the job dies without a word.  An exchange registers an event recorded behind it;
    a daemon thread polls the pending events and, when one is still incomplete `timeout` seconds after it was queued, prints the
    phase name AND the Python stack of every thread (faulthandler), then EXITS THE PROCESS with code 3 (never re-executes anything).

    What is watched (DGLL_EXCHANGE_WATCHDOG): "startup" (default) = the start-up self-test and the first `arm_first` (16) exchanges
    -- the hangs this exists for happen at first contact; a steady-state job is not watched, so a process stopped under a debugger
    (SIGSTOP), a serialised `rocprofv3 --pmc` run or a first-step module load cannot get a healthy job killed without a traceback
    (the clock starts when an exchange is QUEUED, not when it runs); "always" = every exchange; "off".
    DGLL_EXCHANGE_TIMEOUT_S (default 120, 0 = off).  Host-tensor exchanges (gloo on CPU) block in wait() and are bracketed by
    `guard()` instead.  Events come from a small pool (no allocation in the steady state when watching is on)."""

    def __init__(self, timeout=None, rank=0, mode=None, arm_first=16):
        self.timeout = float(os.environ.get("DGLL_EXCHANGE_TIMEOUT_S", "120")) if timeout is None else float(timeout)
        self.mode = (mode or os.environ.get("DGLL_EXCHANGE_WATCHDOG", "startup")).lower()
        if self.mode not in ("startup", "always", "off"):
            raise ValueError("DGLL_EXCHANGE_WATCHDOG must be startup, always or off")
        if self.mode == "off":
            self.timeout = 0.0
        self.arm_first = int(arm_first)
        self.watched = 0
        self.rank = rank
        self._pending = []
        self._lock = threading.Lock()
        self._thread = None
        self._event_pool = []
        self.on_timeout = self._die            # tests replace it

    def armed(self):
        """Whether the next exchange is watched."""
        return self.timeout > 0 and (self.mode == "always" or self.watched < self.arm_first)

    def rearm(self):
        """A NEW exchange pattern is about to make first contact (the halo mode switched, another set of buffers, a new DistGraph):
        watch the next `arm_first` exchanges again.  Without this the "startup" mode's budget could be spent before the pattern
        that hangs is ever used (resolve_halo_mode switches forms after the first 16 exchanges)."""
        self.watched = 0

    def _die(self, phase, age):
        print("dgll_amd.dist: rank %d: exchange phase '%s' did not complete within %.0f s -- exiting (code 3); Python stacks follow" % (
            self.rank, phase, age), file=sys.stderr, flush=True)
        try:
            import faulthandler

            faulthandler.dump_traceback(file=sys.stderr, all_threads=True)
            sys.stderr.flush()
        except Exception:  # noqa: BLE001
            pass
        os._exit(3)

    def _run(self):
        while True:
            time.sleep(min(1.0, max(self.timeout / 4, 0.01)))
            now = time.monotonic()
            with self._lock:
                keep = []
                for phase, probe, t0, event in self._pending:
                    if probe():
                        if event is not None and len(self._event_pool) < 8:
                            self._event_pool.append(event)
                        continue
                    if now - t0 > self.timeout:
                        self.on_timeout(phase, now - t0)
                        continue
                    keep.append((phase, probe, t0, event))
                self._pending = keep

    def _ensure_thread(self):
        if self._thread is None and self.timeout > 0:
            self._thread = threading.Thread(target=self._run, name="dgll-exchange-watchdog", daemon=True)
            self._thread.start()

    def watch_stream(self, phase, stream):
        """Record an event behind the exchange on `stream` and watch it -- when this exchange is to be watched at all (armed())."""
        if not self.armed():
            return
        self.watched += 1
        with self._lock:
            event = self._event_pool.pop() if self._event_pool else None
        if event is None:
            event = torch.cuda.Event()
        event.record(stream)
        self.watch_event(phase, event, _pooled=True)

    def watch_event(self, phase, event, _pooled=False):
        """event: a torch.cuda.Event recorded behind the exchange on its stream."""
        if self.timeout <= 0:
            return
        self._ensure_thread()
        with self._lock:
            self._pending.append((phase, event.query, time.monotonic(), event if _pooled else None))

    def guard(self, phase, force=False):
        """Context manager around a host-blocking wait (force: watched whatever the mode -- the start-up self-test)."""
        wd = self
        on = wd.timeout > 0 and (force or wd.armed())

        class _G:
            def __enter__(self_g):
                self_g.done = False
                if on:
                    wd.watched += 1
                    wd._ensure_thread()
                    with wd._lock:
                        wd._pending.append((phase, lambda: self_g.done, time.monotonic(), None))

            def __exit__(self_g, *exc):
                self_g.done = True

        return _G()


class _Exchange:
    """Halo exchange of packed row blocks, two interchangeable forms (DGLL_EXCHANGE = p2p | alltoall, default p2p):

      p2p       one grouped batch of point-to-point send/recv to all peers at once (xGMI is point-to-point: every link is driven
                concurrently, no ring)                                                     -- dist.batch_isend_irecv
      alltoall  the same packed buffers through ONE all-to-all-v collective with per-peer row counts   -- dist.all_to_all_single
                (the fallback when the grouped p2p form misbehaves on a given RCCL / driver combination)

    RCCL ("nccl"): device buffers, stream-ordered -- the product path.  gloo has no device send/recv (it would read the
    device pointer from the host with no ordering against the GPU kernels that fill the buffer: silent races), so for
    device tensors on gloo -- the functional multi-rank tests that share one GPU -- the rows are staged through host
    memory explicitly: copy out (synchronising), send/recv on CPU tensors, copy back on the communication stream."""

    def __init__(self, part, group=None, form=None, watchdog=None):
        self.part, self.group = part, group
        self.form = (form or os.environ.get("DGLL_EXCHANGE", "p2p")).lower()
        if self.form not in ("p2p", "alltoall"):
            raise ValueError("DGLL_EXCHANGE must be 'p2p' or 'alltoall', got %r" % self.form)
        self.watchdog = watchdog if watchdog is not None else ExchangeWatchdog(rank=part.rank)
        self.bytes_sent = self.bytes_received = self.calls = 0
        self.phase = "exchange"
        self.fault_p2p = False      # tests only: the p2p form delivers the right number of rows in the wrong order

    def _staged(self, t):
        return t.is_cuda and self.part.world > 1 and dist.is_initialized() and dist.get_backend(self.group) != "nccl"

    def start(self, send_buf, recv_buf, reverse=False, more=()):
        """One exchange moving `send_buf` rows to their peers and filling `recv_buf`; `more` = further
        (send, recv) pairs with the same row layout (e.g. the fp32 score rows next to the feature rows)."""
        with rng("exchange"):
            return self._start(send_buf, recv_buf, reverse, more)

    def _start(self, send_buf, recv_buf, reverse, more):
        p = self.part
        s_counts, r_counts = (p.recv_counts, p.send_counts) if reverse else (p.send_counts, p.recv_counts)
        opsl, works, copy_back = [], [], []
        self.calls += 1
        for sb, rb in ((send_buf, recv_buf),) + tuple(more):
            self.bytes_sent += sb.numel() * sb.element_size()
            self.bytes_received += rb.numel() * rb.element_size()
            if self._staged(sb) or self._staged(rb):
                host_recv = torch.empty(rb.shape, dtype=rb.dtype, device="cpu")
                copy_back.append((rb, host_recv))
                sb, rb = sb.cpu(), host_recv                 # .cpu() waits for the kernels that produced the rows
            if self.form == "alltoall":
                if p.world > 1:
                    works.append(dist.all_to_all_single(rb, sb.contiguous(), output_split_sizes=list(r_counts),
                                                        input_split_sizes=list(s_counts), group=self.group, async_op=True))
                continue
            if self.fault_p2p and sb.shape[0] > 1:
                sb = torch.roll(sb, 1, 0)
            so = ro = 0
            for q in range(p.world):
                if s_counts[q]:
                    opsl.append(dist.P2POp(dist.isend, sb[so:so + s_counts[q]], q, self.group))
                if r_counts[q]:
                    opsl.append(dist.P2POp(dist.irecv, rb[ro:ro + r_counts[q]], q, self.group))
                so += s_counts[q]
                ro += r_counts[q]
        reqs = works + (dist.batch_isend_irecv(opsl) if opsl else [])
        return (reqs, copy_back)

    def wait(self, handle):
        with rng("exchange"):
            return self._wait(handle)

    def _wait(self, handle):
        reqs, copy_back = handle
        device_side = bool(reqs) and torch.cuda.is_available() and dist.is_initialized() and dist.get_backend(self.group) == "nccl"
        if device_side:
            for r in reqs:
                r.wait()                                     # stream-ordered: returns at once; a hang shows up behind it
            self.watchdog.watch_stream(self.phase, torch.cuda.current_stream())
        else:
            with self.watchdog.guard(self.phase):
                for r in reqs:
                    r.wait()
        for dev_buf, host_buf in copy_back:
            dev_buf.copy_(host_buf)


def _pack_rows(store, idx):
    """store[idx] as a contiguous [len(idx), ld] block (the rows a rank sends): the HIP row gather on the GPU (16-byte lanes over
    the padded rows; torch's index_select took 0.11 ms for the 87 MB of a 47-wide layer at 8 ranks), index_select elsewhere."""
    if not idx.numel():
        return store[:0]
    if store.is_cuda and store.dtype in (torch.bfloat16, torch.float32) and store.dim() == 2 and store.stride(1) == 1:
        from .cache import gather_rows

        out = torch.empty((int(idx.numel()), store.shape[1]), dtype=store.dtype, device=store.device)
        return gather_rows(store, idx, out=out)
    return store.index_select(0, idx)


def _aggregate_forward(engine, h_own, reduce):
    """out[row] = reduce_j A[row, j] h[j] over the partitioned adjacency (h_own: this rank's rows)."""
    p = engine.part
    feat = h_own.shape[1]
    scale = p.inv_deg if reduce == "mean" else None
    # exchange buffers hold whole (16-byte padded) rows so that every message is one contiguous block
    h_store, h_view = engine.rows_of(h_own)
    send_store = _pack_rows(h_store, p.send_idx)
    halo_store, halo_view = engine.alloc_rows(p.n_halo, feat, h_own.dtype)
    _, out = engine.alloc_rows(p.n_own, feat, h_own.dtype)
    with engine.comm_scope():
        reqs = engine.exchange.start(send_store, halo_store)
    # owned-column edges (the bulk of the work) overlap the exchange
    engine.spmm(p.local, h_view, out, row_scale=scale)
    with engine.comm_scope():
        engine.exchange.wait(reqs)
    engine.join_comm()
    if p.n_halo:   # halo-column edges: their (scaled) sums are ADDED to the rows that have any -- the others stay untouched
        engine.spmm(p.halo, halo_view, out, row_scale=scale, accumulate=2)
    return out


def _aggregate_backward_start(engine, g):
    """First half of A^T . g across the ranks (g already carries the mean's 1/deg): the gradients of the halo rows are
    produced and sent on their way.  Whatever the caller issues before _aggregate_backward_finish overlaps the exchange."""
    p = engine.part
    feat = g.shape[1]
    _, g = engine.rows_of(g)                 # 16-byte aligned rows: a 47-wide gradient would fall on the scalar kernel
    n_send = int(p.send_idx.numel())
    recv_store, recv_view = engine.alloc_rows(n_send, feat, g.dtype)
    ghalo_store, ghalo_view = engine.alloc_rows(p.n_halo, feat, g.dtype)
    if p.n_halo:   # halo gradients first: they have to travel
        engine.spmm(engine.transposed(p.halo), g, ghalo_view)
    with engine.comm_scope():
        reqs = engine.exchange.start(ghalo_store, recv_store, reverse=True)
    return g, reqs, recv_view, n_send, (ghalo_store, recv_store)      # the stores stay referenced until the finish


def _aggregate_backward_finish(engine, state, into=None, gate=None):
    """Second half: the local transposed SpMM (still overlapping the exchange), then the pieces that came back are reduced
    in fixed order.  `into`: a row buffer the result is ACCUMULATED into (the self-path gradient of a fused layer);
    `gate`: rows of the forward activations -- the final accumulation zeroes the result where gate <= 0."""
    p = engine.part
    g, reqs, recv_view, n_send, _keep = state
    if into is None:
        _, g_own = engine.alloc_rows(p.n_own, g.shape[1], g.dtype)
        engine.spmm(engine.transposed(p.local), g, g_own, gate=gate)
    else:
        g_own = into
        engine.spmm(engine.transposed(p.local), g, g_own, accumulate=True, gate=gate)
    with engine.comm_scope():
        engine.exchange.wait(reqs)
    engine.join_comm()
    if n_send:     # returned halo gradients: fixed-order reduction at the owner, no atomics; only the rows that were sent
        engine.spmm(p.send_reduce, recv_view, g_own, accumulate=2, gate=gate)   # are touched (the gate is linear: applied
    return g_own                                                                # to the local part above and to this one)


def _aggregate_backward(engine, g, into=None, gate=None):
    return _aggregate_backward_finish(engine, _aggregate_backward_start(engine, g), into=into, gate=gate)


class DistAggregate(torch.autograd.Function):
    """Neighbour aggregation over the distributed adjacency: out[row] = reduce_j A[row, j] h[j], with h partitioned by
    owner.  forward(h_own [n_own, F]) -> [n_own, F]; reduce 'sum' or 'mean'."""

    @staticmethod
    def forward(ctx, h_own, engine, reduce):
        ctx.engine, ctx.reduce = engine, reduce
        return _aggregate_forward(engine, h_own, reduce)

    @staticmethod
    def backward(ctx, g):
        engine = ctx.engine
        if ctx.reduce == "mean":
            g = g * engine.part.inv_deg.unsqueeze(1).to(g.dtype)
        return _aggregate_backward(engine, g.contiguous()), None, None


class _DistSageLayer(torch.autograd.Function):
    """act(h.Ws + reduce_A(h).Wn) on this rank's rows -- the partitioned twin of fused_layers._SageGraphLayer: the
    neighbour-path gradient is accumulated onto the self-path gradient by the SpMM epilogues, the ReLU mask of the layer
    below rides on the last of them (`gate_input`), and this layer's own mask is skipped when the layer above already
    applied it (`grad_is_gated`).  `placed`: the static input halo (first layer; no gradient to the raw features)."""

    @staticmethod
    def forward(ctx, h, ws, wn, engine, reduce, relu, grad_is_gated, gate_input, placed, token=None, bits_box=None):
        from . import dense, fused_layers

        ctx.token = token

        agg = engine.aggregate_static(placed, reduce) if placed is not None else _aggregate_forward(engine, h, reduce)
        wsd, wnd = dense.wcast(ws, h), dense.wcast(wn, h)
        if h.is_cuda and dense._mfma_ok(h, agg) and ws.shape[1] <= 256:
            if relu and bits_box is not None and fused_layers.GATE_BITS:      # sign bits of the activation: fused_layers._tag_bits
                out, bits = dense.transform_bf16(h, wsd.t(), agg, wnd.t(), relu=relu, bits_out=True)
                bits_box.append(bits)
            else:
                out = dense.transform_bf16(h, wsd.t(), agg, wnd.t(), relu=relu)
        else:
            out = dense.mm2_nt(h, wsd.t(), agg, wnd.t(), relu=relu)
        ctx.engine, ctx.reduce, ctx.relu = engine, reduce, relu
        ctx.grad_is_gated, ctx.gate_input = grad_is_gated, gate_input
        ctx.wparams = (ws, wn)
        ctx.save_for_backward(h, agg, wsd, wnd, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, g):
        from . import dense

        h, agg, wsd, wnd, out = ctx.saved_tensors
        engine = ctx.engine
        g = g.contiguous()
        if ctx.relu and not ctx.grad_is_gated and not (ctx.token is not None and ctx.token.masked):
            g = torch.ops.aten.threshold_backward(g, out, 0)
        state = None
        if ctx.needs_input_grad[0]:   # the neighbour-path gradient first: its halo part has to travel
            inv = engine.part.inv_deg if ctx.reduce == "mean" else None
            if inv is not None and g.is_cuda and dense._mfma_ok(g) and wnd.shape[0] <= 256:
                gagg = dense.transform_bf16(g, wnd, row_scale=inv)                 # (g.Wn^T) / deg in one kernel
            else:
                gagg = dense.mm_nt(g, wnd)
                if inv is not None:
                    gagg = gagg * inv.unsqueeze(1).to(gagg.dtype)
            state = _aggregate_backward_start(engine, gagg)
        # everything below up to the finish overlaps the exchange
        if ctx.needs_input_grad[1] and ctx.needs_input_grad[2]:
            gws, gwn = dense.grad_weight_pair(h, agg, g, out1=grad_slot_of(ctx.wparams[0]),     # one launch, g read once
                                              out2=grad_slot_of(ctx.wparams[1]))
        else:
            gws = dense.grad_weight(h, g, out=grad_slot_of(ctx.wparams[0])) if ctx.needs_input_grad[1] else None
            gwn = dense.grad_weight(agg, g, out=grad_slot_of(ctx.wparams[1])) if ctx.needs_input_grad[2] else None
        gh = None
        if state is not None:
            _, gh = engine.rows_of(dense.input_grad(g, wsd))                      # self path
            gate = h if (ctx.gate_input and h.stride(1) == 1) else None
            gh = _aggregate_backward_finish(engine, state, into=gh, gate=gate)
            if ctx.gate_input and gate is None:
                gh = torch.ops.aten.threshold_backward(gh, h, 0)
        return gh, gws, gwn, None, None, None, None, None, None, None, None


class _DistSageLayerTransformFirst(torch.autograd.Function):
    """act(h.Ws + reduce_A(h.Wn)) -- the narrowing layer: the NARROW product crosses the links and is aggregated."""

    @staticmethod
    def forward(ctx, h, ws, wn, engine, reduce, relu, grad_is_gated, gate_input, token=None):
        from . import dense, fused_layers

        ctx.token = token
        ctx.h_bits = fused_layers._bits_of(h) if gate_input else None
        wsd, wnd = dense.wcast(ws, h), dense.wcast(wn, h)
        z = (dense.transform_bf16(h, wnd.t(), ld_align=64 if wn.shape[1] < 64 else None)
             if (h.is_cuda and dense._mfma_ok(h) and wn.shape[1] <= 256) else dense.mm_nt(h, wnd.t()))
        aggz = _aggregate_forward(engine, z, reduce)
        if h.is_cuda and dense._mfma_ok(h) and aggz.dtype == torch.bfloat16 and aggz.stride(1) == 1 and ws.shape[1] <= 256:
            out = dense.transform_bf16(h, wsd.t(), relu=relu, addend=aggz)
        else:
            out = dense.mm_nt(h, wsd.t(), relu=relu, addend=aggz)
        ctx.engine, ctx.reduce, ctx.relu = engine, reduce, relu
        ctx.grad_is_gated, ctx.gate_input = grad_is_gated, gate_input
        ctx.wparams = (ws, wn)
        ctx.save_for_backward(h, wsd, wnd, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, g):
        from . import dense

        h, wsd, wnd, out = ctx.saved_tensors
        engine = ctx.engine
        masked = ctx.relu and not ctx.grad_is_gated and not (ctx.token is not None and ctx.token.masked)
        if masked:                                                               # (masked) gradient in aligned rows
            _, gm = engine.alloc_rows(g.shape[0], g.shape[1], g.dtype)
            torch.ops.aten.threshold_backward.grad_input(g, out, 0, grad_input=gm)
        else:
            _, gm = engine.rows_of(g)            # the loss kernel's gradient already has 16-byte aligned rows: used as it is
        if ctx.reduce == "mean":
            # the 1 / deg of the mean on a scaled copy of the narrow gradient; over the WHOLE pitch of the rows when that is one
            # contiguous block (a vectorised pass; the padding's product is never read) instead of a strided pass over the view
            full = engine.full_pitch(gm)
            if full is not None:
                gp_full = torch.empty_like(full)
                torch.mul(full, engine.part.inv_deg.unsqueeze(1).to(g.dtype), out=gp_full)
                gp = gp_full[:, :g.shape[1]]
            else:
                _, gp = engine.alloc_rows(g.shape[0], g.shape[1], g.dtype)
                torch.mul(gm, engine.part.inv_deg.unsqueeze(1).to(g.dtype), out=gp)
        else:
            gp = gm
        state = _aggregate_backward_start(engine, gp)
        gws = dense.grad_weight(h, gm, out=grad_slot_of(ctx.wparams[0])) if ctx.needs_input_grad[1] else None      # overlaps the exchange
        gz = _aggregate_backward_finish(engine, state)
        gwn = dense.grad_weight(h, gz, out=grad_slot_of(ctx.wparams[1])) if ctx.needs_input_grad[2] else None
        gh = None
        if ctx.needs_input_grad[0]:
            if g.is_cuda and dense._mfma_ok(gm, gz) and wsd.shape[0] <= 256 and (not ctx.gate_input or h.stride(1) == 1):
                gh = dense.transform_bf16(gm, wsd, gz, wnd, out_gate=h if ctx.gate_input else None, gate_bits=ctx.h_bits)
            else:
                gh = dense.mm2_nt(gm, wsd, gz, wnd)
                if ctx.gate_input:
                    gh = torch.ops.aten.threshold_backward(gh, h, 0)
        return gh, gws, gwn, None, None, None, None, None, None


class DistGatAggregate(torch.autograd.Function):
    """Multi-head edge-softmax aggregation (sparseGatConv semantics, gatconv.py:111-148) over the partitioned adjacency.
    One exchange moves the halo rows of h together with their per-head scores t; the `local` half runs un-normalised
    (numerator, denominator) while the exchange flies, the `halo` half accumulates and normalises.  Backward: the
    row pass over both halves (grad_s accumulates), then the column pass over halo^T -- whose results travel back to the
    owners -- overlapped with the column pass over local^T; returned pieces are reduced in fixed order."""

    @staticmethod
    def forward(ctx, h_own, s_own, t_own, engine, heads, fo, alpha, apply_elu, halo_local=False):
        """halo_local: h / s / t arrive for own AND halo rows ([n_own + n_halo, ...]: the first layer, whose transform of the
        statically placed halo inputs was evaluated on this rank) -- nothing is exchanged in either direction; the gradients of
        the halo rows are returned to the caller, whose autograd turns them into this rank's partial weight gradients."""
        from . import ops_edge as oe

        p = engine.part
        feat = heads * fo
        dev, dtype = h_own.device, h_own.dtype
        h_store, h_view = engine.rows_of(h_own)
        s_own = s_own.detach().float().contiguous()
        t_own = t_own.detach().float().contiguous()
        has_halo = p.n_halo > 0
        _, out = engine.alloc_rows(p.n_own, feat, dtype)
        rowsum = torch.empty((p.n_own, heads), dtype=torch.float32, device=dev)
        merged = halo_local and p.merged is not None and has_halo
        if merged:
            # own and halo rows of h / t sit in ONE buffer (the transform ran on both): ONE pass over the merged adjacency instead of a
            # pass per column half -- the second of those re-read and re-wrote every output row (numerator, denominator) for the
            # ~5 remote edges a row has: 551 us next to the local half's 1168 us on a rank of four
            h_all, t_all = h_view, t_own
            h_view, halo_h = h_all[:p.n_own], h_all[p.n_own:]
            s_own, t_own, halo_t = s_own[:p.n_own], t_all[:p.n_own], t_all[p.n_own:]
            oe.gat_fwd_part(p.merged, h_all, s_own, t_all, out, rowsum, heads, fo, alpha, apply_elu, raw=False, accumulate=False)
            ctx.engine, ctx.cfg, ctx.halo_local, ctx.merged = engine, (heads, fo, alpha, apply_elu), halo_local, True
            ctx.save_for_backward(h_all, t_all, s_own, out, rowsum)
            return out
        if halo_local:
            h_view, halo_h = h_view[:p.n_own], h_view[p.n_own:]
            s_own, t_own, halo_t = s_own[:p.n_own], t_own[:p.n_own], t_own[p.n_own:]
            oe.gat_fwd_part(p.local, h_view, s_own, t_own, out, rowsum, heads, fo, alpha, apply_elu, raw=has_halo, accumulate=False)
        else:
            send_h = _pack_rows(h_store, p.send_idx)
            send_t = t_own.index_select(0, p.send_idx) if p.send_idx.numel() else t_own[:0]
            halo_store, halo_h = engine.alloc_rows(p.n_halo, feat, dtype)
            halo_t = torch.empty((p.n_halo, heads), dtype=torch.float32, device=dev)
            with engine.comm_scope():
                reqs = engine.exchange.start(send_h, halo_store, more=((send_t, halo_t),))
            oe.gat_fwd_part(p.local, h_view, s_own, t_own, out, rowsum, heads, fo, alpha, apply_elu, raw=has_halo, accumulate=False)
            with engine.comm_scope():
                engine.exchange.wait(reqs)
            engine.join_comm()
        if has_halo:
            oe.gat_fwd_part(p.halo, halo_h, s_own, halo_t, out, rowsum, heads, fo, alpha, apply_elu, raw=False, accumulate=True)
        ctx.engine, ctx.cfg, ctx.halo_local, ctx.merged = engine, (heads, fo, alpha, apply_elu), halo_local, False
        ctx.save_for_backward(h_view, halo_h, s_own, t_own, halo_t, out, rowsum)
        return out

    @staticmethod
    def backward(ctx, g):
        from . import ops_edge as oe

        engine = ctx.engine
        heads, fo, alpha, apply_elu = ctx.cfg
        p = engine.part
        feat = heads * fo
        if ctx.merged:      # one rows pass (declared the only launch: exact dd_i) and one transposed pass over merged^T
            h_all, t_all, s_own, out, rowsum = ctx.saved_tensors
            dev, dtype = h_all.device, h_all.dtype
            _, gv = engine.rows_of(g.to(dtype))
            _, dn = engine.alloc_rows(p.n_own, feat, dtype)
            dd = torch.empty((p.n_own, heads), dtype=torch.float32, device=dev)
            grad_s = torch.empty((p.n_own, heads), dtype=torch.float32, device=dev)
            oe.gat_bwd_rows_part(p.merged, h_all, s_own, t_all, out, gv, rowsum, dn, dd, grad_s, heads, fo, alpha, apply_elu, 3)
            _, gh_all = engine.alloc_rows(p.n_own + p.n_halo, feat, dtype)
            gt_all = torch.empty((p.n_own + p.n_halo, heads), dtype=torch.float32, device=dev)
            gs_all = torch.zeros((p.n_own + p.n_halo, heads), dtype=torch.float32, device=dev)   # a halo node's s is never used here
            gs_all[:p.n_own] = grad_s
            oe.gat_bwd_cols_part(engine.transposed(p.merged), dn, h_all, t_all, s_own, dd, gh_all, gt_all, heads, fo, alpha)
            return gh_all, gs_all, gt_all, None, None, None, None, None, None
        h_view, halo_h, s_own, t_own, halo_t, out, rowsum = ctx.saved_tensors
        dev, dtype = h_view.device, h_view.dtype
        _, gv = engine.rows_of(g.to(dtype))
        _, dn = engine.alloc_rows(p.n_own, feat, dtype)
        dd = torch.empty((p.n_own, heads), dtype=torch.float32, device=dev)
        grad_s = torch.empty((p.n_own, heads), dtype=torch.float32, device=dev)
        # two launches over the column halves of A when there is a halo: the exact dd_i is bilinear in the halves' sums, so the first
        # launch parks its (sa, sb, sw) in `partial` and the second finalises (phases 4 / 6); alone, the local launch is declared the
        # only one (3)  -- csrc/gat_kernel.hpp
        partial = torch.empty((p.n_own, 3 * heads), dtype=torch.float32, device=dev) if p.n_halo else None
        oe.gat_bwd_rows_part(p.local, h_view, s_own, t_own, out, gv, rowsum, dn, dd, grad_s, heads, fo, alpha, apply_elu,
                             4 if p.n_halo else 3, partial=partial)
        if p.n_halo:
            oe.gat_bwd_rows_part(p.halo, halo_h, s_own, halo_t, out, gv, rowsum, dn, dd, grad_s, heads, fo, alpha, apply_elu, 6,
                                 partial=partial)
        if ctx.halo_local:      # gradients of own and halo rows side by side; nothing travels
            _, gh_all = engine.alloc_rows(p.n_own + p.n_halo, feat, dtype)
            gt_all = torch.empty((p.n_own + p.n_halo, heads), dtype=torch.float32, device=dev)
            gs_all = torch.zeros((p.n_own + p.n_halo, heads), dtype=torch.float32, device=dev)   # a halo node's s is never used here
            gs_all[:p.n_own] = grad_s
            if p.n_halo:
                oe.gat_bwd_cols_part(engine.transposed(p.halo), dn, halo_h, halo_t, s_own, dd, gh_all[p.n_own:], gt_all[p.n_own:],
                                     heads, fo, alpha)
            oe.gat_bwd_cols_part(engine.transposed(p.local), dn, h_view, t_own, s_own, dd, gh_all[:p.n_own], gt_all[:p.n_own],
                                 heads, fo, alpha)
            return gh_all, gs_all, gt_all, None, None, None, None, None, None
        n_send = int(p.send_idx.numel())
        gh_halo_store, gh_halo = engine.alloc_rows(p.n_halo, feat, dtype)
        gt_halo = torch.empty((p.n_halo, heads), dtype=torch.float32, device=dev)
        recv_store, recv_gh = engine.alloc_rows(n_send, feat, dtype)
        recv_gt = torch.empty((n_send, heads), dtype=torch.float32, device=dev)
        if p.n_halo:   # contributions to REMOTE source nodes first: they have to travel back to their owners
            oe.gat_bwd_cols_part(engine.transposed(p.halo), dn, halo_h, halo_t, s_own, dd, gh_halo, gt_halo, heads, fo, alpha)
        with engine.comm_scope():
            reqs = engine.exchange.start(gh_halo_store, recv_store, reverse=True, more=((gt_halo, recv_gt),))
        _, grad_h = engine.alloc_rows(p.n_own, feat, dtype)
        grad_t = torch.empty((p.n_own, heads), dtype=torch.float32, device=dev)
        oe.gat_bwd_cols_part(engine.transposed(p.local), dn, h_view, t_own, s_own, dd, grad_h, grad_t, heads, fo, alpha)
        with engine.comm_scope():
            engine.exchange.wait(reqs)
        engine.join_comm()
        if n_send:     # fixed-order reduction of the returned pieces at the owner
            engine.spmm(p.send_reduce, recv_gh, grad_h, accumulate=2)
            engine.spmm(p.send_reduce, recv_gt, grad_t, accumulate=2)
        return grad_h, grad_s, grad_t, None, None, None, None, None, None


class _Placed(tuple):
    """Handle of DistGraph.place_input_halo: (own rows, halo rows, all rows) of the input features as views of one buffer, plus
    what is derived from them once per aggregation mode (DistGraph.input_aggregate_all)."""

    def __new__(cls, items):
        obj = super().__new__(cls, items)
        obj.agg_all = {}
        return obj


class _DistSageInputLayerAll(torch.autograd.Function):
    """The FIRST layer, act(x.Ws + reduce_A(x).Wn), on this rank's own rows AND on its halo rows.

    The first layer's inputs depend on no parameter: x of a halo node is placed once (place_input_halo) and so is its aggregated
    input row reduce_A(x)_j, which the owner computes (input_aggregate_all).  With both on the rank, the halo nodes' first-layer
    output is RECOMPUTED here -- (n_own + n_halo) rows of a K = F_in transform -- instead of being received every step as
    n_halo rows of hidden width: at 8 ranks of the bench graph that is 0.15 ms of MFMA work against 347 MB over the links per
    direction and step.  The backward mirrors it: the gradient that reaches a halo node's first-layer output stays on this rank
    and goes straight into this rank's PARTIAL weight gradient (x_j and its aggregate are here; the layer has no input gradient);
    the gradient all-reduce the ranks do anyway sums the partials.  The owner applies the same ReLU mask to the same output, and
    the mask is linear in the gradient, so the sum over ranks equals the owner-side reduction of the exchange it replaces."""

    @staticmethod
    def forward(ctx, ws, wn, engine, reduce, relu, grad_is_gated, placed, bits_box=None):
        from . import dense, fused_layers

        p = engine.part
        x_all = placed[2]
        agg_all = engine.input_aggregate_all(placed, reduce)
        scale = p.inv_deg if reduce == "mean" else None
        engine.spmm(p.merged, x_all, agg_all[:p.n_own], row_scale=scale)        # this rank's rows: aggregated every step
        wsd, wnd = dense.wcast(ws, x_all), dense.wcast(wn, x_all)
        if x_all.is_cuda and dense._mfma_ok(x_all, agg_all) and ws.shape[1] <= 256:
            if relu and bits_box is not None and fused_layers.GATE_BITS:      # sign bits of own AND halo rows: the layer above gates both
                out, bits = dense.transform_bf16(x_all, wsd.t(), agg_all, wnd.t(), relu=relu, bits_out=True)
                bits_box.append(bits)
            else:
                out = dense.transform_bf16(x_all, wsd.t(), agg_all, wnd.t(), relu=relu)
        else:
            out = dense.mm2_nt(x_all, wsd.t(), agg_all, wnd.t(), relu=relu)
        ctx.relu, ctx.grad_is_gated = relu, grad_is_gated
        ctx.wparams = (ws, wn)
        ctx.save_for_backward(x_all, agg_all, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, g):
        from . import dense

        x_all, agg_all, out = ctx.saved_tensors
        g = dense._rows(g)
        if ctx.relu and not ctx.grad_is_gated:
            g = torch.ops.aten.threshold_backward(g, out, 0)
        if ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:
            gws, gwn = dense.grad_weight_pair(x_all, agg_all, g, out1=grad_slot_of(ctx.wparams[0]),   # own + halo rows: this rank's partial
                                              out2=grad_slot_of(ctx.wparams[1]))
        else:
            gws = dense.grad_weight(x_all, g, out=grad_slot_of(ctx.wparams[0])) if ctx.needs_input_grad[0] else None
            gwn = dense.grad_weight(agg_all, g, out=grad_slot_of(ctx.wparams[1])) if ctx.needs_input_grad[1] else None
        return gws, gwn, None, None, None, None, None, None


class _DistSageLayerOnAll(torch.autograd.Function):
    """act(h.Ws + reduce_A(h).Wn) for a layer whose input arrives for own AND halo rows (h_all, from _DistSageInputLayerAll):
    one pass over the merged adjacency forward, the two transposed halves backward -- no exchange in either direction.  The
    gradient it returns covers all n_own + n_halo rows (the self path only the own ones)."""

    @staticmethod
    def forward(ctx, h_all, ws, wn, engine, reduce, relu, grad_is_gated, gate_input, bits_box=None):
        from . import dense, fused_layers

        p = engine.part
        scale = p.inv_deg if reduce == "mean" else None
        _, agg = engine.alloc_rows(p.n_own, h_all.shape[1], h_all.dtype)
        engine.spmm(p.merged, h_all, agg, row_scale=scale)
        h = h_all[:p.n_own]
        wsd, wnd = dense.wcast(ws, h), dense.wcast(wn, h)
        if h.is_cuda and dense._mfma_ok(h, agg) and ws.shape[1] <= 256:
            if relu and bits_box is not None and fused_layers.GATE_BITS:      # sign bits of the activation: fused_layers._tag_bits
                out, bits = dense.transform_bf16(h, wsd.t(), agg, wnd.t(), relu=relu, bits_out=True)
                bits_box.append(bits)
            else:
                out = dense.transform_bf16(h, wsd.t(), agg, wnd.t(), relu=relu)
        else:
            out = dense.mm2_nt(h, wsd.t(), agg, wnd.t(), relu=relu)
        ctx.engine, ctx.reduce, ctx.relu = engine, reduce, relu
        ctx.grad_is_gated, ctx.gate_input = grad_is_gated, gate_input
        ctx.h_bits = fused_layers._bits_of(h_all) if gate_input else None
        ctx.wparams = (ws, wn)
        ctx.save_for_backward(h_all, agg, wsd, wnd, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, g):
        from . import dense, fused_layers

        h_all, agg, wsd, wnd, out = ctx.saved_tensors
        engine = ctx.engine
        p = engine.part
        h = h_all[:p.n_own]
        g = g.contiguous()
        if ctx.relu and not ctx.grad_is_gated:
            g = torch.ops.aten.threshold_backward(g, out, 0)
        gh_all = None
        # The single-GPU step's backward order (fused_layers.BACKWARD_ORDER, round 5): aggregate first -- gt = merged^T (scale . g), ONE
        # plain weighted SpMM into own + halo rows (no read-modify-write of the output, no gate operand) -- then the input gradient as
        # MFMA launches that read the ReLU mask of the layer below as bits: gate(g.Ws^T + gt.Wn^T) on the own rows, gate(gt.Wn^T) on the
        # halo rows (which have no self path here: their owner adds it).  Replaces (g.Wn^T)/deg, g.Ws^T, an accumulating gated SpMM
        # over local^T and a gated SpMM over halo^T.
        agg_first = (fused_layers.BACKWARD_ORDER != "transform-first" and ctx.needs_input_grad[0] and engine._spmm_fn is None
                     and g.is_cuda and dense._mfma_ok(g) and ops.pitch16_ok(g) and wsd.shape[1] <= wsd.shape[0] <= 256
                     and p.merged is not None and (not ctx.gate_input or h_all.stride(1) == 1))
        if agg_first:
            # two launches, one per column half of A: the halo half's rows are short (a remote node feeds ~3 of this rank's rows) and take
            # the row-per-slot kernel; one launch over merged^T ran them through the wave-per-row kernel: 815 us against 500 + 300
            _, gt_all = engine.alloc_rows(p.n_own + p.n_halo, g.shape[1], g.dtype)
            for half, rows in ((p.local, gt_all[:p.n_own]), (p.halo, gt_all[p.n_own:])):
                if rows.shape[0] == 0:
                    continue
                ht = engine.transposed(half)
                engine.spmm(ht, g, rows, val=engine.transposed_scale(half, ctx.reduce))
            _, gh_all = engine.alloc_rows(p.n_own + p.n_halo, h_all.shape[1], h_all.dtype)
            gate = h_all if ctx.gate_input else None
            bits = ctx.h_bits
            dense.transform_bf16(g, wsd, gt_all[:p.n_own], wnd, out=gh_all[:p.n_own],
                                 out_gate=gate[:p.n_own] if gate is not None else None,
                                 gate_bits=bits[:p.n_own] if bits is not None else None)
            if p.n_halo:
                dense.transform_bf16(gt_all[p.n_own:], wnd, out=gh_all[p.n_own:],
                                     out_gate=gate[p.n_own:] if gate is not None else None,
                                     gate_bits=bits[p.n_own:] if bits is not None else None)
        elif ctx.needs_input_grad[0]:
            inv = p.inv_deg if ctx.reduce == "mean" else None
            if inv is not None and g.is_cuda and dense._mfma_ok(g) and wnd.shape[0] <= 256:
                gagg = dense.transform_bf16(g, wnd, row_scale=inv)                 # (g.Wn^T) / deg in one kernel
            else:
                gagg = dense.mm_nt(g, wnd)
                if inv is not None:
                    gagg = gagg * inv.unsqueeze(1).to(gagg.dtype)
            _, gagg = engine.rows_of(gagg)
            _, gh_all = engine.alloc_rows(p.n_own + p.n_halo, h_all.shape[1], h_all.dtype)
            dense.input_grad(g, wsd, out=gh_all[:p.n_own])                         # self path: own rows only, written in place
            gate = h_all if (ctx.gate_input and h_all.stride(1) == 1) else None
            engine.spmm(engine.transposed(p.local), gagg, gh_all[:p.n_own], accumulate=True,
                        gate=gate[:p.n_own] if gate is not None else None)
            if p.n_halo:   # what the exchange used to carry back to the owners stays here (see _DistSageInputLayerAll)
                engine.spmm(engine.transposed(p.halo), gagg, gh_all[p.n_own:], gate=gate[p.n_own:] if gate is not None else None)
            if ctx.gate_input and gate is None:
                gh_all = torch.ops.aten.threshold_backward(gh_all, h_all, 0)
        if ctx.needs_input_grad[1] and ctx.needs_input_grad[2]:
            gws, gwn = dense.grad_weight_pair(h, agg, g, out1=grad_slot_of(ctx.wparams[0]), out2=grad_slot_of(ctx.wparams[1]))
        else:
            gws = dense.grad_weight(h, g, out=grad_slot_of(ctx.wparams[0])) if ctx.needs_input_grad[1] else None
            gwn = dense.grad_weight(agg, g, out=grad_slot_of(ctx.wparams[1])) if ctx.needs_input_grad[2] else None
        return gh_all, gws, gwn, None, None, None, None, None, None


def cost_balanced_bounds(rowptr, n_parts, edge_cost=1, row_cost=0):
    """Contiguous row blocks of about equal COST, cost(block) = edge_cost . nnz + row_cost . rows: cut points on the prefix sum
    edge_cost . rowptr[i] + row_cost . i (monotone), not at n_rows / n_parts -- on a hubs-first RMAT order equal-row blocks are far
    from equal-nnz blocks, and equal-nnz blocks are far from equal-row ones (the last block of RMAT-27 / 8 holds half the rows).
    The costs are bytes: per edge one gathered row + the column id, per row the output row + the row pointer (+ what the
    dense transform moves per row)."""
    n = int(rowptr.numel() - 1)
    c = rowptr.to(torch.int64) * int(edge_cost)
    if row_cost:
        c = c + torch.arange(n + 1, device=rowptr.device, dtype=torch.int64) * int(row_cost)
    total = int(c[-1])
    targets = (torch.arange(1, n_parts, device=rowptr.device, dtype=torch.float64) * (total / n_parts)).to(torch.int64)
    cuts = torch.searchsorted(c, targets).clamp_(0, n).tolist()
    bounds = [0] + cuts + [n]
    for i in range(1, len(bounds)):                      # monotone even when one row outweighs a whole share
        bounds[i] = max(bounds[i], bounds[i - 1])
    return bounds


def row_block(graph, lo, hi):
    """Rows [lo, hi) of a CSR adjacency as their own CSRGraph over ALL source columns (views of the col / val arrays, a rebased
    copy of the row pointers)."""
    lo, hi = int(lo), int(hi)
    e0, e1 = int(graph.rowptr[lo]), int(graph.rowptr[hi])
    return CSRGraph(graph.rowptr[lo:hi + 1] - e0, graph.col[e0:e1], None if graph.val is None else graph.val[e0:e1], hi - lo,
                    graph.n_cols, check=False)


class RowBlockShard:
    """BASELINE config 5's sharding: A is cut into contiguous, cost-balanced row blocks, one per rank
    (process shape: one process per GPU as the reference's mp.spawn, MQGCN.py:161-163); the SOURCE rows X are replicated on every
    rank (RMAT-27, F = 128 bf16: 34 GB of 288 GB), so a layer's aggregation needs no exchange at all -- every rank runs the same
    SpMM kernel over its block against the full X and owns the output rows [own_begin, own_end).  A following layer would need
    the outputs of all ranks: gather_output() (one all-gather of the padded blocks), timed separately by the bench.

    spmm_fn (graph, x, reduce) -> rows: injected by the CPU tests (the product kernels are GPU-only)."""

    def __init__(self, full_graph, world, rank, edge_cost=1, row_cost=0, bounds=None, group=None, spmm_fn=None):
        self.world, self.rank, self.group = int(world), int(rank), group
        self.bounds = list(bounds) if bounds is not None else cost_balanced_bounds(full_graph.rowptr, world, edge_cost, row_cost)
        if len(self.bounds) != self.world + 1 or self.bounds[0] != 0 or self.bounds[-1] != full_graph.n_rows:
            raise ValueError("bounds must run from 0 to n_rows in world + 1 steps")
        self.n_rows_total, self.n_cols = full_graph.n_rows, full_graph.n_cols
        self.own_begin, self.own_end = self.bounds[self.rank], self.bounds[self.rank + 1]
        self.block = row_block(full_graph, self.own_begin, self.own_end)
        at = full_graph.rowptr[torch.tensor(self.bounds, device=full_graph.rowptr.device)].tolist()
        self.block_nnz = [int(at[r + 1] - at[r]) for r in range(self.world)]
        self._spmm_fn = spmm_fn

    @property
    def n_own(self):
        return self.own_end - self.own_begin

    def own_copy(self):
        """Own the block's arrays (copies), so that the full graph can be freed; builds the kernel's row schedule."""
        b = self.block
        self.block = CSRGraph(b.rowptr.clone(), b.col.clone(), None if b.val is None else b.val.clone(), b.n_rows, b.n_cols, check=False)
        if self.block.is_cuda and self._spmm_fn is None:
            self.block.plan()
        return self

    def aggregate(self, x_full, reduce="mean", out=None):
        """Rows [own_begin, own_end) of reduce(A) . X from the replicated X; no communication."""
        if x_full.shape[0] != self.n_cols:
            raise ValueError("the replicated source matrix has %d rows, the adjacency gathers from %d" % (x_full.shape[0], self.n_cols))
        if self._spmm_fn is not None:
            y = self._spmm_fn(self.block, x_full, reduce)
            if out is not None:
                out.copy_(y)
                return out
            return y
        return ops.spmm_raw(self.block, x_full, reduce=reduce, out=out)

    def gather_output(self, y_own, out=None):
        """[n_rows_total, F]: every rank's output rows in one buffer -- what a following layer would gather from.  One broadcast
        per rank straight into that rank's row slice of `out` (the blocks differ in rows: an all-gather would pad every block to
        the largest one, which on a hubs-first order holds half the rows), all in flight together."""
        if out is None:
            out = y_own.new_empty((self.n_rows_total, y_own.shape[1]))
        out[self.own_begin:self.own_end].copy_(y_own)
        if self.world == 1:
            return out
        handles = [dist.broadcast(out[self.bounds[r]:self.bounds[r + 1]], src=dist.get_global_rank(self.group, r) if self.group is not None else r,
                                  group=self.group, async_op=True)
                   for r in range(self.world) if self.bounds[r + 1] > self.bounds[r]]
        for h in handles:
            h.wait()
        return out


class DistGraph:
    """Per-rank engine: owns the Partition, the communication stream and the kernels' scratch."""

    def __init__(self, part, device, group=None, spmm_fn=None):
        self.part = part
        self.device = torch.device(device)
        self.exchange = _Exchange(part, group)
        self._spmm_fn = spmm_fn
        self.comm_stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None
        self.wait_events = None          # set to [] to have join_comm() time the compute stream's stall behind every exchange
        # DGLL_HALO_MODE = recompute | exchange | auto (default recompute).  What happens to the WIDE rows of a remote neighbour in
        # the first two layers: `recompute` evaluates the first layer on own + halo rows (its inputs are static) and exchanges
        # nothing for layers 0 and 1 -- compute proportional to the halo rows; `exchange` sends / receives the hidden-width rows
        # every step and direction.  Which one wins depends on the fabric (xGMI bandwidth RCCL reaches for grouped send/recv), which
        # no model measures: `auto` = resolve_halo_mode() times both for a few warm-up steps on the live ranks and keeps the faster.
        self.halo_mode = os.environ.get("DGLL_HALO_MODE", "recompute")
        if self.halo_mode not in ("recompute", "exchange", "auto"):
            raise ValueError("DGLL_HALO_MODE must be recompute, exchange or auto")
        self.halo_recompute = self.halo_mode != "exchange"       # sage_forward / spgat_forward read this
        self.halo_mode_timings = None
        if self.device.type == "cuda":   # build the schedules up front, not inside the first timed step
            for g in (part.local, part.halo):
                g.plan()
                self.transposed(g).plan()
            if part.send_reduce is not None:
                part.send_reduce.plan()

    def resolve_halo_mode(self, step, reps=3):
        """DGLL_HALO_MODE=auto: run `step` (one whole training step of the caller; these are ordinary warm-up steps) `reps` times in
        either mode after one untimed step each, take the MAX over ranks of the mean step time (the step is the slowest rank's),
        keep the faster mode on every rank.  Returns the chosen mode; `halo_mode_timings` keeps both figures (ms)."""
        if self.halo_mode != "auto":
            return "recompute" if self.halo_recompute else "exchange"
        timings = {}
        for mode in ("recompute", "exchange"):
            self.halo_recompute = mode == "recompute"
            self._rearm_watchdog()                        # each form's exchanges make their own first contact
            step()
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            if dist.is_initialized():
                dist.barrier(self.exchange.group)
            t0 = time.perf_counter()
            for _ in range(reps):
                step()
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            t = torch.tensor([(time.perf_counter() - t0) / reps * 1e3], dtype=torch.float64, device=self.device)
            if dist.is_initialized():
                dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.exchange.group)
            timings[mode] = float(t.item())
        self.halo_mode_timings = timings
        self.halo_recompute = timings["recompute"] <= timings["exchange"]
        self.halo_mode = "recompute" if self.halo_recompute else "exchange"
        self._rearm_watchdog()
        return self.halo_mode

    def _rearm_watchdog(self):
        wd = getattr(self.exchange, "watchdog", None)      # (a stand-in transport of the modelling tools has none)
        if wd is not None:
            wd.rearm()

    def verify(self):
        """Before anything is timed: (1) cross-check the locally derived exchange lists across ranks (a mismatch would otherwise
        hang the first send/recv): every rank must see the same graph, and what r sends to q must be what q expects from r;
        (2) SELF-TEST of the chosen exchange form (DGLL_EXCHANGE): a rank-stamped pattern -- (global row id, sender rank) per row --
        travels through the very code path of the halo exchange, on the communication stream, to every peer and back (the
        transposed direction), and is checked value by value; the watchdog turns a hang into an exit with the phase name."""
        if not dist.is_initialized() or self.part.world == 1:
            return
        p = self.part
        comm_dev = self.device if dist.get_backend(self.exchange.group) == "nccl" else torch.device("cpu")
        mine = torch.tensor(p.send_counts + p.recv_counts + [p.nnz, p.n_own], dtype=torch.int64, device=comm_dev)
        everyone = [torch.empty_like(mine) for _ in range(p.world)]
        dist.all_gather(everyone, mine, group=self.exchange.group)
        for q, row in enumerate(everyone):
            row = row.tolist()
            if row[p.world + p.rank] != p.send_counts[q]:
                raise RuntimeError("halo exchange lists disagree: rank %d sends %d rows to rank %d, which expects %d "
                                   "(the ranks did not build the same graph)" % (p.rank, p.send_counts[q], q, row[p.world + p.rank]))
        # every rank must reach the same verdict: a form that misdelivers on ONE rank is abandoned by all of them together
        err = None
        try:
            self.self_test()
        except RuntimeError as exc:
            err = exc
        bad = torch.tensor([0 if err is None else 1], dtype=torch.int32, device=comm_dev)
        dist.all_reduce(bad, op=dist.ReduceOp.MAX, group=self.exchange.group)
        if int(bad.item()) == 0:
            return
        if self.exchange.form == "p2p" and os.environ.get("DGLL_EXCHANGE_FALLBACK", "1") != "0":
            if p.rank == 0:
                print("dgll_amd.dist: the grouped point-to-point exchange failed its start-up self-test%s; switching every rank to "
                      "DGLL_EXCHANGE=alltoall" % ("" if err is None else " (%s)" % err), file=sys.stderr, flush=True)
            self.exchange.form = "alltoall"
            err2 = None
            try:
                self.self_test()
            except RuntimeError as exc:
                err2 = exc
            bad = torch.tensor([0 if err2 is None else 1], dtype=torch.int32, device=comm_dev)
            dist.all_reduce(bad, op=dist.ReduceOp.MAX, group=self.exchange.group)
            if int(bad.item()) == 0:
                return
            err = err2 or err
        raise err if err is not None else RuntimeError("rank %d: another rank's exchange self-test failed" % p.rank)

    def self_test(self):
        p, ex = self.part, self.exchange
        dev = self.device
        owner = torch.repeat_interleave(torch.arange(p.world, device=dev), torch.tensor(p.recv_counts, device=dev))
        dest = torch.repeat_interleave(torch.arange(p.world, device=dev), torch.tensor(p.send_counts, device=dev))
        sent_ids = p.send_idx.to(dev) + p.own_begin
        phase, ex.phase = ex.phase, "start-up self-test (%s)" % ex.form
        try:
            # forward direction: owners -> halo slots
            send = torch.stack([sent_ids, torch.full_like(sent_ids, p.rank)], dim=1).contiguous()
            recv = torch.full((p.n_halo, 2), -1, dtype=torch.int64, device=dev)
            with self.comm_scope():
                ex.wait(ex.start(send, recv))
            self.join_comm()
            want = torch.stack([p.halo_ids.to(dev), owner], dim=1)
            # transposed direction: halo slots -> owners
            back = torch.full((int(p.send_idx.numel()), 2), -1, dtype=torch.int64, device=dev)
            with self.comm_scope():
                ex.wait(ex.start(torch.stack([p.halo_ids.to(dev), torch.full_like(owner, p.rank)], dim=1).contiguous(), back, reverse=True))
            self.join_comm()
            want_back = torch.stack([sent_ids, dest], dim=1)
            if dev.type == "cuda":
                with ex.watchdog.guard(ex.phase + ": synchronize", force=True):
                    torch.cuda.current_stream(dev).synchronize()
            bad = int((recv != want).any(dim=1).sum()), int((back != want_back).any(dim=1).sum())
        finally:
            ex.phase = phase
        if bad[0] or bad[1]:
            raise RuntimeError("rank %d: the '%s' exchange delivered %d of %d halo rows and %d of %d returned rows wrong in the start-up "
                               "self-test (set DGLL_EXCHANGE=%s to try the other form)" % (
                                   p.rank, ex.form, bad[0], p.n_halo, bad[1], int(p.send_idx.numel()), "alltoall" if ex.form == "p2p" else "p2p"))
        ex.bytes_sent = ex.bytes_received = ex.calls = 0

    # ---- helpers used by DistAggregate
    def _ld(self, feat, dtype):
        epv = 8 if dtype == torch.bfloat16 else 4
        return -(-feat // epv) * epv

    def alloc_rows(self, n, feat, dtype):
        """(storage [n, feat padded to 16 bytes] contiguous, view [n, feat]).  The padding columns are NOT initialised: every
        consumer either masks what lies past `feat` (the MFMA transform's K tail, the gather kernels' ragged last vector) or
        lets it flow into outputs nobody reads (the split-K weight gradient); zero-filling them cost eight strided fill launches
        per step of the 47-wide layer."""
        ld = self._ld(feat, dtype)
        store = torch.empty((n, ld), dtype=dtype, device=self.device)
        return store, (store[:, :feat] if ld != feat else store)

    def rows_of(self, h):
        """(padded rows [n, feat rounded up to 16 bytes], view [n, feat]) holding h: h ITSELF -- whatever its row pitch -- when its
        rows start on 16-byte boundaries and the padding up to the rounded width lies inside its allocation (e.g. the narrow
        product the MFMA transform writes on a 128-byte pitch), else a copy into fresh padded rows."""
        ld = self._ld(h.shape[1], h.dtype)
        esz = h.element_size()
        if h.dim() == 2 and h.stride(1) == 1 and h.stride(0) >= ld and (h.stride(0) * esz) % 16 == 0 and \
                (self.device.type == "cpu" or h.data_ptr() % 16 == 0) and \
                (h.storage_offset() + max(h.shape[0] - 1, 0) * h.stride(0) + ld) * esz <= h.untyped_storage().nbytes():
            return h.as_strided((h.shape[0], ld), (h.stride(0), 1), h.storage_offset()), h
        store, view = self.alloc_rows(h.shape[0], h.shape[1], h.dtype)
        view.copy_(h)
        return store, view

    @staticmethod
    def full_pitch(h):
        """h's rows over their WHOLE pitch as one contiguous [n, pitch] alias (None when the last row's pitch runs past the
        allocation or the rows are not a plain leading block of it)."""
        if h.dim() != 2 or h.stride(1) != 1 or h.stride(0) < h.shape[1]:
            return None
        pitch = h.stride(0)
        if (h.storage_offset() + h.shape[0] * pitch) * h.element_size() > h.untyped_storage().nbytes():
            return None
        return h.as_strided((h.shape[0], pitch), (pitch, 1), h.storage_offset())

    def spmm(self, graph, x, out, row_scale=None, accumulate=False, val=None, gate=None):
        if self._spmm_fn is not None:
            y = self._spmm_fn(graph, x, val)
            if accumulate == 1 or accumulate is True:
                y = y + out
            if row_scale is not None:
                y = y * row_scale.unsqueeze(1).to(y.dtype)
            if gate is not None:
                y = torch.where(gate > 0, y, torch.zeros_like(y))
            if accumulate == 2 and accumulate is not True:
                y = y + out
            out.copy_(y)
            return out
        return ops.spmm_raw(graph, x, val=val, reduce="sum", out=out, row_scale=row_scale, accumulate=accumulate, gate=gate)

    def transposed(self, graph):
        return graph.transpose()[0]

    def transposed_scale(self, half, reduce):
        """Edge values of half^T for the backward of reduce_A over one column half of this rank's adjacency: 1 / deg(i) of the
        destination row i each edge came from -- the FULL degree (part.inv_deg), not the half's -- times the half's own values; cached."""
        key = "_dgll_tscale_" + reduce
        val = getattr(half, key, None)
        if val is None:
            ht = half.transpose()[0]
            val = ht.val
            if reduce == "mean":
                scale = self.part.inv_deg.to(torch.float32)[ht.col.long()]
                val = scale if val is None else val * scale
            setattr(half, key, val if val is not None else False)
        return None if val is False else val

    class _Scope:
        def __init__(self, engine):
            self.engine = engine
            self.ctx = None

        def __enter__(self):
            e = self.engine
            if e.comm_stream is not None:
                e.comm_stream.wait_stream(torch.cuda.current_stream(e.device))
                self.ctx = torch.cuda.stream(e.comm_stream)
                self.ctx.__enter__()

        def __exit__(self, *exc):
            if self.ctx is not None:
                self.ctx.__exit__(*exc)

    def comm_scope(self):
        """Work issued inside runs on the communication stream, ordered after everything already queued."""
        return DistGraph._Scope(self)

    def join_comm(self):
        if self.comm_stream is not None:
            cur = torch.cuda.current_stream(self.device)
            if self.wait_events is not None:      # bench: how long the compute stream sits in this wait = the EXPOSED exchange time
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(cur)
                cur.wait_stream(self.comm_stream)
                b.record(cur)
                self.wait_events.append((a, b))
            else:
                cur.wait_stream(self.comm_stream)

    def exposed_wait_ms(self):
        """Sum of the compute stream's stalls in join_comm() since `wait_events = []` was set (synchronises)."""
        if not self.wait_events:
            return 0.0
        torch.cuda.current_stream(self.device).synchronize()
        return float(sum(a.elapsed_time(b) for a, b in self.wait_events))

    # ---- layer-level API
    def aggregate(self, h_own, reduce="mean"):
        return DistAggregate.apply(h_own, self, reduce)

    def place_input_halo(self, x_own):
        """One-time placement of the halo rows of the INPUT features (they never change: like DistDGL, each partition
        keeps the features of its halo nodes).  Returns a handle for aggregate_static; no communication afterwards."""
        p = self.part
        h_store, h_view = self.rows_of(x_own)
        send_store = h_store.index_select(0, p.send_idx) if p.send_idx.numel() else h_store[:0]
        # own rows and halo rows in ONE buffer, [n_own + n_halo, F]: the first layer then aggregates both column halves in
        # a single pass over the merged adjacency (no second sweep over the rows, no read-modify-write of the output)
        all_store, all_view = self.alloc_rows(p.n_own + p.n_halo, x_own.shape[1], x_own.dtype)
        all_store[:p.n_own].copy_(h_store)
        halo_store = all_store[p.n_own:]
        with self.comm_scope():
            self.exchange.wait(self.exchange.start(send_store, halo_store))
        self.join_comm()
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()
            p.merged.plan()
        return _Placed((all_view[:p.n_own], all_view[p.n_own:], all_view))

    def input_aggregate_all(self, placed, reduce="mean"):
        """[n_own + n_halo, F] rows of reduce_A(x): the first n_own are this rank's (the caller re-computes them every step --
        no work of the model is skipped), the rest belong to the halo nodes and are received ONCE from their owners: like the
        input features themselves they depend on no parameter.  Collective on first use (every rank calls it at the same point
        of its first forward)."""
        if reduce in placed.agg_all:
            return placed.agg_all[reduce]
        p = self.part
        x_all = placed[2]
        store, view = self.alloc_rows(p.n_own + p.n_halo, x_all.shape[1], x_all.dtype)
        self.spmm(p.merged, x_all, view[:p.n_own], row_scale=p.inv_deg if reduce == "mean" else None)
        send_store = store[:p.n_own].index_select(0, p.send_idx) if p.send_idx.numel() else store[:0]
        with self.comm_scope():
            self.exchange.wait(self.exchange.start(send_store, store[p.n_own:]))
        self.join_comm()
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()
        placed.agg_all[reduce] = view
        return view

    def aggregate_static(self, placed, reduce="mean"):
        """Aggregation of input features whose halo rows were placed once (no gradient flows to raw features)."""
        p = self.part
        h_view, halo_view = placed[0], placed[1]
        scale = p.inv_deg if reduce == "mean" else None
        _, out = self.alloc_rows(p.n_own, h_view.shape[1], h_view.dtype)
        if len(placed) > 2 and p.merged is not None:
            self.spmm(p.merged, placed[2], out, row_scale=scale)
            return out
        self.spmm(p.local, h_view, out, row_scale=scale)
        if p.n_halo:
            self.spmm(p.halo, halo_view, out, row_scale=scale, accumulate=2)
        return out

    def permute_to_local(self, x_block):
        """Rows of this rank's block in global order -> local order (the identity for contiguous partitions; kept as
        the one place a relabelling partitioner would hook in)."""
        return x_block

    def gat_layer(self, x, Ws, a1s, a2s, alpha, concat, halo_local=False):
        """One (multi-head) sparseGatConv layer on this rank's rows: the partitioned twin of
        nn.Convolution.gatconv._fused_heads (mode 0, attention dropout inactive).  halo_local: x holds own AND halo rows
        (statically placed inputs): the transform and the scores are evaluated for both, nothing is exchanged."""
        from . import dense, ops
        from .nn.Convolution.gatconv import pack_heads

        heads, fo = len(Ws), Ws[0].shape[1]
        W, A = pack_heads(Ws, a1s, a2s, fo)          # the heads' parameters as two matrices, a handful of launches each way
        h = dense.linear(x, W)
        p = self.part
        if (halo_local and p.merged is not None and p.n_halo > 0 and h.is_cuda and ops.head_width_padded(fo, h.dtype, pow2=False) == fo
                and h.shape[0] == p.n_own + p.n_halo):
            # Own and halo rows of h sit in ONE buffer (the transform ran on both): the layer is the single-GPU autograd node over the
            # rank's merged adjacency (rows = own nodes = its first columns) -- one pass per direction instead of one per column half
            # (the second of those re-read and re-wrote every output row for the ~5 remote edges a row has), the forward forms t_j from
            # the gathered rows, and the scores' own gradient w.r.t. h rides in the transposed pass's epilogue instead of a
            # [rows, 2 heads] x [2 heads, 256] product and an elementwise add over all own + halo rows.  Nothing is exchanged.
            return ops.gat_layer(p.merged, h, A, heads, alpha, apply_elu=concat, pack_scores=False)
        st = dense.skinny_linear(h, A.to(h.dtype))
        fo_pad = ops.head_width_padded(fo, h.dtype)
        hp = h if fo_pad == fo else torch.nn.functional.pad(h.view(-1, heads, fo), (0, fo_pad - fo)).reshape(-1, heads * fo_pad)
        out = DistGatAggregate.apply(hp, st[:, :heads], st[:, heads:], self, heads, fo_pad, alpha, concat, halo_local)
        return out if fo_pad == fo else out.view(-1, heads, fo_pad)[:, :, :fo].reshape(-1, heads * fo)

    def spgat_forward(self, model, x_local, placed_input=None, activations=False):
        """SpGAT.forward (gatconv.py:194-199) on this rank's rows; input/attention dropout must be inactive.  placed_input
        (place_input_halo): the first layer's transform x.W is evaluated on the halo rows too instead of exchanging its
        heads * nhid-wide result every step (dist._DistSageInputLayerAll has the argument; here it needs no placed aggregate).
        activations: return elu(out head) without the final log_softmax (SpGAT.forward_activations: for a fused cross-entropy)."""
        if model.training and model.dropout > 0:
            raise NotImplementedError("the partitioned GAT path runs with dropout inactive (eval mode or p = 0)")
        halves = [att._split_a() for att in model.attentions]
        local = self.halo_recompute and isinstance(placed_input, _Placed) and not x_local.requires_grad
        x = self.gat_layer(placed_input[2] if local else x_local, [att.W for att in model.attentions], [h[0] for h in halves],
                           [h[1] for h in halves], model.attentions[0].alpha, True, halo_local=local)
        a1, a2 = model.out_att._split_a()
        x = torch.nn.functional.elu(self.gat_layer(x, [model.out_att.W], [a1], [a2], model.out_att.alpha, False))
        if activations:
            return x
        return torch.log_softmax(x, dim=1, dtype=torch.float32 if x.dtype == torch.bfloat16 else None)

    def sage_forward(self, model, x_local, placed_input=None):
        """Full-graph GraphSage forward on this rank's rows (x_local in local row order).  `placed_input`: handle from
        place_input_halo(x_local) -- the first layer then needs no exchange."""
        from . import fused_layers

        layers = model.gcn
        fusable = [fused_layers.can_fuse(layer, x_local.is_cuda) for layer in layers]
        # as in GraphSage.forward_graph: layer i returns the gradient of its input already masked by layer i-1's ReLU
        gates = [i > 0 and fusable[i] and fusable[i - 1] and layers[i - 1].activation is not None for i in range(len(layers))]
        h = x_local
        first = 0
        # Layers 0 and 1 without any per-step exchange: the first layer is evaluated on own AND halo rows (its inputs are static,
        # _DistSageInputLayerAll), the second aggregates over the merged adjacency.  Only layers from the third on exchange.
        if (self.halo_recompute and isinstance(placed_input, _Placed) and len(layers) >= 2 and not x_local.requires_grad
                and self.part.merged is not None and all(fused_layers.can_fuse(layers[i], True) for i in (0, 1))
                and not layers[0].transform_first(x_local) and layers[1].hidden_dim >= layers[1].input_dim):
            relu0, relu1 = layers[0].activation is not None, layers[1].activation is not None
            box0 = [] if relu0 else None
            h_all = _DistSageInputLayerAll.apply(layers[0].weight, layers[0].neighborAgg.weight, self, layers[0].aggr_neighbor_method,
                                                 relu0, relu0, placed_input, box0)    # layer 1 returns its gradient masked
            if box0:
                fused_layers._tag_bits(h_all, box0[0])
            gated1 = bool(len(layers) > 2 and gates[2] and relu1)
            box = [] if relu1 else None
            h = _DistSageLayerOnAll.apply(h_all, layers[1].weight, layers[1].neighborAgg.weight, self,
                                          layers[1].aggr_neighbor_method, relu1, gated1, relu0, box)
            if box:
                fused_layers._tag_bits(h, box[0])
            first = 2
        for li, layer in enumerate(layers):
            if li < first:
                continue
            reduce = layer.aggr_neighbor_method
            static = li == 0 and placed_input is not None and not x_local.requires_grad and not layer.transform_first(h)
            if fusable[li]:
                relu = layer.activation is not None
                gated = bool(li + 1 < len(layers) and gates[li + 1] and relu)
                token = ops.GateToken() if (relu and not gated) else None      # see fused_layers.sage_graph_layer
                if layer.transform_first(h):
                    h = _DistSageLayerTransformFirst.apply(h, layer.weight, layer.neighborAgg.weight, self, reduce, relu,
                                                           gated, gates[li], token)
                else:
                    box = [] if relu else None
                    h = _DistSageLayer.apply(h, layer.weight, layer.neighborAgg.weight, self, reduce, relu, gated, gates[li],
                                             placed_input if static else None, token, box)
                    if box:
                        fused_layers._tag_bits(h, box[0])
                if token is not None:
                    h._dgll_gate_token = token
                continue
            if static:
                h = layer.transform_block(h, self.aggregate_static(placed_input, reduce=reduce))
            elif layer.transform_first(h):
                from . import dense

                z = dense.linear(h, layer.neighborAgg.weight)
                h = layer.finish_transform_first(h, self.aggregate(z, reduce=reduce))
            else:
                h = layer.transform_block(h, self.aggregate(h, reduce=reduce))
        return h


# ----------------------------------------------------------------------------------------------------------------
class RaCoM:
    """Gradient sharing in the spirit of the reference's RaCoM queue (README.md:27-37; MQGCN.py:55-79 all-reduces
    every parameter separately and divides by world_size).  Here: ONE flattened bucket, one all-reduce on a dedicated
    stream, averaged and copied back into .grad; `all_reduce_and_wait` is the synchronous form (identical to DDP),
    `launch` / `wait` let the caller overlap the reduction with other work."""

    def __init__(self, params, device, group=None, average="reference", flat=None, in_place=True):
        """average: "reference" = all-reduce SUM, then divide by world_size (MQGCN.py:61-64); "ddp" = divide, then
        all-reduce SUM (torch DDP's order).  The two are bit-identical whenever world_size is a power of two -- every
        configuration BASELINE names (1/2/4/8 GPUs) -- and differ in the last bit otherwise.
        flat: an optim.FlatAdam that owns the parameters.  Its gradient buffer already IS the flattened bucket (the weight-gradient
        kernels write their slots in place), so nothing is copied in or out: in_place=True all-reduces that buffer itself and
        hands the 1 / world_size of the "reference" average to the optimizer's kernel (`grad_scale`: .grad then holds the SUM over
        ranks); in_place=False (several reductions in flight, RaCoMOptimizer) moves the whole buffer with ONE copy each way."""
        if average not in ("reference", "ddp"):
            raise ValueError("average must be 'reference' or 'ddp'")
        self.average = average
        self.params = [p for p in params if p.requires_grad]
        self.device = torch.device(device)
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.flat, self.in_place = flat, bool(in_place) and flat is not None
        if flat is not None and [id(p) for p in self.params] != [id(p) for p in flat.params]:
            raise ValueError("RaCoM(flat=...) must be given the parameters the FlatAdam owns, in its order")
        if self.in_place:
            self.bucket = flat.grad
        else:
            total = flat.total if flat is not None else sum(p.numel() for p in self.params)
            self.bucket = torch.zeros(total, dtype=torch.float32, device=self.device)
        self.stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None
        self._work = None
        self.bytes_reduced = 0

    def launch(self):
        with rng("racom-allreduce"):
            return self._launch()

    def _launch(self):
        if self.flat is not None:
            self.flat.gather_grads()                           # no launch when every gradient was written into its slot
            if not self.in_place:
                self.bucket.copy_(self.flat.grad)
            self._views = None
        else:
            views, off = [], 0
            for p in self.params:
                n = p.numel()
                g = p.grad if p.grad is not None else torch.zeros_like(p)
                views.append((p, off, n))
                self.bucket[off:off + n].copy_(g.reshape(-1))
                off += n
            self._views = views
        if self.world > 1 and self.average == "ddp":
            self.bucket.div_(self.world)
        if self.world > 1:
            self.bytes_reduced += self.bucket.numel() * 4
            if self.stream is not None:
                self.stream.wait_stream(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(self.stream):
                    self._work = dist.all_reduce(self.bucket, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
            else:
                self._work = dist.all_reduce(self.bucket, op=dist.ReduceOp.SUM, group=self.group, async_op=True)

    def wait(self):
        with rng("racom-allreduce"):
            return self._wait()

    def _wait(self):
        if self._work is not None:
            self._work.wait()
            self._work = None
        if self.stream is not None:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)
        if self.flat is not None:
            if self.in_place:
                self.flat.grad_scale = 1.0 / self.world if (self.world > 1 and self.average == "reference") else 1.0
                return
            if self.world > 1 and self.average == "reference":
                self.bucket.div_(self.world)
            self.flat.grad.copy_(self.bucket)
            self.flat.grad_scale = 1.0
            return
        if self.world > 1 and self.average == "reference":
            self.bucket.div_(self.world)                      # MQGCN.py:64
        for p, off, n in self._views:
            if p.grad is None:
                p.grad = torch.empty_like(p)
            p.grad.copy_(self.bucket[off:off + n].view_as(p))

    def all_reduce_and_wait(self):
        self.launch()
        self.wait()


def racom_sync_period(n_nodes, world, lo=2, hi=64):
    """RaCoM's "adaptive periodic synchronisation based on graph size and GPU count" (README.md:35) as a rule: replicas
    that apply gradients one step late drift apart at a rate that grows with the number of replicas and shrinks with the
    amount of data behind every gradient, so the full drain is scheduled every

        P = clamp( round( sqrt(n_nodes / 1e4) / world ), lo, hi )   steps

    -- a products-sized graph (2.4 M nodes) on 8 GPUs drains every 2 steps, on 2 GPUs every 8; a 134 M-node RMAT-27 on 8
    GPUs every 14; tiny graphs or many replicas fall back to `lo` (near-synchronous).  `staleness = 0` ignores the period
    and is the reference's actual, synchronous behaviour (MQGCN.py:55-79)."""
    p = int(round((max(int(n_nodes), 1) / 1e4) ** 0.5 / max(int(world), 1)))
    return max(lo, min(hi, p))


class RaCoMOptimizer:
    """RaCoM's "asynchronous gradient sharing with adaptive periodic synchronisation" (README.md:27,34-37) around any
    torch optimizer.  step() launches the bucket all-reduce of THIS step's gradients on the RaCoM stream and applies the
    gradients reduced `staleness` steps ago (a queue, as the reference's gradient_buffer Queue(maxsize=4),
    buffer_queues.py:76), so communication overlaps the next forward/backward; every `sync_every`-th step (and at
    flush()) the queue is drained so replicas re-converge.  staleness = 0 is the reference's actual (synchronous)
    behaviour, MQGCN.py:55-79, and equals DDP."""

    def __init__(self, optimizer, params, device, staleness=1, sync_every=8, group=None, average="reference"):
        from .optim import FlatAdam

        self.opt = optimizer
        self.flat = optimizer if isinstance(optimizer, FlatAdam) else None     # its gradient buffer moves with one copy each way
        self.average = average
        self.params = [p for p in params if p.requires_grad]
        self.device, self.group = torch.device(device), group
        self.staleness, self.sync_every = int(staleness), int(sync_every)
        self.pending = []      # RaCoM objects whose reduction is in flight, oldest first
        self.free = []
        self.steps = 0

    def _bucket(self):
        return self.free.pop() if self.free else RaCoM(self.params, self.device, self.group, average=self.average, flat=self.flat,
                                                       in_place=False)

    def _apply_oldest(self):
        r = self.pending.pop(0)
        r.wait()               # copies the averaged bucket into .grad
        self.opt.step()
        self.free.append(r)

    def step(self):
        self.steps += 1
        r = self._bucket()
        r.launch()
        self.pending.append(r)
        drain = self.staleness == 0 or (self.sync_every > 0 and self.steps % self.sync_every == 0)
        while self.pending and (drain or len(self.pending) > self.staleness):
            self._apply_oldest()

    def flush(self):
        while self.pending:
            self._apply_oldest()

    def zero_grad(self, set_to_none=False):
        self.opt.zero_grad(set_to_none=set_to_none)
