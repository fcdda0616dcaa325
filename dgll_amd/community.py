"""CoG / CommGNN on the device: modularity communities with a maximum size, merged into groups of at least a batch, relabelled so
that every group is a contiguous id range (the reference's `GPU Accelerator/cog.py:84-86, 64-77, 31-45`, which calls leidenalg on
the host).

`louvain` is Louvain local moving with a size cap, level by level:

  * a sweep is synchronous and semi-active -- every active node (a Philox-seeded half, all of them in the last allowed sweep)
    names the neighbouring community with the largest modularity gain that still has room for it; the gather-reduce over the CSR
    is dgll_amd/csrc/louvain.hip (`dgll_hip_louvain_move`), everything else here is torch on the graph's device;
  * admission: the movers are sorted by (target, node id) and admitted while the target's size at the start of the sweep plus the
    running sum of the admitted sizes stays within the cap (room freed by leavers in the same sweep is not counted), so no community
    exceeds the cap after any sweep;
  * `tot`, `csize`, `cnt` are recomputed with integer index_add_, the coarse graph with a sort and segment sums: two runs with one
    seed give the same labels, and tests/louvain_ref.py restates the whole scheme in numpy with the same bits.

`leiden` is what the reference calls: after the local moving of a level, a refinement phase splits every community into connected,
well-connected sub-communities (synchronous sweeps in which only singletons move and a sub-community that is somebody's target
keeps its members; `dgll_hip_leiden_refine` in the same file), the level is aggregated on the sub-communities, and the next level
starts from the communities carried onto them.  Every community it returns is connected; `louvain`'s may fall into pieces.
tests/leiden_ref.py restates it with the same bits.

Differences from the reference: the refinement merges greedily (largest gain, ties to the smallest id)
where leidenalg draws at random, and `louvain` has no refinement at all; synchronous half-sweeps; a conservative cap;
structure-only weights (every stored entry counts 1, `val` is ignored, as the reference builds its igraph from the edge list).
"""
import torch

from . import _lib
from .graph import CSRGraph

WAVE_MAX_DEG = 128       # rows up to this many entries: one wavefront, a 256-slot table in its LDS (csrc/louvain.hip)
BLOCK_MAX_DEG = 2048     # up to this many: one workgroup, a 4096-slot LDS table; longer rows use the global scratch
_LARGE_NNZ = 1 << 30
_ERRORS = {1: "a column id outside [0, N)", 2: "the scratch table is too small", 4: "a row with 2^30 or more entries or bad row pointers",
           8: "a community id outside [0, N)", 16: "a bound community id outside [0, N)"}


def _square(graph):
    if not isinstance(graph, CSRGraph):
        raise TypeError("graph must be a CSRGraph, got %r" % type(graph))
    if graph.n_rows != graph.n_cols:
        raise ValueError("communities need a square adjacency")
    return graph


def _next_pow2(x):
    """Elementwise smallest power of two >= x (int64, x >= 1)."""
    p = torch.ones_like(x)
    for _ in range(32):
        p = torch.where(p < x, p * 2, p)
    return p


def community_state(k, size, comm, n):
    """(tot, csize, cnt): per community the sum of k, of size, and the member count -- integer adds, order-independent."""
    c = comm.long()
    tot = torch.zeros(n, dtype=torch.int64, device=k.device).index_add_(0, c, k)
    csize = torch.zeros(n, dtype=torch.int64, device=k.device).index_add_(0, c, size)
    return tot, csize, torch.bincount(c, minlength=n).to(torch.int32)


def move_targets(rowptr, col, w, k, size, comm, tot, csize, cnt, two_m, resolution, cap, seed, level, sweep, all_active,
                 wave_max_deg=WAVE_MAX_DEG, block_max_deg=BLOCK_MAX_DEG, return_info=False):
    """One sweep of dgll_hip_louvain_move: int32 [n] targets.  Raises ValueError on the kernel's error bits."""
    if not rowptr.is_cuda:
        raise RuntimeError("dgll_amd.community runs on the GPU only (got a %s graph); there is no CPU fallback" % rowptr.device)
    dev = rowptr.device
    n = rowptr.numel() - 1
    if not 0 < int(two_m) < 2 ** 53:
        raise ValueError("the total weight must lie in [1, 2^53): the modularity gains are exact float64 only below it")
    if int(cap) < 1:
        raise ValueError("max_comm_size must be >= 1")
    scratch, nbytes = _scratch(rowptr, wave_max_deg, block_max_deg)
    target = torch.empty(n, dtype=torch.int32, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    _lib.launch("dgll_hip_louvain_move", dev, rowptr.data_ptr(), _lib.ptr(col), _lib.ptr(w), k.data_ptr(), size.data_ptr(),
                comm.data_ptr(), tot.data_ptr(), csize.data_ptr(), cnt.data_ptr(), n, int(col.numel()), int(two_m), float(resolution),
                int(cap), int(seed) & 0xFFFFFFFFFFFFFFFF, int(level), int(sweep), int(bool(all_active)), int(wave_max_deg),
                int(block_max_deg), scratch.data_ptr(), nbytes, target.data_ptr(), info.data_ptr())
    want, err = info.cpu().tolist()           # the sweep's one blocking read
    if err:
        raise ValueError("louvain: " + ", ".join(m for bit, m in _ERRORS.items() if err & bit))
    return (target, want) if return_info else target


def _scratch(rowptr, wave_max_deg, block_max_deg):
    """(int64 tensor, bytes): the sweep kernels' scratch, with tables for every row longer than the workgroup tier."""
    n = rowptr.numel() - 1
    deg = rowptr[1:] - rowptr[:-1]
    long_deg = deg[deg > max(int(block_max_deg), int(wave_max_deg))]
    long_slots = int((2 * _next_pow2(long_deg)).sum()) if long_deg.numel() else 0
    nbytes = int(_lib.lib.dgll_hip_louvain_scratch_bytes(n, long_slots))
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=rowptr.device), nbytes


def refine_targets(rowptr, col, w, k, size, sub, bound, tot, csize, cnt, totP, two_m, resolution, cap, wave_max_deg=WAVE_MAX_DEG,
                   block_max_deg=BLOCK_MAX_DEG, return_info=False):
    """One sweep of dgll_hip_leiden_refine: (target int32 [n], wS, wC, cut int64 [n]) -- where every singleton of `sub` that is well
    connected to its community in `bound` would go, every node's weight into its own sub-community and into its bound community,
    and every sub-community's weight to the rest of its bound community.  Raises ValueError on the kernel's error bits."""
    if not rowptr.is_cuda:
        raise RuntimeError("dgll_amd.community runs on the GPU only (got a %s graph); there is no CPU fallback" % rowptr.device)
    dev = rowptr.device
    n = rowptr.numel() - 1
    if not 0 < int(two_m) < 2 ** 53:
        raise ValueError("the total weight must lie in [1, 2^53): the modularity gains are exact float64 only below it")
    if int(cap) < 1:
        raise ValueError("max_comm_size must be >= 1")
    scratch, nbytes = _scratch(rowptr, wave_max_deg, block_max_deg)
    target = torch.empty(n, dtype=torch.int32, device=dev)
    wS, wC, cut = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    _lib.launch("dgll_hip_leiden_refine", dev, rowptr.data_ptr(), _lib.ptr(col), _lib.ptr(w), k.data_ptr(), size.data_ptr(),
                sub.data_ptr(), bound.data_ptr(), tot.data_ptr(), csize.data_ptr(), cnt.data_ptr(), totP.data_ptr(), n, int(col.numel()),
                int(two_m), float(resolution), int(cap), int(wave_max_deg), int(block_max_deg), scratch.data_ptr(), nbytes,
                target.data_ptr(), wS.data_ptr(), wC.data_ptr(), cut.data_ptr(), info.data_ptr())
    want, err = info.cpu().tolist()           # the sweep's one blocking read
    if err:
        raise ValueError("leiden: " + ", ".join(m for bit, m in _ERRORS.items() if err & bit))
    return (target, wS, wC, cut, want) if return_info else (target, wS, wC, cut)


def admit(comm, target, size, csize, cap):
    """(movers, targets): the nodes whose target differs, in (target, node id) order, admitted while the target's start-of-sweep size
    plus the running sum of admitted sizes stays within cap."""
    movers = torch.nonzero(target != comm).flatten()
    t = target[movers].long()
    t, order = torch.sort(t, stable=True)
    movers = movers[order]
    if movers.numel() == 0:
        return movers, t
    run = torch.cumsum(size[movers], 0)
    head = torch.ones_like(t, dtype=torch.bool)
    head[1:] = t[1:] != t[:-1]
    start = torch.nonzero(head).flatten()
    seg = torch.cumsum(head.long(), 0) - 1
    base = torch.where(start > 0, run[(start - 1).clamp(min=0)], torch.zeros_like(start))
    ok = csize[t] + (run - base[seg]) <= cap
    return movers[ok], t[ok]


def _aggregate(rowptr, col, w, dense, nc):
    """Coarse CSR of a level: (community of row, community of col) coalesced with int64 weight sums by a sort and segment sums;
    the weight inside a community becomes its self-loop entry."""
    if col.numel() >= _LARGE_NNZ:
        raise NotImplementedError("louvain: the aggregation step sorts the whole entry list; 2^30 or more entries are not supported")
    n = rowptr.numel() - 1
    dev = rowptr.device
    row = torch.repeat_interleave(torch.arange(n, device=dev), rowptr[1:] - rowptr[:-1])
    key = dense[row] * nc + dense[col.long()]
    del row
    if w is None:
        key, _ = torch.sort(key)
        key, ws = torch.unique_consecutive(key, return_counts=True)
    else:
        key, order = torch.sort(key, stable=True)
        w = w[order]
        key, inverse = torch.unique_consecutive(key, return_inverse=True)
        ws = torch.zeros(key.numel(), dtype=torch.int64, device=dev).index_add_(0, inverse, w)
    cr = torch.div(key, nc, rounding_mode="floor")
    ptr = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(cr, minlength=nc), 0, out=ptr[1:])
    return ptr, (key - cr * nc).to(torch.int32), ws.contiguous()


def louvain(graph, max_comm_size=None, resolution=1.0, seed=0, max_levels=10, max_sweeps=32, on_sweep=None):
    """int64 [n] dense community labels of a square CSRGraph on the GPU: size-capped Louvain (module docstring).  max_comm_size=None
    means n.  on_sweep(level, sweep, comm, size): called after every sweep's admission (tests, tools)."""
    graph = _square(graph)
    if not graph.is_cuda:
        raise RuntimeError("dgll_amd.community runs on the GPU only (got a %s graph); there is no CPU fallback" % graph.device)
    n = graph.n_rows
    cap = n if max_comm_size is None else int(max_comm_size)
    if cap < 1:
        raise ValueError("max_comm_size must be >= 1")
    if max_levels < 1 or max_sweeps < 1:
        raise ValueError("max_levels and max_sweeps must be >= 1")
    dev = graph.device
    labels = torch.arange(n, dtype=torch.int64, device=dev)
    if graph.nnz == 0 or n == 0:
        return labels
    rowptr, col, w = graph.rowptr, graph.col, None
    k, size = graph.degrees().contiguous(), torch.ones(n, dtype=torch.int64, device=dev)
    two_m = graph.nnz
    for level in range(max_levels):
        nl = rowptr.numel() - 1
        comm = torch.arange(nl, dtype=torch.int32, device=dev)
        for sweep in range(max_sweeps):
            tot, csize, cnt = community_state(k, size, comm, nl)
            target = move_targets(rowptr, col, w, k, size, comm, tot, csize, cnt, two_m, resolution, cap, seed, level, sweep,
                                  sweep == max_sweeps - 1)
            movers, t = admit(comm, target, size, csize, cap)
            comm[movers] = t.to(torch.int32)
            if on_sweep is not None:
                on_sweep(level, sweep, comm, size)
            if sweep >= 2 and movers.numel() < max(nl // 1000, 1):
                break
        uniq, dense = torch.unique(comm, return_inverse=True)
        if uniq.numel() == nl:
            break
        labels = dense[labels]
        rowptr, col, w = _aggregate(rowptr, col, w, dense, uniq.numel())
        k = torch.zeros(uniq.numel(), dtype=torch.int64, device=dev).index_add_(0, dense, k)
        size = torch.zeros(uniq.numel(), dtype=torch.int64, device=dev).index_add_(0, dense, size)
    return labels


def refine(rowptr, col, w, k, size, bound, two_m, resolution, cap, max_sweeps=32, level=0, on_refine=None,
           wave_max_deg=WAVE_MAX_DEG, block_max_deg=BLOCK_MAX_DEG):
    """int32 [n]: Leiden's sub-communities of a level, from singletons.  Sweeps until one admits nobody (at most max_sweeps): only
    singletons move, a would-be mover that is itself somebody's target stays, then `admit` keeps the cap.  A sub-community's
    members at the start of a sweep therefore never leave it and every joiner is adjacent to one of them: it stays connected."""
    n = rowptr.numel() - 1
    dev = rowptr.device
    sub = torch.arange(n, dtype=torch.int32, device=dev)
    totP = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, bound.long(), k)
    for sweep in range(max_sweeps):
        tot, csize, cnt = community_state(k, size, sub, n)
        target, _, _, _, want = refine_targets(rowptr, col, w, k, size, sub, bound, tot, csize, cnt, totP, two_m, resolution, cap,
                                               wave_max_deg, block_max_deg, return_info=True)
        moved = 0
        if want:
            wants = target != sub
            aimed = torch.zeros(n, dtype=torch.bool, device=dev)
            aimed[target[wants].long()] = True
            target = torch.where(wants & ~aimed[sub.long()], target, sub)
            movers, t = admit(sub, target, size, csize, cap)
            sub[movers] = t.to(torch.int32)
            moved = movers.numel()
        if on_refine is not None:
            on_refine(level, sweep, sub, bound, size)
        if moved == 0:
            break
    return sub


def leiden(graph, max_comm_size=None, resolution=1.0, seed=0, max_levels=20, max_sweeps=32, on_sweep=None, on_refine=None):
    """int64 [n] dense community labels of a square CSRGraph on the GPU: size-capped Leiden (module docstring); every community is
    connected.  max_comm_size=None means n.  max_levels=20: a level shrinks the node count by the refinement's merges only (about
    3x on the test graphs), and 3^20 exceeds the 2^31 nodes the kernels accept.  on_sweep(level, sweep, comm, size): after every
    local-moving sweep's admission; on_refine(level, sweep, sub, bound, size): after every refinement sweep's."""
    graph = _square(graph)
    if not graph.is_cuda:
        raise RuntimeError("dgll_amd.community runs on the GPU only (got a %s graph); there is no CPU fallback" % graph.device)
    n = graph.n_rows
    cap = n if max_comm_size is None else int(max_comm_size)
    if cap < 1:
        raise ValueError("max_comm_size must be >= 1")
    if max_levels < 1 or max_sweeps < 1:
        raise ValueError("max_levels and max_sweeps must be >= 1")
    dev = graph.device
    labels = torch.arange(n, dtype=torch.int64, device=dev)
    if graph.nnz == 0 or n == 0:
        return labels
    rowptr, col, w = graph.rowptr, graph.col, None
    k, size = graph.degrees().contiguous(), torch.ones(n, dtype=torch.int64, device=dev)
    two_m = graph.nnz
    comm = torch.arange(n, dtype=torch.int32, device=dev)
    for level in range(max_levels):
        nl = rowptr.numel() - 1
        for sweep in range(max_sweeps):
            tot, csize, cnt = community_state(k, size, comm, nl)
            target = move_targets(rowptr, col, w, k, size, comm, tot, csize, cnt, two_m, resolution, cap, seed, level, sweep,
                                  sweep == max_sweeps - 1)
            movers, t = admit(comm, target, size, csize, cap)
            comm[movers] = t.to(torch.int32)
            if on_sweep is not None:
                on_sweep(level, sweep, comm, size)
            if sweep >= 2 and movers.numel() < max(nl // 1000, 1):
                break
        uniq, dense = torch.unique(comm, return_inverse=True)
        if uniq.numel() == nl:                     # every community is one supernode: a refined sub-community, so connected
            return dense[labels]
        sub = refine(rowptr, col, w, k, size, comm, two_m, resolution, cap, max_sweeps, level, on_refine)
        usub, dsub = torch.unique(sub, return_inverse=True)
        labels = dsub[labels]
        if usub.numel() == nl or level == max_levels - 1:
            return labels                          # the refined partition: connected whichever way the loop ends
        comm = torch.zeros(usub.numel(), dtype=torch.int32, device=dev)
        comm[dsub] = dense.to(torch.int32)         # the communities carried onto the supernodes
        rowptr, col, w = _aggregate(rowptr, col, w, dsub, usub.numel())
        k = torch.zeros(usub.numel(), dtype=torch.int64, device=dev).index_add_(0, dsub, k)
        size = torch.zeros(usub.numel(), dtype=torch.int64, device=dev).index_add_(0, dsub, size)
    return labels


def modularity(graph, labels, resolution=1.0):
    """float: sum over communities of  inside_c / 2m - resolution (tot_c / 2m)^2  with every stored entry counting 1 (2m = nnz;
    for a symmetric CSR this is the undirected modularity).  float64 torch ops on the graph's device, CPU or GPU."""
    graph = _square(graph)
    if graph.nnz == 0:
        return 0.0
    lab = labels.to(graph.device).long()
    inside = (lab[graph.row_index()] == lab[graph.col.long()]).sum().double()
    nc = int(lab.max()) + 1
    tot = torch.zeros(nc, dtype=torch.float64, device=graph.device).index_add_(0, lab, graph.degrees().double())
    two_m = float(graph.nnz)
    return float(inside / two_m - resolution * (tot * tot).sum() / (two_m * two_m))


# ---- groups: cog.py:64-77 (merge) and :31-45 (relabel), on arrays ---------------------------------------------------------------
def _as_groups(groups_or_labels):
    """(nodes int64 [n], ptr int64 [g + 1]) for a list of id sequences (kept in the order given), a (nodes, ptr) pair, or a label
    vector (communities in label order, members by ascending id)."""
    x = groups_or_labels
    if isinstance(x, tuple) and len(x) == 2 and isinstance(x[0], torch.Tensor):
        return x[0].long(), x[1].long()
    if isinstance(x, torch.Tensor):
        if x.dim() != 1:
            raise ValueError("a label vector must be 1-D")
        lab = x.long()
        nodes = torch.sort(lab, stable=True)[1]
        counts = torch.bincount(lab) if lab.numel() else torch.zeros(0, dtype=torch.int64, device=lab.device)
        ptr = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=lab.device)
        torch.cumsum(counts, 0, out=ptr[1:])
        return nodes, ptr
    parts = [torch.as_tensor(g, dtype=torch.int64).reshape(-1) for g in x]
    ptr = torch.zeros(len(parts) + 1, dtype=torch.int64)
    if parts:
        torch.cumsum(torch.tensor([p.numel() for p in parts], dtype=torch.int64), 0, out=ptr[1:])
    nodes = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64)
    return nodes, ptr


def merge_groups(groups_or_labels, batch_size):
    """Communities, in the order given, merged into groups: a group closes once it holds >= batch_size nodes, the remainder forms a
    last group.  Returns (nodes, group_ptr): the node ids in group order and the groups' boundaries in that list."""
    nodes, ptr = _as_groups(groups_or_labels)
    ends = ptr[1:].tolist()
    bounds, opened = [0], 0
    for e in ends:                                 # one pass over the communities' sizes (host: a running threshold)
        if e - opened >= batch_size and e > opened:
            bounds.append(e)
            opened = e
    if ends and ends[-1] > opened:
        bounds.append(ends[-1])
    return nodes, torch.tensor(bounds, dtype=torch.int64, device=nodes.device)


def relabel_groups(groups):
    """New ids consecutive in group order: (perm, inv_perm, ranges) with perm[new] = old, inv_perm[old] = new and ranges int64 [g, 2]
    the groups' [start, end) in new ids.  `groups`: what merge_groups returns (or anything it accepts)."""
    nodes, ptr = _as_groups(groups)
    n = nodes.numel()
    inv = torch.full((int(nodes.max()) + 1 if n else 0,), -1, dtype=torch.int64, device=nodes.device)
    inv[nodes] = torch.arange(n, device=nodes.device)
    if n and (int((inv >= 0).sum()) != n or inv.numel() != n):
        raise ValueError("the groups must list every node id in [0, n) exactly once")
    keep = ptr[1:] > ptr[:-1]
    return nodes, inv, torch.stack([ptr[:-1][keep], ptr[1:][keep]], 1)


class CommunityBook:
    """What cog_order found: `perm` (new row i = old node perm[i]), `inv_perm`, `community` (int64 [n]: the community of every NEW
    id; communities are numbered in new-id order), `community_ranges` and `group_ranges` (int64 [c, 2] / [g, 2], [start, end) in new
    ids).  Every group is a run of whole communities."""

    def __init__(self, perm, inv_perm, community, community_ranges, group_ranges):
        self.perm, self.inv_perm, self.community = perm, inv_perm, community
        self.community_ranges, self.group_ranges = community_ranges, group_ranges

    @property
    def n_groups(self):
        return int(self.group_ranges.shape[0])

    def relabel(self, graph):
        """The graph in the book's id space (reorder.relabel: rows and columns, columns ascending; `perm` / `inv_perm` attached)."""
        from . import reorder

        return reorder.relabel(graph, self.perm.to(graph.device))


def order_by_labels(labels, deg):
    """(perm, dense): communities largest first, inside a community hubs first, then old id -- the order reorder.locality_order
    uses; dense[v] = rank of v's community."""
    n = labels.numel()
    _, dense, csz = torch.unique(labels, return_inverse=True, return_counts=True)
    rank = torch.empty_like(csz)
    rank[torch.argsort(csz, descending=True, stable=True)] = torch.arange(csz.numel(), device=csz.device)
    dense = rank[dense]
    dmax = int(deg.max()) + 1 if n else 1
    order = torch.argsort((dmax - 1 - deg) * n + torch.arange(n, device=deg.device))
    return order[torch.argsort(dense[order], stable=True)], dense


def cog_order(graph, batch_size, max_comm_size=None, method="louvain", **kw):
    """CoG's preprocessing in one call: `louvain` (the default) or `leiden` communities (capped at max_comm_size; **kw goes to the
    method), ordered largest first (hubs first inside), merged into groups of >= batch_size nodes, relabelled contiguously.
    Returns a CommunityBook."""
    graph = _square(graph)
    if method not in ("louvain", "leiden"):
        raise ValueError("cog_order method must be 'louvain' or 'leiden'")
    if int(batch_size) < 1:
        raise ValueError("batch_size must be >= 1")
    labels = (leiden if method == "leiden" else louvain)(graph, max_comm_size=max_comm_size, **kw)
    order, dense = order_by_labels(labels, graph.degrees())
    counts = torch.bincount(dense)
    cptr = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=order.device)
    torch.cumsum(counts, 0, out=cptr[1:])
    nodes, gptr = merge_groups((order, cptr), batch_size)
    perm, inv, granges = relabel_groups((nodes, gptr))
    return CommunityBook(perm, inv, dense[perm], torch.stack([cptr[:-1], cptr[1:]], 1), granges)
