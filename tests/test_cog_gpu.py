"""CoG on the device: dgll_hip_louvain_move against the numpy restatement (tests/louvain_ref.py) bit for bit through all three
hash-table tiers, the eligibility rules one by one, whole `louvain` runs, and the users of the communities (reorder, partitioner,
CommunityBatchLoader, the example)."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import louvain_ref as lref
from conftest import load_golden
from dgll_amd import community, ops, partition
from dgll_amd.data import DGraph
from dgll_amd.graph import CSRGraph
from dgll_amd.sampling import CommunityBatchLoader

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIERS = [(community.WAVE_MAX_DEG, community.BLOCK_MAX_DEG), (4, 16), (0, 0)]      # defaults; small rows through every tier; all scratch


@pytest.fixture(scope="module")
def golden():
    return load_golden("cog_groups")


def _np_graph(golden, name):
    return golden["rowptr_" + name].astype(np.int64), golden["col_" + name].astype(np.int32)


def _graph(golden, name, dev):
    rowptr, col = _np_graph(golden, name)
    n = len(rowptr) - 1
    return CSRGraph(torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev), None, n, n)


def _sweep_both(dev, rowptr, col, w, k, size, comm, cap, seed=0, level=0, sweep=0, all_active=True, resolution=1.0, tiers=TIERS):
    """The restatement's targets, after checking that the device gives the same ones through every tier setting."""
    n = len(rowptr) - 1
    comm = np.asarray(comm, dtype=np.int32)
    tot, csize, cnt = lref.community_state(k, size, comm, n)
    two_m = int(k.sum())
    want = lref.move_targets(rowptr, col, w, k, size, comm, tot, csize, cnt, two_m, resolution, cap, seed, level, sweep, all_active)
    t = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)  # noqa: E731
    d = dict(rowptr=t(rowptr, torch.int64), col=t(col, torch.int32), w=t(w, torch.int64), k=t(k, torch.int64), size=t(size, torch.int64),
             comm=t(comm, torch.int32), tot=t(tot, torch.int64), csize=t(csize, torch.int64), cnt=t(cnt, torch.int32))
    for wave_max, block_max in tiers:
        got, movers = community.move_targets(d["rowptr"], d["col"], d["w"], d["k"], d["size"], d["comm"], d["tot"], d["csize"], d["cnt"],
                                             two_m, resolution, cap, seed, level, sweep, all_active, wave_max_deg=wave_max,
                                             block_max_deg=block_max, return_info=True)
        got = got.cpu().numpy()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "tiers (%d, %d): %d rows differ, first %s: device %s, restatement %s" % (
            wave_max, block_max, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])
        assert movers == int((want != comm).sum())
    return want


def test_one_sweep_graph_a_level_0(cuda_device, golden):
    rowptr, col = _np_graph(golden, "A")
    n = len(rowptr) - 1
    k, size = np.diff(rowptr).astype(np.int64), np.ones(n, np.int64)
    comm = np.arange(n, dtype=np.int32)
    for sweep in range(3):                                                          # singletons, then two states in mid-run
        target = _sweep_both(cuda_device, rowptr, col, None, k, size, comm, cap=64, seed=0, sweep=sweep, all_active=False)
        assert (target != comm).sum() > 0
        tot, csize, cnt = lref.community_state(k, size, comm, n)
        movers, t = lref.admit(comm, target, size, csize, 64)
        comm[movers] = t


def _tiers_graph():
    """Directed CSR of 6000 nodes with rows of every length at which the kernel takes another path, a 2000-entry row whose neighbours
    sit in 2000 distinct communities (worst table load) and one whose neighbours share one community."""
    rng = np.random.RandomState(5)
    n = 6000
    lengths = [0, 1, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 3, 4, 5, 15, 16, 17]
    rows = [np.sort(rng.choice(n, size=L, replace=False)) for L in lengths]
    rows += [np.zeros(0, np.int64)] * (20 - len(rows))
    rows.append(np.arange(3000, 5000))                                              # node 20: all distinct
    rows.append(np.arange(1000, 3000))                                              # node 21: one community
    rows += [np.sort(rng.choice(n, size=rng.randint(0, 13), replace=False)) for _ in range(n - len(rows))]
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rowptr[1:])
    col = np.concatenate(rows).astype(np.int32)
    comm = np.arange(n, dtype=np.int32)
    comm[:1000] = rng.randint(0, 1000, size=1000)
    comm[1000:3000] = 1000
    return rowptr, col, comm, lengths


def test_one_sweep_every_tier_and_row_length(cuda_device):
    rowptr, col, comm, lengths = _tiers_graph()
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    assert deg[:len(lengths)].tolist() == lengths and deg[20] == 2000 and deg[21] == 2000
    for wave_max, block_max in TIERS:                                               # threshold and threshold +- 1 are present
        assert {wave_max, wave_max + 1, block_max, block_max + 1} <= set(deg.tolist()) | {0}
    k, size = np.maximum(deg, 1).astype(np.int64), np.ones(n, np.int64)
    free = _sweep_both(cuda_device, rowptr, col, None, k, size, comm, cap=n, seed=9, level=1, sweep=2, all_active=True)
    full = _sweep_both(cuda_device, rowptr, col, None, k, size, comm, cap=1500, seed=9, level=1, sweep=2, all_active=True)
    half = _sweep_both(cuda_device, rowptr, col, None, k, size, comm, cap=1500, seed=9, level=1, sweep=2, all_active=False)
    assert min((free != comm).sum(), (full != comm).sum(), (half != comm).sum()) > 100
    assert free[21] == 1000 and full[21] == comm[21]                                # community 1000 holds 2000 nodes: over the cap


def test_one_sweep_coarse_level_with_int64_weights(cuda_device):
    """A hand-built coarse level: int64 weights above 2^31, self-loop entries, node 6 isolated, node 5 an empty row others point to."""
    big = 1 << 33
    rows = {0: [(0, 5 * big), (1, big + 3), (2, 7), (5, 2)], 1: [(0, big + 3), (1, 9), (3, big + 1)], 2: [(0, 7), (2, 4 * big), (4, 11)],
            3: [(1, big + 1), (3, 1), (4, big)], 4: [(2, 11), (3, big), (4, 6), (5, 1)], 5: [], 6: [], 7: [(7, 3)]}
    n = 8
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum([len(rows[v]) for v in range(n)], out=rowptr[1:])
    col = np.array([c for v in range(n) for c, _ in rows[v]], dtype=np.int32)
    w = np.array([x for v in range(n) for _, x in rows[v]], dtype=np.int64)
    k = np.array([sum(x for _, x in rows[v]) for v in range(n)], dtype=np.int64)
    k[5] = 3                                                                        # its in-weight: the level's k is symmetric
    size = np.array([40, 25, 30, 10, 12, 1, 1, 2], dtype=np.int64)
    moved = 0
    for comm in (np.arange(n), np.array([0, 0, 2, 3, 3, 5, 6, 7])):
        for cap in (121, 60):
            for res in (1.0, 0.5):
                target = _sweep_both(cuda_device, rowptr, col, w, k, size, comm, cap=cap, level=2, sweep=1, resolution=res)
                assert target[6] == comm[6] and target[5] == comm[5] and target[7] == comm[7]
                moved += int((target != comm).sum())
    assert moved > 0


def _simple(edges, n):
    rows = [[] for _ in range(n)]
    for a, b in edges:
        rows[a].append(b)
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rowptr[1:])
    return rowptr, np.array([c for r in rows for c in r], dtype=np.int32)


def test_singleton_rule(cuda_device):
    ones = lambda n: np.ones(n, np.int64)  # noqa: E731
    rowptr, col = _simple([(0, 1), (1, 0)], 2)                                      # two nodes: only the larger id moves
    target = _sweep_both(cuda_device, rowptr, col, None, np.diff(rowptr), ones(2), np.arange(2), cap=2)
    assert target.tolist() == [0, 0]
    rowptr, col = _simple([(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2)], 4)      # a path: everybody looks down, nobody swaps
    target = _sweep_both(cuda_device, rowptr, col, None, np.diff(rowptr), ones(4), np.arange(4), cap=4)
    assert target.tolist() == [0, 0, 1, 2]
    # a community of two is no singleton: node 0 (alone) may join the larger id
    rowptr, col = _simple([(0, 1), (1, 0), (1, 2), (2, 1)], 3)
    target = _sweep_both(cuda_device, rowptr, col, None, np.diff(rowptr), ones(3), np.array([0, 2, 2]), cap=3)
    assert target.tolist() == [2, 2, 2]


def test_tie_goes_to_the_smaller_id_and_the_cap_filters(cuda_device):
    rowptr, col = _simple([(2, 1), (2, 0), (0, 2), (1, 2)], 3)                      # node 2 sees 1 first, then 0: equal gains
    k = np.diff(rowptr).astype(np.int64)
    target = _sweep_both(cuda_device, rowptr, col, None, k, np.ones(3, np.int64), np.arange(3), cap=3)
    assert target[2] == 0
    target = _sweep_both(cuda_device, rowptr, col, None, k, np.array([5, 1, 1], dtype=np.int64), np.arange(3), cap=5)
    assert target[2] == 1                                                           # community 0 is full


def test_inactive_half_keeps_its_community(cuda_device, golden):
    rowptr, col = _np_graph(golden, "A")
    n = len(rowptr) - 1
    comm = np.arange(n, dtype=np.int32)
    k, size = np.diff(rowptr).astype(np.int64), np.ones(n, np.int64)
    half = _sweep_both(cuda_device, rowptr, col, None, k, size, comm, cap=n, seed=4, sweep=1, all_active=False, tiers=TIERS[:1])
    full = _sweep_both(cuda_device, rowptr, col, None, k, size, comm, cap=n, seed=4, sweep=1, all_active=True, tiers=TIERS[:1])
    active = lref.active_mask(n, 4, 0, 1, False)
    assert 0.4 * n < active.sum() < 0.6 * n
    assert np.array_equal(half[~active], comm[~active]) and np.array_equal(half[active], full[active])
    assert (full[~active] != comm[~active]).any()


@pytest.fixture(scope="module")
def whole_runs(golden):
    """The restatement's labels, computed once: (graph, cap) -> labels."""
    out = {}
    for name in "AB":
        rowptr, col = _np_graph(golden, name)
        for cap in (None, 64):
            out[name, cap] = lref.louvain(rowptr, col, max_comm_size=cap, seed=0)
    return out


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("cap", [None, 64])
def test_whole_run_equals_the_restatement(cuda_device, golden, whole_runs, name, cap):
    g = _graph(golden, name, cuda_device)
    worst = [0]

    def check(level, sweep, comm, size):
        worst[0] = max(worst[0], int(torch.zeros(comm.numel(), dtype=torch.int64, device=comm.device).index_add_(0, comm.long(), size).max()))

    labels = community.louvain(g, max_comm_size=cap, seed=0, on_sweep=check)
    assert labels.dtype == torch.int64 and labels.device == g.device
    assert np.array_equal(labels.cpu().numpy(), whole_runs[name, cap])
    assert worst[0] <= (cap or g.n_rows) and int(torch.bincount(labels).max()) <= (cap or g.n_rows)
    assert torch.equal(community.louvain(g, max_comm_size=cap, seed=0), labels)            # a second call
    q = community.modularity(g, labels)
    assert abs(q - lref.modularity(*_np_graph(golden, name), whole_runs[name, cap])) < 1e-12
    if cap is None:
        assert q >= 0.98 * float(golden["nx_modularity_" + name].min())


def test_whole_run_in_a_fresh_process(cuda_device, whole_runs):
    code = ("import sys, hashlib, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from conftest import load_golden; from dgll_amd import community; from dgll_amd.graph import CSRGraph\n"
            "g = load_golden('cog_groups'); n = len(g['rowptr_A']) - 1\n"
            "graph = CSRGraph(g.t('rowptr_A', 'cuda:0', torch.int64), g.t('col_A', 'cuda:0', torch.int32), None, n, n)\n"
            "print('sha', hashlib.sha256(community.louvain(graph, max_comm_size=64, seed=0).cpu().numpy().tobytes()).hexdigest())\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    assert re.search(r"sha (\w+)", res.stdout).group(1) == hashlib.sha256(whole_runs["A", 64].astype(np.int64).tobytes()).hexdigest()


def test_reorder_with_louvain(cuda_device, golden):
    g = _graph(golden, "A", cuda_device)
    g2, perm = g.reorder(method="louvain", max_comm_size=64, seed=0)
    n = g.n_rows
    assert sorted(perm.tolist()) == list(range(n))
    labels = community.louvain(g, max_comm_size=64, seed=0)[perm]                          # communities are contiguous ranges
    change = int((labels[1:] != labels[:-1]).sum())
    assert change + 1 == int(labels.unique().numel())
    x = torch.randn(n, 16, device=cuda_device)
    y = ops.spmm(g, x)
    y2 = ops.spmm(g2, g2.to_engine_order(x))
    torch.testing.assert_close(g2.to_caller_order(y2), y, rtol=1e-5, atol=1e-5)


def test_community_batch_loader(cuda_device, golden):
    g = _graph(golden, "B", cuda_device)
    n = g.n_rows
    feats = torch.arange(n, dtype=torch.float32, device=cuda_device).unsqueeze(1).repeat(1, 3)
    labels = torch.arange(n, device=cuda_device) % 7
    loader = CommunityBatchLoader(g, feats, labels, 500, max_comm_size=200)
    rowptr, col = _np_graph(golden, "B")
    dg = DGraph.from_csr(rowptr, col.astype(np.int64))
    perm = loader.book.perm.cpu()
    at, seen = 0, 0
    for (start, end), sub, x, y in loader:
        assert start == at and end > start                                           # the ranges tile [0, n)
        assert end - start >= 500 or end == n
        at = end
        nodes = perm[start:end]
        assert torch.equal(x[:, 0].cpu().long(), nodes) and torch.equal(y.cpu(), nodes % 7)
        want = dg.get_induced_subgraph(nodes)
        dense = torch.zeros(end - start, end - start, dtype=torch.int32)
        dense[sub.row_index().cpu(), sub.col.long().cpu()] = 1
        assert sub.nnz == int(want.sum()) and torch.equal(dense, want)               # entry for entry (no duplicates: nnz matches)
        sums = torch.zeros(end - start, device=cuda_device).index_add_(0, sub.row_index(), sub.val)
        filled = sub.degrees() > 0
        torch.testing.assert_close(sums[filled], torch.ones(int(filled.sum()), device=cuda_device), rtol=1e-6, atol=1e-6)
        assert float(sums[~filled].abs().sum()) == 0.0
        seen += 1
    assert at == n and seen == len(loader) >= 2
    raw = CommunityBatchLoader(loader.book, None, None, 500, normalize=None, graph=loader.graph)
    assert raw.batch(0)[1].val is None and raw.batch(0)[1].nnz == loader.batch(0)[1].nnz
    comm = loader.book.community                                                     # a group is a run of whole communities
    for start, end in loader.book.group_ranges.tolist()[:-1]:
        assert int(comm[end - 1]) != int(comm[end])
    assert int(torch.bincount(comm).max()) <= 200


def test_community_parts_with_louvain(cuda_device, golden):
    g = _graph(golden, "B", cuda_device)
    part = partition.community_parts(g, 4, method="louvain", max_comm_size=200)
    assert part.shape == (g.n_rows,) and sorted(part.unique().tolist()) == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="method"):
        partition.community_parts(g, 4, method="metis")


def test_cog_example(cuda_device):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cog", "train.py"), "--nodes", "20000", "--batch", "2500",
                          "--max-comm-size", "1000", "--epochs", "4"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    loss = [float(v) for v in re.findall(r"loss ([0-9.]+)", res.stdout)]
    q = float(re.search(r"modularity ([0-9.]+)", res.stdout).group(1))
    assert len(loss) == 4 and loss[-1] < loss[0] and q > 0.3, res.stdout


def test_error_paths(cuda_device, golden):
    rowptr = torch.tensor([0, 2, 3, 4, 5], dtype=torch.int64, device=cuda_device)
    col = torch.tensor([1, 7, 0, 3, 2], dtype=torch.int32, device=cuda_device)        # 7 is no node of a 4-node graph
    g = CSRGraph(rowptr, col, None, 4, 4)
    with pytest.raises(ValueError, match="column id outside"):
        community.louvain(g)
    good = _graph(golden, "A", cuda_device)
    with pytest.raises(ValueError, match="max_comm_size"):
        community.louvain(good, max_comm_size=0)
    with pytest.raises(RuntimeError, match="GPU only"):
        community.louvain(good.to("cpu"))
    assert community.louvain(CSRGraph(torch.zeros(4, dtype=torch.int64, device=cuda_device),
                                      torch.zeros(0, dtype=torch.int32, device=cuda_device), None, 3, 3)).tolist() == [0, 1, 2]
