"""Leiden on the device: dgll_hip_leiden_refine against the numpy restatement (tests/leiden_ref.py) bit for bit -- targets, wS, wC
and cut for every sweep of a level, through the default and the lowered tier limits -- whole `leiden` runs, the kernel's error bits
and cog_order(method="leiden")."""
import numpy as np
import pytest
import torch

import leiden_ref as ldref
import louvain_ref as lref
from conftest import load_golden
from dgll_amd import community
from dgll_amd.graph import CSRGraph
from dgll_amd.sampling import CommunityBatchLoader

pytestmark = pytest.mark.gpu
TIERS = [(community.WAVE_MAX_DEG, community.BLOCK_MAX_DEG), (4, 16)]              # defaults; graph A's rows through every tier


@pytest.fixture(scope="module")
def golden():
    return load_golden("cog_groups")


def _np_graph(golden, name):
    return golden["rowptr_" + name].astype(np.int64), golden["col_" + name].astype(np.int32)


def _graph(golden, name, dev):
    rowptr, col = _np_graph(golden, name)
    n = len(rowptr) - 1
    return CSRGraph(torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev), None, n, n)


def _dev(dev, x, dt):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)


def _sweep_both(dev, rowptr, col, w, k, size, sub, bound, cap, resolution=1.0, tiers=TIERS):
    """The restatement's (target, wS, wC, cut), after checking that the device gives the same through every tier setting."""
    n = len(rowptr) - 1
    sub, bound = np.asarray(sub, dtype=np.int32), np.asarray(bound, dtype=np.int32)
    tot, csize, cnt = lref.community_state(k, size, sub, n)
    totP = np.zeros(n, np.int64)
    np.add.at(totP, bound, k)
    two_m = int(k.sum())
    want = ldref.refine_targets(rowptr, col, w, k, size, sub, bound, tot, csize, cnt, totP, two_m, resolution, cap)
    i64, i32 = torch.int64, torch.int32
    d = [_dev(dev, rowptr, i64), _dev(dev, col, i32), _dev(dev, w, i64), _dev(dev, k, i64), _dev(dev, size, i64), _dev(dev, sub, i32),
         _dev(dev, bound, i32), _dev(dev, tot, i64), _dev(dev, csize, i64), _dev(dev, cnt, i32), _dev(dev, totP, i64)]
    for wave_max, block_max in tiers:
        *got, movers = community.refine_targets(*d, two_m, resolution, cap, wave_max_deg=wave_max, block_max_deg=block_max,
                                                return_info=True)
        for name, g, x in zip(("target", "wS", "wC", "cut"), got, want):
            g = g.cpu().numpy()
            bad = np.nonzero(g != x)[0]
            assert bad.size == 0, "tiers (%d, %d), %s: %d rows differ, first %s: device %s, restatement %s" % (
                wave_max, block_max, name, bad.size, bad[:5], g[bad[:5]], x[bad[:5]])
        assert movers == int((want[0] != sub).sum())
    return want


def _level_both(dev, rowptr, col, w, k, size, bound, cap, resolution=1.0, tiers=TIERS):
    """Every sweep of a level's refinement on both sides; returns (sub, sweeps, movers admitted)."""
    n = len(rowptr) - 1
    sub = np.arange(n, dtype=np.int32)
    moved = 0
    for sweep in range(32):
        target = _sweep_both(dev, rowptr, col, w, k, size, sub, bound, cap, resolution, tiers)[0]
        csize = lref.community_state(k, size, sub, n)[1]
        movers, t = lref.admit(sub, ldref.settle(sub, target), size, csize, cap)
        sub[movers] = t
        moved += movers.size
        if movers.size == 0:
            break
    return sub, sweep + 1, moved


def _level0(golden, name):
    rowptr, col = _np_graph(golden, name)
    n = len(rowptr) - 1
    return rowptr, col, np.diff(rowptr).astype(np.int64), np.ones(n, np.int64)


@pytest.mark.parametrize("name", ["A", "B"])
def test_refine_after_local_moving(cuda_device, golden, name):
    rowptr, col, k, size = _level0(golden, name)
    n = len(rowptr) - 1
    bound = ldref.local_moving(rowptr, col, None, k, size, np.arange(n, dtype=np.int32), int(k.sum()), 1.0, 64, 0, 0, 32)
    sub, sweeps, moved = _level_both(cuda_device, rowptr, col, None, k, size, bound, 64)
    assert sweeps >= 2 and moved > n // 2 and ldref.disconnected(rowptr, col, sub) == 0
    assert np.array_equal(sub, ldref.refine(rowptr, col, None, k, size, bound, int(k.sum()), 1.0, 64))


def test_refine_inside_the_planted_communities(cuda_device, golden):
    rowptr, col, k, size = _level0(golden, "A")
    bound = golden["planted_A"].astype(np.int32)
    for cap in (len(k), 64):
        sub, sweeps, moved = _level_both(cuda_device, rowptr, col, None, k, size, bound, cap)
        assert sweeps >= 2 and moved > len(k) // 2 and np.bincount(sub).max() <= cap
        assert ldref.disconnected(rowptr, col, sub) == 0


def test_refine_on_a_coarse_weighted_level(cuda_device, golden):
    """Graph A aggregated once by the restatement: int64 weights, self-loop entries, k and size no longer ones."""
    rowptr, col, k, size = _level0(golden, "A")
    n = len(rowptr) - 1
    two_m = int(k.sum())
    comm = ldref.local_moving(rowptr, col, None, k, size, np.arange(n, dtype=np.int32), two_m, 1.0, 64, 0, 0, 32)
    dense = np.unique(comm, return_inverse=True)[1]
    dsub = np.unique(ldref.refine(rowptr, col, None, k, size, comm, two_m, 1.0, 64), return_inverse=True)[1].astype(np.int64)
    nc = int(dsub.max()) + 1
    bound = np.zeros(nc, np.int32)
    bound[dsub] = dense
    rowptr, col, w, k, size = ldref.coarsen(rowptr, col, None, k, size, dsub, nc)
    assert w.max() > 1 and size.max() > 1 and (col == np.repeat(np.arange(nc), np.diff(rowptr))).any()
    bound = ldref.local_moving(rowptr, col, w, k, size, bound, two_m, 1.0, 64, 0, 1, 32)
    sub, sweeps, moved = _level_both(cuda_device, rowptr, col, w, k, size, bound, 64)
    assert sweeps >= 2 and moved > 0 and np.bincount(sub, weights=size).max() <= 64


def _tiers_graph():
    """Directed CSR of 3000 nodes: rows of every length at which the kernels take another path, all inside bound community 0 (nodes
    0-2799, so every entry of those rows counts); nodes 2800-2999 sit in other bound communities.  Some sub-communities have
    several members, so targets, wS and cut are not trivial."""
    rng = np.random.RandomState(11)
    n, inside = 3000, 2800
    lengths = [1, 2, 127, 128, 129, 2048, 2049, 0, 4, 5, 16, 17]
    rows = [np.sort(rng.choice(inside, size=L, replace=False)) for L in lengths]
    rows += [np.sort(rng.choice(n, size=rng.randint(0, 13), replace=False)) for _ in range(n - len(rows))]
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rowptr[1:])
    col = np.concatenate(rows).astype(np.int32)
    bound = np.zeros(n, np.int32)
    bound[inside:] = rng.randint(1, 20, size=n - inside)
    sub = np.arange(n, dtype=np.int32)
    sub[100:400] = 100 + (np.arange(300) // 3) * 3                                  # a hundred sub-communities of three
    sub[400:500] = 400
    return rowptr, col, bound, sub, lengths


def test_every_tier_and_row_length(cuda_device):
    rowptr, col, bound, sub, lengths = _tiers_graph()
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    assert deg[:len(lengths)].tolist() == lengths
    k, size = np.maximum(deg, 1).astype(np.int64), np.ones(n, np.int64)
    tiers = TIERS + [(0, 0)]                                                        # and every row through the scratch table
    moved, targets = [], []
    for cap, res in ((n, 1.0), (n, 0.25), (3, 0.25)):
        target, wS, wC, cut = _sweep_both(cuda_device, rowptr, col, None, k, size, sub, bound, cap, res, tiers)
        assert wC[:7].tolist() == [L - int(v in col[rowptr[v]:rowptr[v + 1]]) for v, L in enumerate(lengths[:7])]
        assert wS[100:500].sum() > 0 and cut.sum() == (wC - wS).sum()
        moved.append(target != sub)
        targets.append(target)
    assert min(m.sum() for m in moved) > 100
    assert moved[1][[2, 3, 4, 5, 6]].all()                                          # the long rows decide and move
    assert (targets[1] != targets[2]).sum() > 100                                   # cap 3: the sub-communities of three are full


@pytest.fixture(scope="module")
def whole_runs(golden):
    """The restatement's labels, computed once: (graph, cap, seed) -> labels."""
    out = {}
    for name in "AB":
        rowptr, col = _np_graph(golden, name)
        for cap in (None, 64):
            for seed in (0, 1):
                out[name, cap, seed] = ldref.leiden(rowptr, col, max_comm_size=cap, seed=seed)
    return out


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("cap", [None, 64])
@pytest.mark.parametrize("seed", [0, 1])
def test_whole_run_equals_the_restatement(cuda_device, golden, whole_runs, name, cap, seed):
    g = _graph(golden, name, cuda_device)
    seen = {"move": 0, "refine": 0}

    def on_sweep(level, sweep, comm, size):
        seen["move"] += 1

    def on_refine(level, sweep, sub, bound, size):
        seen["refine"] += 1
        assert sub.shape == bound.shape == size.shape

    labels = community.leiden(g, max_comm_size=cap, seed=seed, on_sweep=on_sweep, on_refine=on_refine)
    assert labels.dtype == torch.int64 and labels.device == g.device
    assert np.array_equal(labels.cpu().numpy(), whole_runs[name, cap, seed])
    assert seen["move"] >= 3 and seen["refine"] >= 2
    rowptr, col = _np_graph(golden, name)
    assert ldref.disconnected(rowptr, col, labels.cpu().numpy()) == 0
    assert int(torch.bincount(labels).max()) <= (cap or g.n_rows)
    assert torch.equal(community.leiden(g, max_comm_size=cap, seed=seed), labels)                    # a second call
    assert torch.equal(dgll_leiden()(g, max_comm_size=cap, seed=seed), labels)


def dgll_leiden():
    import dgll

    return dgll.community.leiden


def test_error_bits(cuda_device, golden):
    rowptr, col, k, size = _level0(golden, "A")
    n = len(rowptr) - 1
    i64, i32 = torch.int64, torch.int32
    sub, bound = np.arange(n, dtype=np.int32), golden["planted_A"].astype(np.int32)
    tot, csize, cnt = lref.community_state(k, size, sub, n)
    totP = np.zeros(n, np.int64)
    np.add.at(totP, bound, k)

    def run(col=col, sub=sub, bound=bound):
        dev = cuda_device
        return community.refine_targets(_dev(dev, rowptr, i64), _dev(dev, col, i32), None, _dev(dev, k, i64), _dev(dev, size, i64),
                                        _dev(dev, sub, i32), _dev(dev, bound, i32), _dev(dev, tot, i64), _dev(dev, csize, i64),
                                        _dev(dev, cnt, i32), _dev(dev, totP, i64), int(k.sum()), 1.0, n)

    run()
    bad = col.copy()
    bad[7] = n
    with pytest.raises(ValueError, match="column id outside"):
        run(col=bad)
    bad = bound.copy()
    bad[5] = -1
    with pytest.raises(ValueError, match="bound community id outside"):
        run(bound=bad)
    bad = bound.copy()
    bad[n - 1] = n
    with pytest.raises(ValueError, match="bound community id outside"):
        run(bound=bad)
    bad = sub.copy()
    bad[3] = n + 5
    with pytest.raises(ValueError, match="a community id outside"):
        run(sub=bad)
    g = _graph(golden, "A", cuda_device)
    with pytest.raises(ValueError, match="max_comm_size"):
        community.leiden(g, max_comm_size=0)
    assert community.leiden(CSRGraph(torch.zeros(4, dtype=torch.int64, device=cuda_device),
                                     torch.zeros(0, dtype=torch.int32, device=cuda_device), None, 3, 3)).tolist() == [0, 1, 2]


def test_cog_order_with_leiden(cuda_device, golden):
    g = _graph(golden, "B", cuda_device)
    n = g.n_rows
    book = community.cog_order(g, 500, max_comm_size=200, method="leiden", seed=0)
    comm = book.community
    assert sorted(book.perm.tolist()) == list(range(n)) and int(torch.bincount(comm).max()) <= 200
    ranges = book.group_ranges.tolist()
    assert ranges[0][0] == 0 and ranges[-1][1] == n and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert int((comm[1:] != comm[:-1]).sum()) + 1 == int(comm.unique().numel())     # a community is one contiguous run
    for start, end in ranges[:-1]:                                                   # a group is a run of whole communities
        assert int(comm[end - 1]) != int(comm[end])
    g2 = book.relabel(g)
    assert ldref.disconnected(g2.rowptr.cpu().numpy(), g2.col.cpu().numpy(), comm.cpu().numpy()) == 0
    feats = torch.arange(n, dtype=torch.float32, device=cuda_device).unsqueeze(1)
    loader = CommunityBatchLoader(g, feats, torch.arange(n, device=cuda_device) % 7, 500, max_comm_size=200, method="leiden")
    assert torch.equal(loader.book.perm, book.perm)
    at = 0
    for (start, end), sub, x, y in loader:
        assert start == at and sub.n_rows == end - start and torch.equal(x[:, 0].long(), loader.book.perm[start:end])
        at = end
    assert at == n and len(loader) >= 2
    # without `method` the parent commit's result: the book of `louvain`'s labels
    labels = community.louvain(g, max_comm_size=200, seed=0)
    plain = community.cog_order(g, 500, max_comm_size=200, seed=0)
    assert torch.equal(labels[plain.perm].unique_consecutive(return_inverse=True)[1], plain.community)
    named = community.cog_order(g, 500, max_comm_size=200, method="louvain", seed=0)
    assert torch.equal(named.perm, plain.perm) and torch.equal(named.group_ranges, plain.group_ranges)
    order, dense = community.order_by_labels(labels, g.degrees())
    assert torch.equal(plain.community, dense[plain.perm])
