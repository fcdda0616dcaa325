"""Leiden on the host: the numpy restatement (tests/leiden_ref.py, what the device is held to bit for bit in test_leiden_gpu.py) on
the two fixture graphs -- every community connected, the cap kept, modularity next to networkx's and to the size-capped Louvain's,
the refinement's invariants after every sweep -- and the argument checks that need no GPU."""
import numpy as np
import pytest
import torch

import leiden_ref as ldref
import louvain_ref as lref
from conftest import load_golden
from dgll_amd import community
from dgll_amd.graph import CSRGraph


@pytest.fixture(scope="module")
def golden():
    return load_golden("cog_groups")


def _graph(golden, name):
    return golden["rowptr_" + name].astype(np.int64), golden["col_" + name].astype(np.int32)


@pytest.fixture(scope="module")
def runs(golden):
    """(graph, cap, seed) -> the restatement's labels, computed once."""
    return {(name, cap, seed): ldref.leiden(*_graph(golden, name), max_comm_size=cap, seed=seed)
            for name in "AB" for cap in (None, 64) for seed in (0, 1, 2)}


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("cap", [None, 64])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_every_community_is_connected(golden, runs, name, cap, seed):
    rowptr, col = _graph(golden, name)
    labels = runs[name, cap, seed]
    sizes = np.bincount(labels)
    print("graph", name, "cap", cap, "seed", seed, "communities", sizes.size, "largest", sizes.max())
    assert labels.dtype == np.int64 and sorted(np.unique(labels).tolist()) == list(range(int(labels.max()) + 1))      # dense
    assert ldref.disconnected(rowptr, col, labels) == 0
    if cap is not None:
        assert 32 < sizes.max() <= 64


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_uncapped_modularity_reaches_networkx(golden, runs, name, seed):
    rowptr, col = _graph(golden, name)
    q = lref.modularity(rowptr, col, runs[name, None, seed])
    floor = float(golden["nx_modularity_" + name].min())
    print("graph", name, "seed", seed, "Q", q, "networkx min", floor, "ratio", q / floor)
    assert q >= 0.98 * floor


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_capped_modularity_keeps_louvains(golden, runs, name, seed):
    rowptr, col = _graph(golden, name)
    q = lref.modularity(rowptr, col, runs[name, 64, seed])
    base = lref.modularity(rowptr, col, lref.louvain(rowptr, col, max_comm_size=64, seed=seed))
    print("graph", name, "cap 64 seed", seed, "Q", q, "louvain Q", base, "ratio", q / base)
    assert q >= 0.98 * base


def _check_sweeps(graph_of_level, cap):
    """An on_refine callback that holds every sweep to the refinement's invariants; graph_of_level(level) -> (rowptr, col) or None."""
    state = {"level": -1, "calls": 0}

    def check(level, sweep, sub, bound, size):
        n = len(sub)
        if level != state["level"]:
            assert sweep == 0
            state.update(level=level, before=np.arange(n, dtype=np.int32))
        before = state["before"]
        pairs = np.unique(np.stack([sub.astype(np.int64), np.asarray(bound, dtype=np.int64)]), axis=1)
        assert pairs.shape[1] == np.unique(sub).size                                   # inside one bound community
        assert np.bincount(sub, weights=size).max() <= cap
        settled = np.bincount(before, minlength=n)[before] > 1                         # members of a non-singleton stay
        assert np.array_equal(sub[settled], before[settled])
        g = graph_of_level(level)
        if g is not None:
            assert ldref.disconnected(g[0], g[1], sub) == 0
        state["before"] = sub.copy()
        state["calls"] += 1

    return check, state


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("cap", [None, 64])
def test_refinement_invariants_after_every_sweep(golden, name, cap):
    rowptr, col = _graph(golden, name)
    n = len(rowptr) - 1
    check, state = _check_sweeps(lambda level: (rowptr, col) if level == 0 else None, cap or n)
    ldref.leiden(rowptr, col, max_comm_size=cap, seed=0, on_refine=check)
    assert state["level"] >= 2 and state["calls"] >= 6
    # a coarse level with its own graph: connectivity there too
    k, size = np.diff(rowptr).astype(np.int64), np.ones(n, np.int64)
    two_m = int(k.sum())
    comm = ldref.local_moving(rowptr, col, None, k, size, np.arange(n, dtype=np.int32), two_m, 1.0, cap or n, 0, 0, 32)
    dense = np.unique(comm, return_inverse=True)[1]
    dsub = np.unique(ldref.refine(rowptr, col, None, k, size, comm, two_m, 1.0, cap or n), return_inverse=True)[1].astype(np.int64)
    nc = int(dsub.max()) + 1
    bound = np.zeros(nc, np.int32)
    bound[dsub] = dense
    coarse = ldref.coarsen(rowptr, col, None, k, size, dsub, nc)
    check, state = _check_sweeps(lambda level: coarse[:2], cap or n)
    sub = ldref.refine(*coarse, bound, two_m, 1.0, cap or n, level=1, on_refine=check)
    assert state["calls"] >= 2 and np.unique(sub).size < nc


def test_the_fixture_shows_louvains_defect(golden):
    rowptr, col = _graph(golden, "B")
    for seed in (0, 2):
        pieces = ldref.disconnected(rowptr, col, lref.louvain(rowptr, col, max_comm_size=64, seed=seed))
        print("graph B cap 64 seed", seed, "louvain: disconnected communities", pieces)
        assert pieces > 0


def test_two_runs_give_identical_labels(golden, runs):
    rowptr, col = _graph(golden, "A")
    assert np.array_equal(ldref.leiden(rowptr, col, max_comm_size=64, seed=2), runs["A", 64, 2])
    assert not np.array_equal(runs["A", 64, 2], runs["A", 64, 1])                      # the seed picks the active halves


def test_targets_stay():
    sub = np.array([0, 1, 2, 3, 3], dtype=np.int32)
    target = np.array([0, 0, 1, 3, 3], dtype=np.int32)                                 # 2 aims at 1, which wants to leave: 1 stays
    assert ldref.settle(sub, target).tolist() == [0, 1, 1, 3, 3]


def test_leiden_needs_the_gpu_and_a_known_method(golden):
    rowptr, col = _graph(golden, "A")
    n = len(rowptr) - 1
    g = CSRGraph(torch.from_numpy(rowptr), torch.from_numpy(col), None, n, n)
    with pytest.raises(RuntimeError, match="GPU only"):
        community.leiden(g)
    import dgll

    with pytest.raises(RuntimeError, match="GPU only"):
        dgll.community.leiden(g, max_comm_size=64)
    with pytest.raises(RuntimeError, match="GPU only"):
        community.cog_order(g, 100, method="leiden")
    with pytest.raises(ValueError, match="'louvain' or 'leiden'"):
        community.cog_order(g, 100, method="nope")
    k = torch.from_numpy(np.diff(rowptr))
    with pytest.raises(RuntimeError, match="GPU only"):
        community.refine_targets(g.rowptr, g.col, None, k, k, g.col, g.col, k, k, g.col, k, n, 1.0, n)


def test_abi_rejects_bad_arguments_without_a_gpu():
    from dgll_amd import _lib

    p = 16                                                        # never dereferenced: validation comes first
    args = lambda two_m, cap, wave, block: (None, p, p, None, p, p, p, p, p, p, p, p, 4, 4, two_m, 1.0, cap, wave, block, p, 1 << 20,  # noqa: E731
                                            p, p, p, p, p)
    refine = _lib.lib.dgll_hip_leiden_refine
    assert refine(*args(2 ** 53, 4, -1, -1)) == -1 and "2^53" in _lib.last_error()
    assert refine(*args(0, 4, -1, -1)) == -1 and "2^53" in _lib.last_error()
    assert refine(*args(8, 0, -1, -1)) == -1 and "cap" in _lib.last_error()
    assert refine(*args(8, 4, 129, -1)) == -1 and "wave_max_deg" in _lib.last_error()
    assert refine(*args(8, 4, 4, 4096)) == -1 and "block_max_deg" in _lib.last_error()
    null = list(args(8, 4, -1, -1))
    null[7] = None                                                # bound
    assert refine(*null) == -1 and "NULL" in _lib.last_error()
    small = list(args(8, 4, -1, -1))
    small[20] = 64                                                # scratch bytes: no room for the queue
    assert refine(*small) == -1 and "scratch" in _lib.last_error()
