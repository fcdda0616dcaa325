"""Neighbour sampler, host side: the numpy restatement (tests/neighbor_ref.py) draws uniform subsets and builds valid blocks; the C ABI
and the Python front end refuse bad arguments without a GPU."""
import numpy as np
import pytest
import torch

import neighbor_ref as ref

STAT_SEED = 20240607


def regular_graph(n_rows, nbrs):
    """Rows 0 .. n_rows-1 each list the same in-neighbours; the remaining nodes have none."""
    nbrs = np.asarray(nbrs, np.int32)
    n = max(n_rows, int(nbrs.max()) + 1)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:n_rows + 1] = len(nbrs)
    rowptr = np.cumsum(rowptr)
    return rowptr, np.tile(nbrs, n_rows), n


def test_subsets_are_uniform():
    """4096 rows of degree 12, fan-out 5, one seed: inclusion counts per position against 4096 * 5 / 12 (Pearson statistic below the
    chi-square 0.999 quantile at 11 degrees of freedom, 31.26 -- conservative, inclusions without replacement are negatively
    correlated) and every pair of positions within 15 % of 4096 * (5 * 4) / (12 * 11)."""
    rows, d, f = 4096, 12, 5
    single = np.zeros(d)
    pair = np.zeros((d, d))
    for v in range(rows):
        p = ref.positions(d, v, f, STAT_SEED, 0)
        assert len(p) == f and len(set(p)) == f and p == sorted(p) and 0 <= p[0] and p[-1] < d
        single[p] += 1
        for a in p:
            for b in p:
                pair[a, b] += a != b
    exp = rows * f / d
    chi2 = float(((single - exp) ** 2 / exp).sum())
    print("pearson", chi2, "counts", single)
    assert chi2 < 31.26, chi2
    exp2 = rows * (f * (f - 1)) / (d * (d - 1))
    off = pair[~np.eye(d, dtype=bool)]
    print("pairs: expected", exp2, "min", off.min(), "max", off.max())
    assert np.all(np.abs(off - exp2) < 0.15 * exp2), (off.min(), off.max(), exp2)


def test_exact_cases():
    for d, f in ((7, 7), (3, 7), (0, 4), (1, 1)):                 # d == f, d < f: all kept
        assert ref.positions(d, 11, f, 5, 1) == list(range(d))
    for d in (2, 8, 65):                                         # d == f + 1: exactly one dropped
        f = d - 1
        dropped = set()
        for v in range(200):
            p = ref.positions(d, v, f, 9, 0)
            assert len(p) == f and len(set(p)) == f and set(p) <= set(range(d))
            dropped |= set(range(d)) - set(p)
        assert len(dropped) > 1                                  # and not always the same one
    hits = np.zeros(9)
    for v in range(900):                                         # f = 1: one position, all of them reachable
        p = ref.positions(9, v, 1, 3, 2)
        assert len(p) == 1
        hits[p[0]] += 1
    assert hits.min() > 0
    assert ref.positions(5000, 3, -1, 1, 0) == list(range(5000))   # f = -1: every neighbour
    # the draw depends on (seed, layer, node, fan-out) only
    assert ref.positions(100, 42, 10, 7, 1) == ref.positions(100, 42, 10, 7, 1)
    assert len({tuple(ref.positions(100, 42, 10, s, l)) for s in (7, 8) for l in (0, 1)}) == 4
    rowptr, col, _ = regular_graph(4, [9, 3, 7, 5])
    assert ref.draw(rowptr, col, 2, -1, 0, 0) == [9, 3, 7, 5]     # ascending POSITION, not id
    got = ref.draw(rowptr, col, 2, 2, 0, 0)
    assert [c for c in [9, 3, 7, 5] if c in got] == got and len(got) == 2


def small_graph(n=203, seed=1):
    rng = np.random.default_rng(seed)
    rows = []
    for v in range(n):
        d = int(rng.choice([0, 1, 2, 3, 4, 6, 11, 40]))
        nb = rng.choice(n, d, replace=False)
        if v % 5 == 0 and d:
            nb[0] = v                                            # self-loops
        rows.append(np.unique(nb))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rowptr, np.concatenate(rows).astype(np.int32), n


@pytest.mark.parametrize("fanouts", [[1], [5, 2], [-1, 3], [3, 3, 3]], ids=str)
@pytest.mark.parametrize("norm", ["mean", None])
def test_restatement_builds_valid_blocks(fanouts, norm):
    rowptr, col, n = small_graph()
    seeds = np.random.default_rng(2).permutation(n)[:37]
    seeds[0] = n - 1
    inp, blocks = ref.sample_blocks(rowptr, col, seeds, fanouts, 17, norm)
    ref.check_invariants(rowptr, col, seeds, fanouts, inp, blocks, norm)
    inp2, blocks2 = ref.sample_blocks(rowptr, col, seeds, fanouts, 17, norm)
    assert np.array_equal(inp, inp2) and all(np.array_equal(a["col"], b["col"]) for a, b in zip(blocks, blocks2))
    with pytest.raises(AssertionError):
        ref.sample_blocks(rowptr, col, [3, 4, 3], fanouts, 17, norm)


def test_c_abi_argument_validation_needs_no_gpu():
    from dgll_amd import _lib

    lib = _lib.lib
    assert lib.dgll_hip_nb_max_fanout() >= 64
    p = 16                     # any non-NULL address: the checks fail before anything is touched
    assert lib.dgll_hip_nb_sample(None, None, p, 10, p, 4, 2, 1, 0, p, p, 1, p, p, p, 8, p, p) == -1 and "non-NULL" in _lib.last_error()
    assert lib.dgll_hip_nb_sample(None, p, p, 10, p, 4, 65, 1, 0, p, p, 1, p, p, p, 260, p, p) == -1 and "fan-out" in _lib.last_error()
    assert lib.dgll_hip_nb_sample(None, p, p, 10, p, 4, 0, 1, 0, p, p, 1, p, p, p, 260, p, p) == -1 and "fan-out" in _lib.last_error()
    assert lib.dgll_hip_nb_sample(None, p, p, 10, p, 4, 2, 1, 0, p, p, 0, p, p, p, 8, p, p) == -1 and "epoch" in _lib.last_error()
    assert lib.dgll_hip_nb_sample(None, p, p, 10, p, 4, 2, 1, 0, p, p, 1, p, p, p, 7, p, p) == -1 and "draw buffer" in _lib.last_error()
    assert lib.dgll_hip_nb_sample(None, p, p, 2 ** 31, p, 4, 2, 1, 0, p, p, 1, p, p, p, 8, p, p) == -1
    assert lib.dgll_hip_nb_block(None, p, p, 10, p, 4, 2, p, p, 1, p, p, p, p, 8, 3, p, None, p, None) == -1 and "non-NULL" in _lib.last_error()
    assert lib.dgll_hip_nb_block(None, p, p, 10, p, 4, 2, p, p, 1, p, p, None, p, 8, 3, p, p, p, None) == -1 and "draw buffer" in _lib.last_error()
    assert lib.dgll_hip_nb_block(None, p, p, 10, p, 4, 2, p, p, 1, p, p, p, p, 8, 11, p, p, p, None) == -1
    assert lib.dgll_hip_nb_block(None, p, p, 10, p, 4, -1, p, p, 1, p, p, None, p, 8, 3, None, p, p, None) == -1


def test_front_end_refuses_what_it_documents(monkeypatch):
    from dgll_amd.graph import CSRGraph
    from dgll_amd.sampling import NeighborSampler
    from dgll_amd.sampling import neighbor

    import dgll.sampling.neighbor as alias

    assert alias.NeighborSampler is NeighborSampler and neighbor.MAX_FANOUT >= 64
    with pytest.raises(NotImplementedError, match="replace"):
        NeighborSampler([4, 4], replace=True)
    for bad in ([neighbor.MAX_FANOUT + 1], [4, 0], [], [-2]):
        with pytest.raises(ValueError, match="fanouts"):
            NeighborSampler(bad)
    with pytest.raises(ValueError, match="norm"):
        NeighborSampler([4], norm="sum")
    rowptr, col, n = small_graph()
    g = CSRGraph(torch.as_tensor(rowptr), torch.as_tensor(col), None, n, n)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU"):
        NeighborSampler([4, 4], g)
    s = NeighborSampler([4, 4])                  # the graph may come with the first sample()
    with pytest.raises(RuntimeError, match="GPU"):
        s.sample(g, [1, 2, 3])
    with pytest.raises(ValueError, match="graph"):
        s.sample(None, [1, 2, 3])
