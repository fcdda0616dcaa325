"""Edge-weighted neighbour sampling (NeighborSampler(prob=...)), host side: the numpy restatement (tests/neighbor_weighted_ref.py)
follows Plackett-Luce and builds valid blocks with zero weights present; the weight check, the new C entry point and the front end
refuse bad arguments without a GPU."""
import numpy as np
import pytest
import torch

import neighbor_ref as ref
import neighbor_weighted_ref as wref


def test_kept_sets_follow_plackett_luce():
    """20 000 rows over the same 7 neighbours, weights 0.38 .. 0.04 and 0, fan-out 3, one seed: the counts of the 20 kept sets."""
    sets, min_gap = wref.dist_reference()
    print("smallest gap", min_gap)
    assert min_gap > wref.MIN_GAP               # the device draws the same sets (test_neighbor_weighted_gpu.py relies on it)
    wref.check_set_counts(sets)


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
def test_restatement_builds_valid_blocks_with_zero_weights(fanouts, norm):
    rowptr, col, n = small_graph()
    w = wref.build_weights(rowptr, 3, zero_every=2)
    assert (w == 0).sum() > 50 and (w > 0).sum() > 50
    seeds = np.random.default_rng(2).permutation(n)[:37]
    seeds[0] = n - 1
    inp, blocks, _, (frp, fcol, fw) = wref.sample_blocks(rowptr, col, w, seeds, fanouts, 17, norm)
    assert len(fcol) == len(fw) == (w > 0).sum() == frp[-1] and np.all(fw > 0)
    ref.check_invariants(frp, fcol, seeds, fanouts, inp, blocks, norm)          # min(positive entries, f) per row, every edge kept
    inp2, blocks2, _, _ = wref.sample_blocks(rowptr, col, w, seeds, fanouts, 17, norm)
    assert np.array_equal(inp, inp2) and all(np.array_equal(a["col"], b["col"]) for a, b in zip(blocks, blocks2))
    zero_edges = {(v, int(c)) for v in range(n) for c, x in zip(col[rowptr[v]:rowptr[v + 1]], w[rowptr[v]:rowptr[v + 1]]) if x == 0}
    for blk in blocks:                                                           # an entry of weight 0 is never sampled
        for r, v in enumerate(blk["dst"]):
            for c in blk["src"][blk["col"][blk["rowptr"][r]:blk["rowptr"][r + 1]]]:
                assert (int(v), int(c)) not in zero_edges


def test_exact_cases():
    rng = np.random.default_rng(0)
    for d, f in ((7, 7), (3, 7), (0, 4), (1, 1), (5000, -1)):    # d == f, d < f, f = -1: every positive entry
        assert wref.positions(rng.uniform(0.1, 9.0, d).astype(np.float32), 11, f, 5, 1) == (list(range(d)), None)
    for d in (2, 8, 65):                                         # d == f + 1: exactly one dropped
        f, w = d - 1, rng.uniform(0.5, 2.0, d).astype(np.float32)
        dropped = set()
        for v in range(200):
            p, gap = wref.positions(w, v, f, 9, 0)
            assert len(p) == f and len(set(p)) == f and set(p) <= set(range(d)) and p == sorted(p) and 0 < gap < 1
            dropped |= set(range(d)) - set(p)
        assert len(dropped) > 1                                  # and not always the same one
    w = rng.uniform(0.5, 2.0, 100).astype(np.float32)            # the draw depends on (seed, layer, node, fan-out, its row) only
    assert wref.positions(w, 42, 10, 7, 1) == wref.positions(w.copy(), 42, 10, 7, 1)
    assert len({tuple(wref.positions(w, 42, 10, s, l)[0]) for s in (7, 8) for l in (0, 1)}) == 4
    heavy = np.full(50, 1e-6, np.float32)                        # in proportion to the weights: three entries carry all the mass
    heavy[[4, 17, 33]] = 1e6
    assert all(wref.positions(heavy, v, 3, 1, 0)[0] == [4, 17, 33] for v in range(50))
    # the stream is not the uniform sampler's: counter word 2 carries the high bit
    assert ref.philox([5, 0, 1, 0], [7, 0]) != ref.philox([5, 0, 1 | 0x80000000, 0], [7, 0])


def test_weight_check_needs_no_gpu():
    from dgll_amd.sampling import neighbor

    w = neighbor.check_weights(np.array([0.5, 0.0, 3.0], np.float64), 3)
    assert w.dtype == torch.float32 and w.tolist() == [0.5, 0.0, 3.0]
    assert neighbor.check_weights(torch.tensor([1, 2, 0]), 3).dtype == torch.float32
    for bad in ([1.0, -0.5, 2.0], [1.0, float("nan"), 2.0], [1.0, float("inf"), 2.0], [1.0, 1e39, 2.0]):
        with pytest.raises(ValueError, match="finite"):
            neighbor.check_weights(np.array(bad), 3)
        with pytest.raises(ValueError, match="finite"):
            neighbor.check_weights(torch.tensor(bad, dtype=torch.float64), 3)
    for n in (2, 4, 0):
        with pytest.raises(ValueError, match="one weight per entry"):
            neighbor.check_weights(np.ones(3, np.float32), n)
    rowptr, col, w3 = torch.tensor([0, 2, 2, 5]), torch.tensor([1, 2, 0, 1, 2], dtype=torch.int32), torch.tensor([1.0, 0.0, 0.0, 2.0, 0.0])
    frp, fcol, fw = neighbor.drop_zero_weights(rowptr, col, w3)
    assert frp.tolist() == [0, 1, 1, 2] and fcol.tolist() == [1, 1] and fw.tolist() == [1.0, 2.0] and fcol.dtype == torch.int32
    same = neighbor.drop_zero_weights(rowptr, col, torch.ones(5))
    assert same[0] is rowptr and same[1] is col
    want = wref.drop_zero_weights(rowptr.numpy(), col.numpy(), w3.numpy())
    assert all(np.array_equal(a.numpy(), b) for a, b in zip((frp, fcol, fw), want))


def test_c_abi_argument_validation_needs_no_gpu():
    from dgll_amd import _lib

    lib = _lib.lib
    assert 64 <= lib.dgll_hip_nb_long_row() <= 4096
    p = 16                     # any non-NULL address: the checks fail before anything is touched
    ok = [None, p, p, p, 10, p, 4, 2, 1, 0, p, p, 1, p, p, p, 12, p, p]          # stream, rowptr, col, weight, n, rows, 4 rows, f = 2, ...

    def call(**change):
        a = list(ok)
        for i, x in change.items():
            a[int(i[1:])] = x
        return lib.dgll_hip_nb_sample_weighted(*a)

    for i in (1, 2, 3, 5, 10, 11, 13, 14, 15, 17, 18):                            # every pointer argument
        assert call(**{"a%d" % i: None}) == -1 and "non-NULL" in _lib.last_error(), i
    for f in (0, -1, 65):
        assert call(a7=f, a16=4 * 66) == -1 and "fan-out" in _lib.last_error(), f
    assert call(a16=11) == -1 and "draw buffer" in _lib.last_error()              # 4 rows * (2 + 1) entries are needed
    assert call(a16=8) == -1 and "draw buffer" in _lib.last_error()               # the uniform entry's size is too short here
    assert call(a12=0) == -1 and "epoch" in _lib.last_error()
    assert call(a4=2 ** 31) == -1 and call(a6=0) == -1 and call(a9=-1) == -1


def test_front_end_refuses_what_it_documents(monkeypatch):
    from dgll_amd.graph import CSRGraph
    from dgll_amd.sampling import NeighborSampler

    with pytest.raises(ValueError, match="prob"):
        NeighborSampler([4], prob="degree")
    with pytest.raises(NotImplementedError, match="replace"):
        NeighborSampler([4], replace=True, prob="weight")
    rowptr, col, n = small_graph()
    g = CSRGraph(torch.as_tensor(rowptr), torch.as_tensor(col), None, n, n)
    s = NeighborSampler([4, 4], prob=np.ones(len(col)))         # nothing is checked before a graph is bound
    assert s.graph is None and s.prob is not None
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU"):
        NeighborSampler([4, 4], g, prob="weight")
