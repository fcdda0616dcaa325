"""Edge-weighted walks without a GPU: the restated walker on a host-built alias table against the reference's weighted transition
probabilities (tests/golden/node2vec_probs_weighted.npz), the distribution the host builder's tables imply, and argument
validation of the two new C-ABI functions."""
import ctypes as C

import numpy as np
import pytest

import weighted_walk_ref as wref
from conftest import load_golden
from test_embedding_host import golden_starts, transition_check


def row_shares(rowptr, val):
    """w / sum of the row's w in float64, 0 in a row whose weights sum to 0."""
    deg = np.diff(rowptr)
    rows = np.repeat(np.arange(len(deg)), deg)
    total = np.bincount(rows, weights=np.asarray(val, np.float64), minlength=len(deg))[rows]
    return np.where(total > 0, np.asarray(val, np.float64) / np.where(total > 0, total, 1.0), 0.0)


def hub_first_step_excess(golden, walk_arr):
    """Worst excess of |first-step frequency from the hub - w / sum w| over transition_check's cap 5 sqrt(P (1 - P) / n) + 1 / n."""
    hub, rowptr = golden.meta["hub"], golden["rowptr"]
    b, e = rowptr[hub], rowptr[hub + 1]
    P = row_shares(rowptr, golden["val"])[b:e]
    first = walk_arr[walk_arr[:, 0] == hub, 1]
    n = float(len(first))
    pos = np.searchsorted(golden["col"][b:e], first)
    assert np.array_equal(golden["col"][b:e][pos], first)
    freq = np.bincount(pos, minlength=e - b) / n
    assert not freq[P == 0].any()
    return float((np.abs(freq - P) - (5.0 * np.sqrt(P * (1.0 - P) / n) + 1.0 / n)).max())


@pytest.fixture(scope="module")
def golden():
    return load_golden("node2vec_probs_weighted")


def test_weighted_fixture_has_the_promised_shape(golden):
    plain = load_golden("node2vec_probs")
    assert np.array_equal(golden["rowptr"], plain["rowptr"]) and np.array_equal(golden["col"], plain["col"])
    val, rowptr = golden["val"], golden["rowptr"]
    assert val.dtype == np.float32 and np.isfinite(val).all() and (val >= 0).all()
    assert (val == 0).sum() == golden.meta["zero_weights"] > 0
    deg = np.diff(rowptr)
    total = np.bincount(np.repeat(np.arange(len(deg)), deg), weights=val.astype(np.float64), minlength=len(deg))
    assert (total[deg > 0] > 0).all()                                   # never a whole row of zeros
    hub = val[rowptr[golden.meta["hub"]]:rowptr[golden.meta["hub"] + 1]]
    assert 500 <= np.sort(hub)[-1] / np.sort(hub)[-2] <= 2000           # one edge dominates the rest by about 10^3
    assert golden["start_reps"].sum() == golden.meta["n_walks"]
    for i in range(2):
        sums = np.add.reduceat(np.append(golden["probs_%d" % i], 0.0), golden["prob_ptr"][:-1])
        np.testing.assert_allclose(sums[np.diff(golden["prob_ptr"]) > 0], 1.0, rtol=1e-12)
        assert (golden["probs_%d" % i] == 0).any()                      # a zero-weight edge is a transition of probability 0


@pytest.mark.parametrize("case", [0, 1])
def test_restated_weighted_walker_follows_the_reference_probabilities(golden, case):
    p, q = golden.meta["pq"][case]
    T, alias = wref.build_alias(golden["rowptr"], golden["val"])
    wk, capped = wref.walks(golden["rowptr"], golden["col"], T, alias, golden_starts(golden), 3, p, q, seed=golden.meta["seed"],
                            return_capped=True)
    assert capped == 0
    checked, mass, excess = transition_check(golden, wk, case)
    print("p=%g q=%g: %d of %d cells checked, worst excess over the cap %.3g" % (p, q, checked, mass, excess))
    assert excess <= 0.0


def test_restated_first_step_is_weighted(golden):
    T, alias = wref.build_alias(golden["rowptr"], golden["val"])
    wk = wref.walks(golden["rowptr"], golden["col"], T, alias, golden_starts(golden), 2, seed=golden.meta["seed"])
    assert hub_first_step_excess(golden, wk) <= 0.0


def test_host_builder_implies_the_weights():
    rowptr, _, val, kinds = wref.shapes_graph()
    T, alias = wref.build_alias(rowptr, val)
    deg = np.diff(rowptr)
    assert (alias < np.repeat(deg, deg)).all()
    got, want = wref.implied_probs(rowptr, T, alias), row_shares(rowptr, val)
    assert not got[val == 0].any()
    assert np.abs(got - want).max() <= 2.0 ** -30
    sums = np.bincount(np.repeat(np.arange(len(deg)), deg), weights=got, minlength=len(deg))
    live = np.array([k not in (None, "all_zero") for k in kinds]) & (deg > 0)
    np.testing.assert_allclose(sums[live], 1.0, rtol=0, atol=1e-12)
    assert not sums[~live].any()
    ones = wref.implied_probs(rowptr, *wref.build_alias(rowptr, np.ones(len(val))))
    assert np.array_equal(ones, 1.0 / np.repeat(deg, deg))              # unit weights: exactly uniform


def test_weighted_entry_points_validate_without_a_gpu():
    from dgll_amd import _lib

    lib = _lib.lib
    buf = (C.c_int64 * 16)()
    a = C.addressof(buf)
    good = dict(rowptr=a, col=a, table=a, n_nodes=4, starts=a, n=2, length=3, first=0, seed=0, p=1.0, q=1.0, cap=1024, walks=a, info=a)

    def walk(**kw):
        k = dict(good, **kw)
        return lib.dgll_hip_random_walk_weighted(None, k["rowptr"], k["col"], k["table"], k["n_nodes"], k["starts"], k["n"], k["length"],
                                                 k["first"], k["seed"], k["p"], k["q"], k["cap"], k["walks"], k["info"])

    for kw, word in ((dict(table=None), "NULL"), (dict(rowptr=None), "NULL"), (dict(info=None), "NULL"), (dict(table=a + 4), "aligned"),
                     (dict(length=0), "length"), (dict(p=0.0), "p and q"), (dict(p=-1.0), "p and q"), (dict(q=0.0), "p and q"),
                     (dict(cap=8), "1024")):
        assert walk(**kw) == -1 and word in _lib.last_error(), (kw, _lib.last_error())
    build = dict(rowptr=a, val=a, n_rows=2, nnz=4, scratch=a, scratch_bytes=48, table=a, info=a)

    def alias_build(**kw):
        k = dict(build, **kw)
        return lib.dgll_hip_alias_build(None, k["rowptr"], k["val"], k["n_rows"], k["nnz"], k["scratch"], k["scratch_bytes"], k["table"],
                                        k["info"])

    for kw, word in ((dict(table=None), "NULL"), (dict(val=None), "NULL"), (dict(scratch=None), "NULL"), (dict(info=None), "NULL"),
                     (dict(n_rows=-1), "counts"), (dict(scratch_bytes=47), "12 bytes"), (dict(table=a + 4), "aligned")):
        assert alias_build(**kw) == -1 and word in _lib.last_error(), (kw, _lib.last_error())


def test_python_layer_refuses_weighted_walks_it_cannot_draw():
    import torch

    import dgll_amd
    from dgll_amd import embedding

    g = dgll_amd.CSRGraph.from_coo(torch.tensor([0, 1]), torch.tensor([1, 0]), None, (2, 2))
    with pytest.raises(ValueError):
        embedding.AliasTable.from_graph(g)                              # no values
    with pytest.raises(RuntimeError):
        embedding.AliasTable.from_graph(g.with_values(torch.ones(2)))   # values, but not on the GPU
    with pytest.raises(ValueError):
        embedding.AliasTable(torch.zeros((3, 2), dtype=torch.int64), 3)
