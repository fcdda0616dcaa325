"""struc2vec without a GPU: the numpy restatement (tests/struc2vec_ref.py) against the fixture recorded from the reference's own
functions (tests/golden/gen_struc2vec_goldens.py), the restated walker's frequencies, and the public class's plumbing."""
import numpy as np
import pytest

import struc2vec_ref as sref
import weighted_walk_ref as wref
from conftest import load_golden

GOLDEN = "struc2vec_context"
# walks per start node of the frequency tests.  The rule needs 500 stay steps from a row before it judges the row's cells, and a
# walk of 12 nodes at stay_prob 0.3 spends most of its steps in layers 0 and 1: 600 walks from each of the 57 nodes leave every
# row of the two layers some thousands of stay steps (printed below).  The fixture's smallest positive weights of layers 0 and 1
# are 3.7e-3 and 9.3e-21: no walk count gives a cell like the latter 650 expected visits, and the rule does not need it -- its
# 1 / n term covers a cell that is expected, and seen, 0 times.
WALKS_PER_NODE, LENGTH, STAY, SEED = 600, 12, 0.3, 29


@pytest.fixture(scope="module")
def golden():
    return load_golden(GOLDEN)


@pytest.fixture(scope="module")
def restated(golden):
    return [sref.build(golden["rowptr"], golden["col"], *s) for s in sref.SETTINGS]


def ragged_lists(lists, n_layers, count_one):
    ptr, deg, cnt = [0], [], []
    for levels in lists:
        for l in range(n_layers):
            for d, c in (levels[l] if l < len(levels) else []):
                deg.append(d)
                cnt.append(c)
            ptr.append(len(deg))
    return np.array(ptr), np.array(deg), np.array(cnt)


def sorted_rows(rowptr, col, w):
    """Every row's (col, weight) entries sorted: rows compare as multisets."""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    order = np.lexsort((w, col, rows))
    return np.asarray(col)[order], np.asarray(w)[order]


@pytest.mark.parametrize("case", [0, 1, 2])
def test_restatement_reproduces_the_reference(golden, restated, case):
    assert [tuple(s) for s in golden.meta["settings"]] == sref.SETTINGS
    lists, pairs, dist, ctx = restated[case]
    n_layers = golden.meta["n_layers"][case]
    assert dist.shape[1] == n_layers
    ptr, deg, cnt = ragged_lists(lists, n_layers, not sref.SETTINGS[case][0])
    assert np.array_equal(ptr, golden["lists_ptr_%d" % case])
    assert np.array_equal(deg, golden["lists_deg_%d" % case]) and np.array_equal(cnt, golden["lists_cnt_%d" % case])
    assert np.array_equal(np.array(pairs), golden["pairs_%d" % case])
    want = golden["dist_%d" % case]
    assert np.array_equal(dist < 0, want < 0)
    np.testing.assert_allclose(dist, want, rtol=1e-12, atol=0)
    assert np.array_equal(ctx["rowptr"], golden["nb_ptr_%d" % case])
    col, w = sorted_rows(ctx["rowptr"], ctx["col"], ctx["norm"])
    gcol, gw = sorted_rows(golden["nb_ptr_%d" % case], golden["nb_col_%d" % case], golden["nb_w_%d" % case])
    assert np.array_equal(col, gcol)
    np.testing.assert_allclose(w, gw, rtol=1e-12, atol=1e-18)       # atol: only for weights the reference's exp(-d) rounds to 0
    assert np.array_equal(ctx["gamma"], golden["gamma_%d" % case])
    np.testing.assert_allclose(ctx["average"], golden["average_%d" % case], rtol=1e-12)


def test_fixture_has_the_promised_shape(golden):
    deg = np.diff(golden["rowptr"])
    assert deg.min() == 1 and deg.max() >= 20
    pairs = set(map(tuple, golden["pairs_0"].tolist()))
    assert any((b, a) in pairs for a, b in pairs)
    n, m = golden.meta["n_nodes"], golden.meta["motif"]
    for i in range(3):
        filled = np.diff(golden["nb_ptr_%d" % i]).reshape(-1, n).sum(axis=1)
        assert (filled > 0).sum() >= 3
    # the two copies are isomorphic under v -> v + motif
    rowptr, col = golden["rowptr"], golden["col"]
    for v in range(m):
        assert np.array_equal(col[rowptr[v]:rowptr[v + 1]] + m, col[rowptr[v + m]:rowptr[v + m + 1]])


def test_dtw_is_symmetric_and_zero_on_the_diagonal():
    rng = np.random.default_rng(3)
    for m, n in [(1, 1), (3, 65), (64, 129)]:
        a = sorted((int(d), int(c)) for d, c in zip(rng.integers(0, 10 ** 6, m), rng.integers(1, 10 ** 3, m)))
        b = sorted((int(d), int(c)) for d, c in zip(rng.integers(0, 10 ** 6, n), rng.integers(1, 10 ** 3, n)))
        assert sref.dtw(a, a) == 0.0 and sref.dtw(a, b) == sref.dtw(b, a)


def test_package_pair_selection_equals_the_restatement(golden):
    from dgll_amd.embedding.struc2vec import select_pairs, up_thresholds

    deg = np.diff(golden["rowptr"])
    for case, opt2 in [(0, True), (2, False)]:
        assert np.array_equal(select_pairs(deg, opt2), golden["pairs_%d" % case])
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 64, 257):
        d = rng.integers(0, 9, n)
        assert np.array_equal(select_pairs(d, True).reshape(-1, 2), np.array(sref.select_pairs(d, True), dtype=np.int32).reshape(-1, 2))
    g = np.arange(0, 50)
    t = up_thresholds(g)
    assert t.dtype == np.uint32 and np.array_equal(t, sref.up_thresholds(g)) and t[0] == 2 ** 31


def test_restated_walker_follows_the_reference_weights(golden, restated):
    _, _, _, ctx = restated[0]
    n, L = ctx["n_nodes"], ctx["n_layers"]
    T, alias = wref.build_alias(ctx["rowptr"], ctx["shifted"].astype(np.float32))
    t_up = sref.up_thresholds(ctx["gamma"])
    starts = np.repeat(np.arange(n, dtype=np.int64), WALKS_PER_NODE)
    moves = np.zeros((2, L * n), dtype=np.int64)
    wk, lay, capped = sref.walks(ctx["rowptr"], ctx["col"], T, alias, t_up, n, L, starts, LENGTH, STAY, seed=SEED, moves=moves)
    assert capped == 0 and (wk >= 0).all() and lay.max() >= 2
    cells, P = sref.stay_cells(golden["nb_ptr_0"], golden["nb_col_0"], golden["nb_w_0"], n)
    count, visits = sref.stay_frequencies(wk, lay, cells, n)
    checked, mass, excess = sref.frequency_excess(count, visits, P)
    print("stay steps: %d of %d cells checked, fewest stay steps of a row %d, worst excess over the cap %.3g"
          % (checked, mass, visits.min(), excess))
    assert excess <= 0.0
    rows = np.arange(2 * n)                                                    # up-moves: the rows of layers 0 and 1
    checked, mass, excess = sref.frequency_excess(moves[1, rows], moves[0, rows], sref.up_probability(golden["gamma_0"][rows]))
    print("up-moves: %d of %d rows checked, fewest move attempts %d, worst excess over the cap %.3g"
          % (checked, mass, moves[0, rows].min(), excess))
    assert excess <= 0.0


def test_restated_walker_cap_and_stay_limits(restated):
    _, _, _, ctx = restated[0]
    n, L = ctx["n_nodes"], ctx["n_layers"]
    T, alias = wref.build_alias(ctx["rowptr"], ctx["shifted"].astype(np.float32))
    t_up = sref.up_thresholds(ctx["gamma"])
    starts = np.arange(n, dtype=np.int64)
    wk, lay, capped = sref.walks(ctx["rowptr"], ctx["col"], T, alias, t_up, n, L, starts, 9, 0.3, seed=1, max_attempts=1)
    assert capped == n * 8 and (lay == 0).all() and (wk >= 0).all()
    wk, lay, capped = sref.walks(ctx["rowptr"], ctx["col"], T, alias, t_up, n, L, starts, 9, 1.0, seed=1)
    assert capped == 0 and (lay == 0).all()


def test_constructor_defaults_and_argument_checks():
    """What can be checked without a device: the signature, and that nothing runs on a CPU graph."""
    import inspect

    import torch

    import dgll_amd
    from dgll_amd.embedding import RandomWalkEmbedding, Struc2Vec, StrucContext, struc_walks

    assert issubclass(Struc2Vec, RandomWalkEmbedding)
    sig = inspect.signature(Struc2Vec.__init__)
    want = dict(verbose=0, stay_prob=0, opt1_reduce_len=True, opt2_reduce_sim_calc=True, opt3_num_layers=None)
    assert {k: sig.parameters[k].default for k in want} == want
    assert "temp_path" in sig.parameters and "reuse" in sig.parameters
    assert list(inspect.signature(struc_walks).parameters)[:8] == ["ctx", "starts", "length", "stay_prob", "seed", "first_walk_index",
                                                                    "info", "return_layers"]
    g = dgll_amd.CSRGraph.from_coo(torch.tensor([0, 1]), torch.tensor([1, 0]), None, (2, 2))
    with pytest.raises(RuntimeError, match="GPU only"):
        StrucContext.from_graph(g)
    with pytest.raises(RuntimeError, match="GPU only"):
        struc_walks(None, torch.zeros(1, dtype=torch.int64), 3, 0.3, 0, 0)
    with pytest.warns(UserWarning, match="Provide a graph"), pytest.raises(SystemExit):
        Struc2Vec(None)


def test_argument_validation_needs_no_gpu():
    from dgll_amd import _lib

    assert _lib.lib.dgll_hip_struc_dtw_max_rows() == 1024
    code = _lib.lib.dgll_hip_struc_dtw(None, None, None, None, 4, 2, None, 1, None)
    assert code == -1 and "non-NULL" in _lib.last_error()
    code = _lib.lib.dgll_hip_struc_walk(None, 8, 8, 8, 8, 4, 2, 8, 1, 5, 0, 0, 1.5, 1024, 8, None, 8)
    assert code == -1 and "stay_prob" in _lib.last_error()
    code = _lib.lib.dgll_hip_struc_walk(None, 8, 8, 8, 8, 4, 2, 8, 1, 5, 0, 0, 0.3, 0, 8, None, 8)
    assert code == -1 and "attempt cap" in _lib.last_error()


def test_dgll_namespace_exports_struc2vec():
    import dgll.embedding
    from dgll.embedding import Struc2Vec  # noqa: F401
    from dgll_amd import embedding

    assert dgll.embedding.Struc2Vec is embedding.Struc2Vec
