"""dgll_amd.embedding without a GPU: the numpy Philox against the library's, argument validation of the new C-ABI functions, the
restated walker's node2vec transition frequencies against the reference's probabilities (tests/golden/node2vec_probs.npz), and
the float64 restatement of the whole trainer on a planted partition."""
import ctypes as C

import numpy as np
import pytest

import embedding_ref as ref
from conftest import load_golden


def test_numpy_philox_equals_the_library():
    from dgll_amd import _lib

    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, (64, 4), dtype=np.uint64).astype(np.uint32)
    ctr[0] = 0
    ctr[1] = 0xFFFFFFFF
    for key in ((0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0xA4093822, 0x299F31D0)):
        mine = ref.philox4x32_10(ctr, key)
        k = (C.c_uint32 * 2)(*key)
        for i in range(len(ctr)):
            c, out = (C.c_uint32 * 4)(*[int(x) for x in ctr[i]]), (C.c_uint32 * 4)()
            assert _lib.lib.dgll_host_philox4x32_10(c, k, out) == 0
            assert list(out) == [int(x) for x in mine[i]], (key, i)
    # Random123's known-answer vector for the all-ones counter and key
    assert [hex(int(x)) for x in ref.philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))[0]] == \
        ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]


def test_thresholds_equal_the_library():
    from dgll_amd import _lib

    for p, q in ((1.0, 1.0), (0.5, 2.0), (4.0, 0.25), (0.5, 0.8), (3.0, 7.0)):
        out = (C.c_uint64 * 3)()
        assert _lib.lib.dgll_host_node2vec_thresholds(p, q, out) == 0
        assert list(out) == [int(x) for x in ref.thresholds(p, q)]
    assert max(int(x) for x in ref.thresholds(0.5, 2.0)) == 2 ** 32


def test_argument_validation_needs_no_gpu():
    from dgll_amd import _lib

    lib = _lib.lib
    buf = (C.c_int64 * 8)()
    a = C.addressof(buf)
    good = dict(rowptr=a, col=a, n_nodes=4, starts=a, n=2, length=3, first=0, seed=0, p=1.0, q=1.0, cap=1024, walks=a, info=a)

    def walk(**kw):
        k = dict(good, **kw)
        return lib.dgll_hip_random_walk(None, k["rowptr"], k["col"], k["n_nodes"], k["starts"], k["n"], k["length"], k["first"], k["seed"],
                                        k["p"], k["q"], k["cap"], k["walks"], k["info"])

    for kw, word in ((dict(rowptr=None), "NULL"), (dict(walks=None), "NULL"), (dict(info=None), "NULL"), (dict(length=0), "length"),
                     (dict(p=0.0), "p and q"), (dict(p=-1.0), "p and q"), (dict(q=0.0), "p and q"), (dict(cap=8), "1024")):
        assert walk(**kw) == -1 and word in _lib.last_error(), (kw, _lib.last_error())
    out = (C.c_uint64 * 3)()
    assert lib.dgll_host_node2vec_thresholds(0.0, 1.0, out) == -1 and "p and q" in _lib.last_error()
    assert lib.dgll_hip_sgns_negatives(None, None, 1, 4, 1, 1, a, 4, 0, 0, a) == -1 and "NULL" in _lib.last_error()
    assert lib.dgll_hip_sgns_negatives(None, a, 1, 4, 0, 1, a, 4, 0, 0, a) == -1 and "window" in _lib.last_error()
    assert lib.dgll_hip_sgns_step(None, None, a, 4, 2, a, 1, 4, 1, 1, a, 0, 0, 0.1, a, a, a, a) == -1 and "NULL" in _lib.last_error()
    assert lib.dgll_hip_sgns_step(None, a, a, 4, 0, a, 1, 4, 1, 1, a, 0, 0, 0.1, a, a, a, a) == -1 and "dimension" in _lib.last_error()


def test_python_layer_refuses_cpu_tensors():
    import torch

    import dgll_amd
    from dgll_amd import embedding

    g = dgll_amd.CSRGraph.from_coo(torch.tensor([0, 1]), torch.tensor([1, 0]), None, (2, 2))
    with pytest.raises(RuntimeError):
        embedding.random_walks(g, torch.tensor([0, 1]), 4)
    noise = embedding.NoiseTable([1.0, 1.0])
    with pytest.raises(RuntimeError):
        embedding.sgns_step(torch.rand(2, 4), torch.rand(2, 4), torch.zeros((1, 3), dtype=torch.int32), 1, 1, noise, 0.1, 0)
    with pytest.raises(RuntimeError):
        embedding.sgns_negatives(torch.zeros((1, 3), dtype=torch.int32), 1, 1, noise, 0)


def test_noise_table_is_the_restated_cdf():
    from dgll_amd import embedding

    w = np.array([0.0, 3.0, 0.0, 1.0, 5.0, 0.0, 0.0])
    cdf = embedding.NoiseTable(w).cdf.numpy().astype(np.uint64)
    assert np.array_equal(cdf, ref.noise_cdf(w)) and cdf[-1] == 2 ** 32
    draws = np.searchsorted(cdf, np.arange(0, 2 ** 32, 65537, dtype=np.uint64), side="right")
    assert set(draws.tolist()) == {1, 3, 4}


def transition_check(golden, walk_arr, case):
    """The distribution rule both the host and the device test apply: conditional frequencies of step 3 given (t, v) against the
    reference's probabilities, cap 5 sqrt(P (1 - P) / n) + 1 / n per cell, cells with n >= 500 only, and at least 90 % of the cells
    that have probability mass must qualify.  Returns (cells checked, cells with mass, worst excess over the cap)."""
    rowptr, col, prob_ptr = golden["rowptr"], golden["col"].astype(np.int64), golden["prob_ptr"]
    probs = golden["probs_%d" % case]
    n_nodes = len(rowptr) - 1
    edge_key = np.repeat(np.arange(n_nodes), np.diff(rowptr)) * n_nodes + col
    w = np.asarray(walk_arr, dtype=np.int64)
    w = w[w[:, 2] >= 0]
    e1 = np.searchsorted(edge_key, w[:, 0] * n_nodes + w[:, 1])               # edge (t, v)
    e2 = np.searchsorted(edge_key, w[:, 1] * n_nodes + w[:, 2])               # edge (v, x)
    assert np.array_equal(edge_key[e1], w[:, 0] * n_nodes + w[:, 1]) and np.array_equal(edge_key[e2], w[:, 1] * n_nodes + w[:, 2])
    cell = prob_ptr[e1] + (e2 - rowptr[w[:, 1]])                              # x's rank among v's out-neighbours
    count = np.bincount(cell, minlength=len(probs)).astype(np.float64)
    n_edge = np.bincount(e1, minlength=len(col)).astype(np.float64)
    n_cell = np.repeat(n_edge, np.diff(prob_ptr))
    mass = probs > 0
    assert not count[~mass].any(), "a transition of probability 0 was taken"
    ok = mass & (n_cell >= 500)
    assert ok.sum() >= 0.9 * mass.sum(), (int(ok.sum()), int(mass.sum()))
    P, n = probs[ok], n_cell[ok]
    excess = np.abs(count[ok] / n - P) - (5.0 * np.sqrt(P * (1.0 - P) / n) + 1.0 / n)
    return int(ok.sum()), int(mass.sum()), float(excess.max())


def golden_starts(golden):
    return np.repeat(np.arange(len(golden["start_reps"]), dtype=np.int64), golden["start_reps"])


@pytest.mark.parametrize("case", [0, 1])
def test_restated_walker_follows_the_reference_probabilities(case):
    golden = load_golden("node2vec_probs")
    p, q = golden.meta["pq"][case]
    starts = golden_starts(golden)
    assert len(starts) == golden.meta["n_walks"] == 200_000
    wk, capped = ref.walks(golden["rowptr"], golden["col"], starts, 3, p, q, seed=golden.meta["seed"], return_capped=True)
    assert capped == 0
    checked, mass, excess = transition_check(golden, wk, case)
    print("p=%g q=%g: %d of %d cells checked, worst excess over the cap %.3g" % (p, q, checked, mass, excess))
    assert excess <= 0.0


def test_fixture_graph_has_the_promised_shape():
    golden = load_golden("node2vec_probs")
    deg = np.diff(golden["rowptr"])
    assert deg[golden.meta["hub"]] >= 100
    assert deg[golden.meta["sink"]] == 0 and (golden["col"] == golden.meta["sink"]).any()
    assert deg[golden.meta["isolated"]] == 0 and not (golden["col"] == golden.meta["isolated"]).any()
    for i in range(2):              # every (t, v) block of probabilities sums to 1 (or is empty: v is a dead end)
        sums = np.add.reduceat(np.append(golden["probs_%d" % i], 0.0), golden["prob_ptr"][:-1])
        sizes = np.diff(golden["prob_ptr"])
        np.testing.assert_allclose(sums[sizes > 0], 1.0, rtol=1e-12)


def test_float64_trainer_separates_a_planted_partition():
    rowptr, col, comm = ref.planted_partition()
    emb, losses = ref.train_host(rowptr, col)
    intra, inter = ref.cosine_split(emb, comm)
    print("host trainer: intra %.4f inter %.4f losses %s" % (intra, inter, ["%.1f" % x for x in losses]))
    assert intra > inter
    assert losses[-1] < losses[0]


def test_dgll_namespace_resolves_the_package():
    import dgll
    import dgll.embedding
    from dgll_amd import embedding

    assert dgll.embedding is embedding
    from dgll.embedding import DeepWalk, Node2vec, SkipGramModel  # noqa: F401
