"""struc2vec on the device: the DTW kernel against the float64 host DP, the context graph against the fixture recorded from the
reference, the multilayer walk bit for bit against the restatement, and the trainer end to end."""
import numpy as np
import pytest
import torch

import embedding_ref as ref
import struc2vec_ref as sref
import weighted_walk_ref as wref
from conftest import load_golden
from test_struc2vec_host import LENGTH, SEED, STAY, WALKS_PER_NODE, ragged_lists, sorted_rows

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 63, 64, 65, 129, 300)
# the end-to-end run: as embedding_ref.TRAIN with 4 walks per vertex, 10 epochs and a tenth of its lr -- the context graph's walks
# return to the same few structurally close nodes, a batch's summed gradients are that much larger, and at lr 0.005 the float64
# host trainer diverges
E2E = dict(dim=16, length=20, window=3, negatives=5, walks_per_vertex=4, lr=0.0005, batch_walks=19, epochs=10, seed=7, stay_prob=0.3)


@pytest.fixture(scope="module")
def golden():
    return load_golden("struc2vec_context")


@pytest.fixture(scope="module")
def csr(golden, cuda_device):
    import dgll_amd

    return dgll_amd.CSRGraph(golden.t("rowptr", cuda_device), golden.t("col", cuda_device), None, golden.meta["n_nodes"],
                             golden.meta["n_nodes"])


@pytest.fixture(scope="module")
def contexts(csr):
    from dgll_amd.embedding import StrucContext

    return [StrucContext.from_graph(csr, *s) for s in sref.SETTINGS]


@pytest.fixture(scope="module")
def tables(contexts):
    """Setting 0's device tables on the host: what the restated walker is fed."""
    ctx = contexts[0]
    T, alias = ctx.alias.numpy()
    return dict(rowptr=ctx.graph.rowptr.cpu().numpy(), col=ctx.graph.col.cpu().numpy(), T=T, alias=alias,
                t_up=ctx.t_up.cpu().numpy().view(np.uint32), n=ctx.n_nodes, L=ctx.n_layers)


def host_walks(tb, starts, length, stay, seed, first=0, max_attempts=ref.MAX_ATTEMPTS):
    return sref.walks(tb["rowptr"], tb["col"], tb["T"], tb["alias"], tb["t_up"], tb["n"], tb["L"], starts, length, stay, seed=seed,
                      first_walk_index=first, max_attempts=max_attempts)


# ---- the DTW kernel ------------------------------------------------------------------------------------------------------------
def random_sequence(rng, n):
    deg = np.sort(rng.choice(10 ** 6 + 1, n, replace=False))
    return [(int(d), int(c)) for d, c in zip(deg, rng.integers(1, 10 ** 3 + 1, n))]


@pytest.fixture(scope="module")
def dtw_case(cuda_device):
    """17 nodes, 2 levels.  Level 0: nodes 0..7 and 8..15 hold one random sequence of every length in LENGTHS each, node 16 none.
    Level 1: nodes 0..7 hold a short sequence, the others none.  Pairs: every (i, 8 + j) and its reverse, every (i, i), (0, 16)."""
    from dgll_amd.embedding import DegreeSequences, struc_dtw

    rng = np.random.default_rng(17)
    level0 = [random_sequence(rng, n) for n in LENGTHS] + [random_sequence(rng, n) for n in LENGTHS] + [[]]
    level1 = [random_sequence(rng, 2 + i % 2) for i in range(8)] + [[] for _ in range(9)]
    lists = [[a, b] for a, b in zip(level0, level1)]
    ptr, deg, cnt = [0], [], []
    for levels in lists:
        for seq in levels:
            deg += [d for d, _ in seq]
            cnt += [c for _, c in seq]
            ptr.append(len(deg))
    seqs = DegreeSequences(torch.tensor(ptr, dtype=torch.int64, device=cuda_device), torch.tensor(deg, dtype=torch.int32, device=cuda_device),
                           torch.tensor(cnt, dtype=torch.int32, device=cuda_device), 17, 2)
    pairs = [(i, 8 + j) for i in range(8) for j in range(8)] + [(8 + j, i) for i in range(8) for j in range(8)] + \
            [(i, i) for i in range(16)] + [(0, 16), (16, 0)]
    dist = struc_dtw(seqs, torch.tensor(pairs, dtype=torch.int32, device=cuda_device)).cpu().numpy()
    return lists, pairs, dist


def test_dtw_equals_the_float64_host_dp(dtw_case):
    lists, pairs, dist = dtw_case
    worst = 0.0
    for p, (a, b) in enumerate(pairs[:64]):
        want = sref.dtw(lists[a][0], lists[b][0])
        worst = max(worst, abs(dist[p, 0] - want) / want)
        assert dist[p, 1] == -1.0                                              # node 8 + j has no level 1
    print("DTW, %d tasks of up to 300 x 300 cells: worst relative error %.3g" % (64, worst))
    assert worst <= 1e-12


def test_dtw_symmetry_diagonal_and_invalid_levels(dtw_case):
    lists, pairs, dist = dtw_case
    assert np.array_equal(dist[:64, 0].view(np.int64), dist[64:128, 0].view(np.int64))          # d(a, b) and d(b, a): the same bits
    diag = dist[128:144]
    assert (diag[:, 0] == 0.0).all() and (diag[:8, 1] == 0.0).all() and (diag[8:, 1] == -1.0).all()
    assert (dist[144:] == -1.0).all()                                          # an empty partner, in either order


def test_dtw_refuses_sequences_the_strip_buffer_cannot_hold(cuda_device):
    from dgll_amd.embedding import DegreeSequences, struc_dtw

    n = 1025
    seqs = DegreeSequences(torch.tensor([0, n, 2 * n, 2 * n + 3], dtype=torch.int64, device=cuda_device),
                           torch.arange(2 * n + 3, dtype=torch.int32, device=cuda_device) % n,
                           torch.ones(2 * n + 3, dtype=torch.int32, device=cuda_device), 3, 1)
    with pytest.raises(ValueError, match="1024"):
        struc_dtw(seqs, torch.tensor([[0, 1]], dtype=torch.int32, device=cuda_device))
    d = struc_dtw(seqs, torch.tensor([[0, 2]], dtype=torch.int32, device=cuda_device)).cpu().numpy()       # the shorter one is 3 long
    want = sref.dtw([(i, 1) for i in range(n)], [(0, 1), (1, 1), (2, 1)])
    assert abs(d[0, 0] - want) <= 1e-12 * want


# ---- the context graph ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 1, 2])
def test_context_graph_equals_the_reference(golden, contexts, case):
    ctx = contexts[case]
    n, n_layers = golden.meta["n_nodes"], golden.meta["n_layers"][case]
    assert (ctx.n_nodes, ctx.n_layers) == (n, n_layers)
    ptr, deg, cnt = ragged_lists(ctx.seqs.tolist(), n_layers, False)
    assert np.array_equal(ctx.seqs.seq_ptr.cpu().numpy(), golden["lists_ptr_%d" % case]) and np.array_equal(ptr, golden["lists_ptr_%d" % case])
    assert np.array_equal(deg, golden["lists_deg_%d" % case]) and np.array_equal(cnt, golden["lists_cnt_%d" % case])
    assert np.array_equal(ctx.pairs.cpu().numpy(), golden["pairs_%d" % case])
    dist, want = ctx.dist.cpu().numpy(), golden["dist_%d" % case]
    assert np.array_equal(dist < 0, want < 0)
    np.testing.assert_allclose(dist, want, rtol=1e-12, atol=0)
    rowptr, col = ctx.graph.rowptr.cpu().numpy(), ctx.graph.col.cpu().numpy()
    g_ptr, g_col, g_w = golden["nb_ptr_%d" % case], golden["nb_col_%d" % case], golden["nb_w_%d" % case]
    assert np.array_equal(rowptr, g_ptr)
    c1, w1 = sorted_rows(rowptr, col, ctx.norm_weights.cpu().numpy())
    c2, w2 = sorted_rows(g_ptr, g_col, g_w)
    assert np.array_equal(c1, c2)
    np.testing.assert_allclose(w1, w2, rtol=1e-12, atol=1e-18)
    # val: the float32 cast of exp(-(d - row minimum)) = the golden's normalised weight over the largest of its row
    rows = np.repeat(np.arange(len(g_ptr) - 1), np.diff(g_ptr))
    top = np.zeros(len(g_ptr) - 1)
    np.maximum.at(top, rows, g_w)
    _, v1 = sorted_rows(rowptr, col, ctx.graph.val.cpu().numpy().astype(np.float64))
    _, v2 = sorted_rows(g_ptr, g_col, g_w / top[rows])
    assert np.abs(v1 - v2).max() <= 1e-6
    assert np.array_equal(ctx.gamma.cpu().numpy(), golden["gamma_%d" % case])
    assert np.array_equal(ctx.t_up.cpu().numpy().view(np.uint32), sref.up_thresholds(golden["gamma_%d" % case]))
    np.testing.assert_allclose(ctx.layer_average.cpu().numpy(), golden["average_%d" % case], rtol=1e-12)
    # the alias table implies the float32 weights' distribution
    T, alias = ctx.alias.numpy()
    val = ctx.graph.val.cpu().numpy().astype(np.float64)
    want_p = val / np.bincount(rows, weights=val, minlength=len(g_ptr) - 1)[rows]
    assert np.abs(wref.implied_probs(rowptr, T, alias) - want_p).max() <= 2.0 ** -30


# ---- the walk ------------------------------------------------------------------------------------------------------------------
def test_walks_and_layers_are_bit_equal_to_the_restatement(contexts, tables, cuda_device):
    from dgll_amd.embedding import struc_walks, walk_info

    n = tables["n"]
    starts = np.tile(np.arange(n, dtype=np.int64), 6)                          # 342 walks: more than one block
    info = torch.zeros(2, dtype=torch.int64, device=cuda_device)
    dev_starts = torch.from_numpy(starts).to(cuda_device)
    wk, lay = struc_walks(contexts[0], dev_starts, 25, 0.3, 123, 1000, info=info, return_layers=True)
    want_wk, want_lay, capped = host_walks(tables, starts, 25, 0.3, 123, first=1000)
    assert np.array_equal(wk.cpu().numpy(), want_wk) and np.array_equal(lay.cpu().numpy(), want_lay)
    assert walk_info(info) == capped == 0 and want_lay.max() >= 2
    # whatever the batch split
    parts = [struc_walks(contexts[0], dev_starts[a:b], 25, 0.3, 123, 1000 + a) for a, b in [(0, 1), (1, 100), (100, 342)]]
    assert torch.equal(torch.cat(parts), wk)
    assert torch.equal(struc_walks(contexts[0], dev_starts, 25, 0.3, 123, 1000), wk)              # without layers_out


def test_walk_cap_and_stay_limits(contexts, tables, cuda_device):
    from dgll_amd.embedding import struc_walks, walk_info

    n = tables["n"]
    starts = np.arange(n, dtype=np.int64)
    dev_starts = torch.from_numpy(starts).to(cuda_device)
    info = torch.zeros(2, dtype=torch.int64, device=cuda_device)
    wk, lay = struc_walks(contexts[0], dev_starts, 9, 0.3, 5, 0, info=info, return_layers=True, max_attempts=1)
    want_wk, want_lay, capped = host_walks(tables, starts, 9, 0.3, 5, max_attempts=1)
    assert np.array_equal(wk.cpu().numpy(), want_wk) and (lay == 0).all() and (wk >= 0).all()
    assert walk_info(info) == capped == n * 8                                  # every step stayed at its only attempt
    for stay in (1.0, 1.0 - 1e-10):
        wk, lay = struc_walks(contexts[0], dev_starts, 30, stay, 5, 0, return_layers=True)
        assert (lay == 0).all() and (wk >= 0).all()
    bad = torch.tensor([0, n, -1], dtype=torch.int64, device=cuda_device)
    info.zero_()
    wk = struc_walks(contexts[0], bad, 4, 0.3, 5, 0, info=info)
    assert (wk[1:] == -1).all() and (wk[0] >= 0).all()
    with pytest.raises(RuntimeError, match="start node"):
        walk_info(info)


def test_device_walks_follow_the_reference_weights(golden, contexts, cuda_device):
    from dgll_amd.embedding import struc_walks

    n = golden.meta["n_nodes"]
    starts = torch.arange(n, dtype=torch.int64, device=cuda_device).repeat_interleave(WALKS_PER_NODE)
    wk, lay = struc_walks(contexts[0], starts, LENGTH, STAY, SEED, 0, return_layers=True)
    cells, P = sref.stay_cells(golden["nb_ptr_0"], golden["nb_col_0"], golden["nb_w_0"], n)
    count, visits = sref.stay_frequencies(wk.cpu().numpy(), lay.cpu().numpy(), cells, n)
    checked, mass, excess = sref.frequency_excess(count, visits, P)
    print("device stay steps: %d of %d cells checked, worst excess over the cap %.3g" % (checked, mass, excess))
    assert excess <= 0.0


def test_walks_cross_between_the_isomorphic_copies(golden, contexts, csr, cuda_device):
    from dgll_amd.embedding import random_walks, struc_walks

    m = golden.meta["motif"]
    starts = torch.arange(m, dtype=torch.int64, device=cuda_device).repeat(20)
    wk = struc_walks(contexts[0], starts, 20, 0.3, 3, 0)
    assert bool(((wk >= m) & (wk < 2 * m)).any())
    plain = random_walks(csr, starts, 20, seed=3)
    assert bool((plain < m).all())


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def mirror_split(emb, m):
    """(mean cosine over the mirror pairs (v, v + m), mean over all cross-copy pairs)."""
    e = np.asarray(emb, dtype=np.float64)[:2 * m]
    e = e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-30)
    sim = e[:m] @ e[m:].T
    return float(np.diag(sim).mean()), float(sim.mean())


def test_struc2vec_embeds_mirror_nodes_together(golden, csr, cuda_device):
    """Host check of the same configuration (embedding_ref.train_host's loop fed the restated struc2vec walks, float64): mirror
    pairs 0.6774, all cross-copy pairs 0.5425 after the 10 epochs, the gap growing from epoch 4 on."""
    from dgll_amd.embedding import SkipGramModel, Struc2Vec

    cfg = E2E
    torch.manual_seed(cfg["seed"])
    s2v = Struc2Vec(csr, cfg["length"], cfg["dim"], cfg["walks_per_vertex"], cfg["window"], cfg["lr"], stay_prob=cfg["stay_prob"],
                    opt3_num_layers=3, negatives=cfg["negatives"], batch_walks=cfg["batch_walks"], seed=cfg["seed"])
    model = SkipGramModel(s2v.totalNodes, cfg["dim"], device=cuda_device)
    for _ in range(cfg["epochs"]):
        s2v.learnNodeEmbedding(model)
    assert s2v.last_capped == 0 and s2v.losses[-1] < s2v.losses[0]
    mirror, cross = mirror_split(model.W1.data.cpu().numpy(), golden.meta["motif"])
    print("struc2vec on the device: mirror pairs %.4f, all cross-copy pairs %.4f, losses %.1f -> %.1f"
          % (mirror, cross, s2v.losses[0], s2v.losses[-1]))
    assert mirror > cross
    assert len(s2v.RandomWalk(0, 10)) == 10
    assert s2v.getEdgeEmbedding(0, 1).shape == (cfg["dim"],)


def test_constructor_defaults_and_warnings(csr):
    from dgll_amd.embedding import Struc2Vec

    with pytest.warns(UserWarning) as rec:
        s2v = Struc2Vec(csr, 0, 0, 0, 0, 0, opt3_num_layers=1, temp_path="./nowhere/", reuse=True, seed=1)
    text = " ".join(str(w.message) for w in rec)
    assert "Set stay prob. to default: 0.3" in text and "Set Walk to default" in text
    assert s2v.stay_prob == 0.3 and s2v.walkLength == 3 and s2v.context.n_layers == 2
    import os

    assert not os.path.exists("./nowhere/")
