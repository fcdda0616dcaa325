"""dgll_amd.embedding on the device: walks bit-equal to the numpy restatement, independent of the batching and distributed as the
reference's node2vec probabilities; negatives equal to the restatement; one skip-gram step against the float64 oracle; DeepWalk
and Node2vec end to end on a planted partition; the reference's interface.  No test reads the reference tree."""
import warnings

import numpy as np
import pytest
import torch

import embedding_ref as ref
from conftest import load_golden
from test_embedding_host import golden_starts, transition_check

pytestmark = pytest.mark.gpu

PQ = [(1.0, 1.0), (0.5, 2.0), (4.0, 0.25)]
GRAD_BAR = 1e-3          # the project's fp32 gradient bar: relative L2


def _csr(rowptr, col, dev):
    import dgll_amd

    return dgll_amd.CSRGraph(torch.from_numpy(np.asarray(rowptr, np.int64)), torch.from_numpy(np.asarray(col, np.int32)), None,
                             len(rowptr) - 1, len(rowptr) - 1).to(dev)


@pytest.fixture(scope="module")
def golden():
    return load_golden("node2vec_probs")


@pytest.fixture(scope="module")
def golden_graph(golden, cuda_device):
    return _csr(golden["rowptr"], golden["col"], cuda_device)


# ---- walks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q", PQ)
def test_walks_equal_the_restatement(golden, golden_graph, cuda_device, p, q):
    from dgll_amd import embedding

    rowptr, col = golden["rowptr"], golden["col"]
    n_nodes = len(rowptr) - 1
    starts = np.tile(np.arange(n_nodes, dtype=np.int64), 3)
    info = torch.zeros(2, dtype=torch.int64, device=cuda_device)
    got = embedding.random_walks(golden_graph, torch.from_numpy(starts).to(cuda_device), 12, p=p, q=q, seed=1234, info=info).cpu().numpy()
    want, capped = ref.walks(rowptr, col, starts, 12, p, q, seed=1234, return_capped=True)
    assert got.dtype == np.int32 and got.shape == (len(starts), 12)
    assert np.array_equal(got, want)
    assert embedding.walk_info(info) == capped == 0
    assert np.array_equal(got[:, 0], starts)
    deg = np.diff(rowptr)
    edges = set(zip(np.repeat(np.arange(n_nodes), deg).tolist(), col.tolist()))
    for w in got:
        for a, b in zip(w[:-1], w[1:]):
            if b >= 0:
                assert (int(a), int(b)) in edges
            else:
                assert a < 0 or deg[a] == 0          # -1 only after a dead end, and it is sticky
    iso = golden.meta["isolated"]
    assert all(np.array_equal(w, [iso] + [-1] * 11) for w in got[starts == iso])
    assert (got[:, 1:] >= 0).mean() > 0.3           # the walks do go somewhere


@pytest.mark.parametrize("p,q", PQ[:2])
def test_walks_do_not_depend_on_the_batching(golden_graph, cuda_device, p, q):
    from dgll_amd import embedding

    n = 2 * golden_graph.n_rows
    starts = (torch.arange(n, device=cuda_device) * 7) % golden_graph.n_rows
    whole = embedding.random_walks(golden_graph, starts, 9, p=p, q=q, seed=5)
    lo = embedding.random_walks(golden_graph, starts[:n // 2], 9, p=p, q=q, seed=5, first_walk_index=0)
    hi = embedding.random_walks(golden_graph, starts[n // 2:], 9, p=p, q=q, seed=5, first_walk_index=n // 2)
    assert torch.equal(whole, torch.cat([lo, hi]))
    assert torch.equal(whole, embedding.random_walks(golden_graph, starts, 9, p=p, q=q, seed=5))
    assert not torch.equal(whole, embedding.random_walks(golden_graph, starts, 9, p=p, q=q, seed=6))


def test_biased_walks_refuse_unsorted_rows(cuda_device):
    from dgll_amd import embedding

    g = _csr([0, 2, 3, 4], [2, 1, 0, 0], cuda_device)
    starts = torch.zeros(4, dtype=torch.int64, device=cuda_device)
    assert embedding.random_walks(g, starts, 3).shape == (4, 3)           # uniform walks do not need the order
    with pytest.raises(ValueError):
        embedding.random_walks(g, starts, 3, p=0.5, q=2.0)


@pytest.mark.parametrize("case", [0, 1])
def test_device_walks_follow_the_reference_probabilities(golden, golden_graph, cuda_device, case):
    from dgll_amd import embedding

    p, q = golden.meta["pq"][case]
    starts = torch.from_numpy(golden_starts(golden)).to(cuda_device)
    info = torch.zeros(2, dtype=torch.int64, device=cuda_device)
    wk = embedding.random_walks(golden_graph, starts, 3, p=p, q=q, seed=golden.meta["seed"], info=info).cpu().numpy()
    assert embedding.walk_info(info) == 0
    checked, mass, excess = transition_check(golden, wk, case)
    print("p=%g q=%g: %d of %d cells checked, worst excess over the cap %.3g" % (p, q, checked, mass, excess))
    assert excess <= 0.0


# ---- skip-gram ------------------------------------------------------------------------------------------------------------------
N_STEP = 97


@pytest.fixture(scope="module")
def step_case(cuda_device):
    """A 97-node directed graph whose nodes 88..96 are isolated (never walked, noise weight 0: their rows must not change) and whose
    nodes 80..87 are sinks (walks through them end in -1 tails); 24 walks of 10 over 88 nodes repeat nodes within a batch."""
    from dgll_amd import embedding

    rng = np.random.default_rng(3)
    src = rng.integers(0, 80, 400)
    dst = rng.integers(0, 88, 400)
    g = __import__("dgll_amd").CSRGraph.from_coo(torch.from_numpy(src), torch.from_numpy(dst), None, (N_STEP, N_STEP)).to(cuda_device)
    starts = torch.from_numpy(rng.integers(0, 88, 24)).to(cuda_device)
    wk = embedding.random_walks(g, starts, 10, seed=9, first_walk_index=100)
    wk_np = wk.cpu().numpy()
    assert (wk_np == -1).any() and (wk_np[:, -1] >= 0).any() and wk_np.max() < 88
    assert any(len(set(w[w >= 0].tolist())) < (w >= 0).sum() for w in wk_np)          # a walk that repeats a node
    noise = embedding.NoiseTable.from_graph(g)
    assert noise.cdf.is_cuda
    return g, wk, wk_np, noise, noise.cdf.cpu().numpy().astype(np.uint64)


@pytest.mark.parametrize("window,k_neg", [(1, 1), (3, 5), (2, 70)])
def test_negatives_equal_the_restatement(step_case, window, k_neg):
    from dgll_amd import embedding

    g, wk, wk_np, noise, cdf = step_case
    got = embedding.sgns_negatives(wk, window, k_neg, noise, seed=21, first_walk_index=100).cpu().numpy()
    want = ref.negatives(wk_np, window, k_neg, cdf, 21, 100)
    assert got.shape == (24, 10, 2 * window, k_neg) and got.dtype == np.int32
    assert np.array_equal(got, want)
    assert np.array_equal(got[..., 0] < 0, ~ref.pair_mask(wk_np, window))             # -1 exactly where there is no pair
    indeg = np.bincount(g.col.cpu().numpy(), minlength=N_STEP)
    drawn = np.unique(got[got >= 0])
    assert (indeg[drawn] > 0).all() and len(drawn) > 20                               # never a node of zero noise weight


def _rel(a, b):
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


# D: 2 (4-lane groups), 16 (16-lane groups), 64 / 100 / 128 (a wavefront per centre, ragged at 100), 300 (the delta in LDS)
@pytest.mark.parametrize("k_neg", [1, 5])
@pytest.mark.parametrize("window", [1, 3])
@pytest.mark.parametrize("dim", [2, 16, 64, 100, 128, 300])
def test_one_step_against_the_float64_oracle(step_case, cuda_device, dim, window, k_neg):
    """The update of each table and the loss sum against the float64 oracle at the fp32 gradient bar, three chained steps; the test
    prints the errors it measures (DESIGN.md 6.2 has no recorded figures yet)."""
    from dgll_amd import embedding

    g, wk, wk_np, noise, cdf = step_case
    gen = torch.Generator().manual_seed(dim * 100 + window * 10 + k_neg)
    w_in = torch.rand((N_STEP, dim), generator=gen).to(cuda_device)
    w_out = torch.rand((N_STEP, dim), generator=gen).to(cuda_device)
    lr = 0.01
    for step in range(3):
        seed, first = 40 + step, 100 + 24 * step
        before_in, before_out = w_in.cpu().clone(), w_out.cpu().clone()
        loss = embedding.sgns_step(w_in, w_out, wk, window, k_neg, noise, lr, seed, first)
        negs = ref.negatives(wk_np, window, k_neg, cdf, seed, first)
        want_in, want_out, want_loss = ref.sgns_step(before_in, before_out, wk_np, window, negs, lr)
        assert loss.dtype == torch.float64 and loss.is_cuda
        err_loss = abs(float(loss) - want_loss) / abs(want_loss)
        upd_in, upd_out = w_in.cpu().double() - before_in.double(), w_out.cpu().double() - before_out.double()
        err_in, err_out = _rel(upd_in, want_in - before_in.double()), _rel(upd_out, want_out - before_out.double())
        print("D=%d W=%d K=%d step %d: rel L2 of the update W_in %.3g W_out %.3g, loss %.3g" % (dim, window, k_neg, step, err_in, err_out, err_loss))
        assert err_in <= GRAD_BAR and err_out <= GRAD_BAR and err_loss <= GRAD_BAR
        # rows no pair touches are bit-identical: the isolated nodes, and in W_in every node that is nowhere a centre
        assert torch.equal(w_in.cpu()[88:], before_in[88:]) and torch.equal(w_out.cpu()[88:], before_out[88:])
        untouched_in = (want_in == before_in.double()).all(dim=1)
        untouched_out = (want_out == before_out.double()).all(dim=1)
        assert untouched_in[88:].all() and untouched_out[88:].all()
        assert torch.equal(w_in.cpu()[untouched_in], before_in[untouched_in])
        assert torch.equal(w_out.cpu()[untouched_out], before_out[untouched_out])


# ---- end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["deepwalk", "node2vec"])
def test_end_to_end_separates_a_planted_partition(cuda_device, method):
    from dgll_amd import embedding

    rowptr, col, comm = ref.planted_partition()
    cfg = ref.TRAIN
    g = _csr(rowptr, col, cuda_device)
    kw = dict(negatives=cfg["negatives"], batch_walks=cfg["batch_walks"], seed=cfg["seed"])
    if method == "deepwalk":
        emb = embedding.DeepWalk(g, cfg["length"], cfg["dim"], cfg["walks_per_vertex"], cfg["window"], cfg["lr"], **kw)
    else:
        emb = embedding.Node2vec(g, cfg["length"], cfg["dim"], cfg["walks_per_vertex"], cfg["window"], cfg["lr"], p=0.5, q=2.0, **kw)
    torch.manual_seed(cfg["seed"])
    model = embedding.SkipGramModel(emb.totalNodes, cfg["dim"])
    for _ in range(cfg["epochs"]):
        model = emb.learnNodeEmbedding(model)
    intra, inter = ref.cosine_split(model.W1.detach().cpu().numpy(), comm)
    print("%s: intra %.4f inter %.4f losses %s" % (method, intra, inter, ["%.1f" % x for x in emb.losses]))
    assert intra > inter
    assert emb.losses[-1] < emb.losses[0]
    assert emb.last_capped == 0


# ---- the reference's interface ----------------------------------------------------------------------------------------------------
def test_reference_interface(cuda_device):
    import networkx as nx

    import dgll.embedding
    from dgll_amd import embedding

    assert dgll.embedding is embedding
    names = ["n%02d" % i for i in range(12)]
    g = nx.Graph()
    g.add_nodes_from(reversed(names))                                   # insertion order is not the sorted order
    g.add_edges_from((names[i], names[(i + 1) % 12]) for i in range(12))
    g.add_edges_from((names[i], names[(i + 3) % 12]) for i in range(0, 12, 2))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        dw = embedding.DeepWalk(g, seed=1)
        n2v = embedding.Node2vec(g, seed=1)
    text = " | ".join(str(w.message) for w in caught)
    for piece in ("Set Walk to default: 3", "Set Embedding Dimention to default: 2", "Set Context Window to default: 3",
                  "Set Learning Rate to default: 0.25", "Set p to default: 0.5", "Set q to default: 0.8"):
        assert piece in text, piece
    assert (dw.walkLength, dw.embedDim, dw.numbOfWalksPerVertex, dw.windowSize, dw.lr) == (3, 2, 3, 3, 0.25)
    assert (n2v.p, n2v.q) == (0.5, 0.8) and dw.totalNodes == 12
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        emb = embedding.Node2vec(g, 6, 8, 2, 2, 0.01, 0.5, 2.0, seed=3)                # explicit arguments: no default is chosen
    assert not [w for w in caught if "default" in str(w.message)]
    assert emb.getAdjacencyList()[0] == [1, 3, 11]                                    # encoded by sorted label order
    walk = emb.RandomWalk("n04", 6)
    assert 1 <= len(walk) <= 6 and walk[0] == 4 and all(0 <= v < 12 for v in walk)
    assert all(g.has_edge(names[a], names[b]) for a, b in zip(walk[:-1], walk[1:]))
    model = embedding.SkipGramModel(12, 8)
    assert model.W1.shape == (12, 8) and model.W2.shape == (8, 12) and model.W1.is_cuda
    assert float(model.W1.min()) >= 0.0 and float(model.W1.max()) < 1.0
    before = model.W1.detach().clone()
    assert emb.learnNodeEmbedding(model) is model and emb.learnEdgeEmbedding(model) is model
    assert not torch.equal(before, model.W1) and len(emb.losses) == 2
    e4 = emb.getNodeEmbedding("n04")
    assert e4.shape == (8,) and torch.equal(e4, model.W1[4].data)
    assert torch.equal(emb.getEdgeEmbedding("n04", "n05"), model.W1[4].data * model.W1[5].data)
    one_hot = torch.zeros(12)
    one_hot[4] = 1
    assert torch.allclose(model(one_hot), model.W1[4] @ model.W2)
