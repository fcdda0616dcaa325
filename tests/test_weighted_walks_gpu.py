"""Edge-weighted walks on the device: the alias tables (valid, within 2^-30 of w / sum w, reproducible), walks bit-equal to the numpy
restatement fed the device-built table, independent of the batching, distributed as the reference's weighted node2vec
probabilities, the refusals, and DeepWalk / Node2vec with weighted=True end to end.  No test reads the reference tree."""
import numpy as np
import pytest
import torch

import embedding_ref as ref
import weighted_walk_ref as wref
from conftest import load_golden
from test_embedding_host import golden_starts, transition_check
from test_weighted_walks_host import hub_first_step_excess, row_shares

pytestmark = pytest.mark.gpu

PQ = [(1.0, 1.0), (0.5, 2.0), (4.0, 0.25)]


def _csr(rowptr, col, val, dev):
    import dgll_amd

    n = len(rowptr) - 1
    return dgll_amd.CSRGraph(torch.from_numpy(np.asarray(rowptr, np.int64)), torch.from_numpy(np.asarray(col, np.int32)),
                             None if val is None else torch.from_numpy(np.asarray(val, np.float32)), n, n).to(dev)


@pytest.fixture(scope="module")
def golden():
    return load_golden("node2vec_probs_weighted")


@pytest.fixture(scope="module")
def golden_graph(golden, cuda_device):
    return _csr(golden["rowptr"], golden["col"], golden["val"], cuda_device)


@pytest.fixture(scope="module")
def golden_table(golden_graph):
    from dgll_amd import embedding

    return embedding.AliasTable.from_graph(golden_graph).numpy()


# ---- the table --------------------------------------------------------------------------------------------------------------------
def test_table_on_the_shapes_graph(cuda_device):
    from dgll_amd import embedding

    rowptr, col, val, kinds = wref.shapes_graph()
    deg = np.diff(rowptr)
    assert sorted(set(deg.tolist())) == sorted(set(wref.SHAPE_DEGREES + (wref.SHAPE_LONG,)))
    g = _csr(rowptr, col, val, cuda_device)
    table = embedding.AliasTable.from_graph(g)
    assert embedding.AliasTable.from_graph(g) is table                      # cached on the graph
    T, alias = table.numpy()
    assert (alias < np.repeat(deg, deg)).all()
    got, want = wref.implied_probs(rowptr, T, alias), row_shares(rowptr, val)
    assert not got[val == 0].any()                                          # no zero-weight edge has implied mass
    err = np.abs(got - want).max()
    print("worst |implied - w / sum w| = %.3g (bound 2^-30 = %.3g)" % (err, 2.0 ** -30))
    assert err <= 2.0 ** -30
    again = embedding.AliasTable.from_graph(_csr(rowptr, col, val, cuda_device))
    assert again is not table and torch.equal(again.table, table.table)     # a second build: the same bits
    # walks: a row of zeros is a dead end, a zero-weight edge is never taken, and the device equals the restatement here too
    starts = np.repeat(np.nonzero(deg)[0], 64)
    info = torch.zeros(2, dtype=torch.int64, device=cuda_device)
    wk = embedding.random_walks(g, torch.from_numpy(starts).to(cuda_device), 4, seed=9, info=info, weighted=True).cpu().numpy()
    assert embedding.walk_info(info) == 0
    assert np.array_equal(wk, wref.walks(rowptr, col, T, alias, starts, 4, seed=9))
    dead = np.array([k == "all_zero" for k in kinds])
    assert (wk[dead[starts], 1:] == -1).all() and (wk[~dead[starts], 1] >= 0).all()
    zero_edges = set(zip(np.repeat(np.arange(len(deg)), deg)[val == 0].tolist(), col[val == 0].tolist()))
    taken = set(zip(wk[:, :-1].ravel().tolist(), wk[:, 1:].ravel().tolist()))
    assert not (taken & zero_edges)


def test_unit_weights_give_exactly_uniform_tables(golden, cuda_device):
    from dgll_amd import embedding

    rowptr, col = golden["rowptr"], golden["col"]
    g = _csr(rowptr, col, np.ones(len(col), np.float32), cuda_device)
    T, alias = embedding.AliasTable.from_graph(g).numpy()
    deg = np.diff(rowptr)
    assert np.array_equal(wref.implied_probs(rowptr, T, alias), 1.0 / np.repeat(deg, deg))


# ---- walks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q", PQ)
def test_weighted_walks_equal_the_restatement(golden, golden_graph, golden_table, cuda_device, p, q):
    from dgll_amd import embedding

    rowptr, col = golden["rowptr"], golden["col"]
    n_nodes = len(rowptr) - 1
    starts = np.tile(np.arange(n_nodes, dtype=np.int64), 3)
    info = torch.zeros(2, dtype=torch.int64, device=cuda_device)
    got = embedding.random_walks(golden_graph, torch.from_numpy(starts).to(cuda_device), 12, p=p, q=q, seed=1234, info=info,
                                 weighted=True).cpu().numpy()
    want, capped = wref.walks(rowptr, col, *golden_table, starts, 12, p, q, seed=1234, return_capped=True)
    assert got.dtype == np.int32 and got.shape == (len(starts), 12)
    assert np.array_equal(got, want)
    assert embedding.walk_info(info) == capped
    positive = set(zip(np.repeat(np.arange(n_nodes), np.diff(rowptr))[golden["val"] > 0].tolist(), col[golden["val"] > 0].tolist()))
    steps = set(zip(got[:, :-1].ravel().tolist(), got[:, 1:].ravel().tolist()))
    assert {(a, b) for a, b in steps if b >= 0} <= positive                 # only edges of positive weight are walked
    assert (got[:, 1:] >= 0).mean() > 0.3
    unweighted = embedding.random_walks(golden_graph, torch.from_numpy(starts).to(cuda_device), 12, p=p, q=q, seed=1234).cpu().numpy()
    assert np.array_equal(unweighted, ref.walks(rowptr, col, starts, 12, p, q, seed=1234))      # values do not touch the default path


@pytest.mark.parametrize("p,q", PQ[:2])
def test_weighted_walks_do_not_depend_on_the_batching(golden_graph, cuda_device, p, q):
    from dgll_amd import embedding

    n = 2 * golden_graph.n_rows
    starts = (torch.arange(n, device=cuda_device) * 7) % golden_graph.n_rows
    alias = embedding.AliasTable.from_graph(golden_graph)
    whole = embedding.random_walks(golden_graph, starts, 9, p=p, q=q, seed=5, weighted=True)
    lo = embedding.random_walks(golden_graph, starts[:n // 2], 9, p=p, q=q, seed=5, first_walk_index=0, alias=alias)
    hi = embedding.random_walks(golden_graph, starts[n // 2:], 9, p=p, q=q, seed=5, first_walk_index=n // 2, alias=alias)
    assert torch.equal(whole, torch.cat([lo, hi]))
    assert not torch.equal(whole, embedding.random_walks(golden_graph, starts, 9, p=p, q=q, seed=6, weighted=True))
    assert not torch.equal(whole, embedding.random_walks(golden_graph, starts, 9, p=p, q=q, seed=5))


@pytest.mark.parametrize("case", [0, 1])
def test_device_weighted_walks_follow_the_reference_probabilities(golden, golden_graph, cuda_device, case):
    from dgll_amd import embedding

    p, q = golden.meta["pq"][case]
    starts = torch.from_numpy(golden_starts(golden)).to(cuda_device)
    info = torch.zeros(2, dtype=torch.int64, device=cuda_device)
    wk = embedding.random_walks(golden_graph, starts, 3, p=p, q=q, seed=golden.meta["seed"], info=info, weighted=True).cpu().numpy()
    assert embedding.walk_info(info) == 0
    checked, mass, excess = transition_check(golden, wk, case)
    print("p=%g q=%g: %d of %d cells checked, worst excess over the cap %.3g" % (p, q, checked, mass, excess))
    assert excess <= 0.0


def test_device_first_step_follows_the_weights(golden, golden_graph, cuda_device):
    from dgll_amd import embedding

    starts = torch.from_numpy(golden_starts(golden)).to(cuda_device)
    wk = embedding.random_walks(golden_graph, starts, 2, seed=golden.meta["seed"], weighted=True).cpu().numpy()
    excess = hub_first_step_excess(golden, wk)
    print("first step from the hub: worst excess over the cap %.3g" % excess)
    assert excess <= 0.0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_weighted_walks_refuse_what_they_cannot_draw(cuda_device):
    from dgll_amd import embedding

    starts = torch.zeros(4, dtype=torch.int64, device=cuda_device)
    with pytest.raises(ValueError):
        embedding.random_walks(_csr([0, 2, 3, 4], [1, 2, 0, 0], None, cuda_device), starts, 3, weighted=True)       # no values
    for bad in (float("nan"), -1.0, float("inf")):
        with pytest.raises(ValueError, match="weight"):
            embedding.random_walks(_csr([0, 2, 3, 4], [1, 2, 0, 0], [1.0, bad, 1.0, 1.0], cuda_device), starts, 3, weighted=True)
    g = _csr([0, 2, 3, 4], [2, 1, 0, 0], [1.0, 2.0, 1.0, 1.0], cuda_device)                                          # row 0 descends
    assert embedding.random_walks(g, starts, 3, weighted=True).shape == (4, 3)
    with pytest.raises(ValueError):
        embedding.random_walks(g, starts, 3, p=0.5, q=2.0, weighted=True)
    other = embedding.AliasTable.from_graph(_csr([0, 1, 2], [1, 0], [1.0, 1.0], cuda_device))
    with pytest.raises(ValueError):
        embedding.random_walks(g, starts, 3, alias=other)                                                             # another graph's


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["deepwalk", "node2vec"])
def test_weighted_models_never_cross_a_zero_weight_cut(cuda_device, method):
    import networkx as nx

    from dgll_amd import embedding

    rowptr, col, comm = ref.planted_partition()
    n = len(comm)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    assert (comm[row] != comm[col]).any()                                   # the cut exists; its edges get weight 0
    graph = nx.Graph()
    graph.add_nodes_from(range(n))
    for a, b in zip(row.tolist(), col.tolist()):
        if comm[a] != comm[b]:
            graph.add_edge(a, b, weight=0.0)
        elif (a + b) % 3:
            graph.add_edge(a, b, weight=1.0 + (a + b) % 4)
        else:
            graph.add_edge(a, b)                                            # no attribute: weight 1
    cfg = ref.TRAIN
    kw = dict(negatives=cfg["negatives"], batch_walks=cfg["batch_walks"], seed=cfg["seed"], device=cuda_device, weighted=True)
    if method == "deepwalk":
        emb = embedding.DeepWalk(graph, cfg["length"], cfg["dim"], cfg["walks_per_vertex"], cfg["window"], cfg["lr"], **kw)
    else:
        emb = embedding.Node2vec(graph, cfg["length"], cfg["dim"], cfg["walks_per_vertex"], cfg["window"], cfg["lr"], 0.5, 2.0, **kw)
    assert emb.csr.val is not None and emb.alias is not None
    want = np.where(comm[row] != comm[col], 0.0, np.where((row + col) % 3 != 0, 1.0 + (row + col) % 4, 1.0))
    assert np.array_equal(emb.csr.val.cpu().numpy(), want.astype(np.float32))
    starts = torch.arange(n, device=cuda_device).repeat(8)
    walks, _ = emb._walk_batch(starts, 30)
    wk = walks.cpu().numpy()
    side = np.where(wk >= 0, comm[np.maximum(wk, 0)], -1)
    assert ((side == side[:, :1]) | (side < 0)).all()                       # exact: no walk leaves its start's community
    assert (wk[:, 1] >= 0).all()
    torch.manual_seed(cfg["seed"])
    model = embedding.SkipGramModel(n, cfg["dim"], device=cuda_device)
    for _ in range(cfg["epochs"]):
        model = emb.learnNodeEmbedding(model)
    assert emb.last_capped == 0 and emb.losses[-1] < emb.losses[0]
    intra, inter = ref.cosine_split(model.W1.data.cpu().numpy(), comm)
    print("%s weighted: intra %.4f inter %.4f" % (method, intra, inter))
    assert intra > inter
