"""Subgraph samplers on the MI355X (dgll_amd/csrc/subgraph.hip): node_subgraph, ShaDowKHopSampler and SAINTSampler bit-equal to the
numpy restatement (tests/subgraph_ref.py), stale tags, determinism, the refusals, training numerics on a batch subgraph against
float64 autograd, and the example.

Graph: 1003 nodes (no multiple of 32), degrees 0 .. 65, self-loops, node 500 with a row of 1000 entries and node 300 with a row of
2 * dgll_hip_sg_long_row() + 3 entries (capped at 1002): both rows take the workgroup kernel, every other row the lane-group one."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import neighbor_weighted_ref as wref
import subgraph_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

N = 1003
HUB, HUB2 = 500, 300


def device_graph(rowptr, col, val, n, device):
    from dgll_amd.graph import CSRGraph

    return CSRGraph(torch.as_tensor(rowptr), torch.as_tensor(col), None if val is None else torch.as_tensor(val), n, n).to(device)


@pytest.fixture(scope="module")
def main_graph(cuda_device):
    from dgll_amd import _lib

    long_row = int(_lib.lib.dgll_hip_sg_long_row())
    second = min(2 * long_row + 3, 1002)
    rowptr, col, n = wref.build_graph(N, {HUB: 1000, HUB2: second}, 5)
    assert rowptr[HUB + 1] - rowptr[HUB] == 1000 and rowptr[HUB2 + 1] - rowptr[HUB2] == second
    val = np.random.default_rng(8).random(len(col)).astype(np.float32) + np.float32(0.25)
    return {"rowptr": rowptr, "col": col, "val": val, "n": n, "long_row": long_row,
            "g": device_graph(rowptr, col, None, n, cuda_device), "gv": device_graph(rowptr, col, val, n, cuda_device)}


def assert_sub_equal(sub, eid, want, m):
    rp, cl, vl, we = want
    assert (sub.n_rows, sub.n_cols, sub.nnz) == (m, m, len(cl))
    assert sub.rowptr.dtype == torch.int64 and sub.col.dtype == torch.int32
    assert np.array_equal(sub.rowptr.cpu().numpy(), rp)
    assert np.array_equal(sub.col.cpu().numpy(), cl)
    if vl is None:
        assert sub.val is None
    else:
        assert sub.val.dtype == torch.float32 and np.array_equal(sub.val.cpu().numpy().view(np.uint32), vl.view(np.uint32))
    if eid is not None:
        assert eid.dtype == torch.int64 and np.array_equal(eid.cpu().numpy(), we)


def check_node_subgraph(graph, nodes, with_val, normalize, eids, workspace=None):
    from dgll_amd.sampling import node_subgraph

    g = graph["gv"] if with_val else graph["g"]
    out = node_subgraph(g, nodes, normalize=normalize, return_eids=eids, workspace=workspace)
    sub, eid = out if eids else (out, None)
    want = ref.node_subgraph(graph["rowptr"], graph["col"], graph["val"] if with_val else None, nodes, normalize)
    assert_sub_equal(sub, eid, want, len(nodes))
    return sub, want


def random_nodes(m, seed, must=(), never=()):
    rng = np.random.default_rng(seed)
    rest = np.setdiff1d(rng.permutation(N), np.concatenate([np.asarray(must, np.int64), np.asarray(never, np.int64)]), assume_unique=True)
    out = np.concatenate([np.asarray(must, np.int64), rest])[:m]
    return rng.permutation(out)


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 257, 1003])
def test_node_subgraph_sizes(m, main_graph):
    """Random node sets in random order; values, normalisation and eids cycle through their settings."""
    nodes = random_nodes(m, 40 + m)
    for k, (with_val, normalize, eids) in enumerate([(False, None, False), (True, None, True), (False, "row", True), (True, "row", False)]):
        check_node_subgraph(main_graph, nodes if k % 2 == 0 else nodes[::-1].copy(), with_val, normalize, eids)


@pytest.mark.parametrize("with_val", [False, True])
@pytest.mark.parametrize("normalize", [None, "row"])
def test_long_rows(with_val, normalize, main_graph):
    """Sets with and without each long row; one keeps fewer than 8 entries of the 1000-entry row, one keeps all of them."""
    rowptr, col = main_graph["rowptr"], main_graph["col"]
    hub_cols = col[rowptr[HUB]:rowptr[HUB + 1]].astype(np.int64)
    others = np.setdiff1d(np.arange(N), np.concatenate([hub_cols, [HUB]]))           # the nodes the hub's row misses
    few = np.concatenate([[HUB], np.setdiff1d(hub_cols, [HUB])[[3, 400, 900]], others])
    sub, want = check_node_subgraph(main_graph, few, with_val, normalize, True)
    assert 3 <= want[0][1] - want[0][0] < 8
    every = np.concatenate([hub_cols[::-1], [HUB] if HUB not in hub_cols else []]).astype(np.int64)
    sub, want = check_node_subgraph(main_graph, every, with_val, normalize, True)
    r = int(np.nonzero(every == HUB)[0][0])
    assert want[0][r + 1] - want[0][r] == 1000
    for must, never in (((HUB,), (HUB2,)), ((HUB2,), (HUB,)), ((HUB, HUB2), ()), ((), (HUB, HUB2))):
        nodes = random_nodes(600, 77 + len(must), must, never)
        assert all(v in nodes for v in must) and not any(v in nodes for v in never)
        check_node_subgraph(main_graph, nodes, with_val, normalize, True)


def test_identity_and_permutation(main_graph):
    sub, _ = check_node_subgraph(main_graph, np.arange(N), True, None, True)
    g = main_graph["gv"]
    assert torch.equal(sub.rowptr, g.rowptr) and torch.equal(sub.col, g.col) and torch.equal(sub.val, g.val)      # the parent exactly
    perm = np.random.default_rng(2).permutation(N)
    sub, _ = check_node_subgraph(main_graph, perm, True, None, True)
    inv = np.empty(N, np.int64)
    inv[perm] = np.arange(N)
    rowptr, col, val = main_graph["rowptr"], main_graph["col"], main_graph["val"]
    deg = np.diff(rowptr)[perm]
    assert np.array_equal(np.diff(sub.rowptr.cpu().numpy()), deg)                                                   # the parent relabelled
    starts = np.repeat(rowptr[perm], deg) + (np.arange(deg.sum()) - np.repeat(np.cumsum(deg) - deg, deg))
    assert np.array_equal(sub.col.cpu().numpy(), inv[col[starts]]) and np.array_equal(sub.val.cpu().numpy(), val[starts])


def test_parallel_entries_and_unsorted_rows(cuda_device):
    from dgll_amd import _lib

    rng = np.random.default_rng(12)
    n = 331
    deg = rng.integers(0, 40, n)
    deg[7] = 2 * int(_lib.lib.dgll_hip_sg_long_row()) + 70               # a long row of parallel entries
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    val = rng.random(len(col)).astype(np.float32)
    graph = {"rowptr": rowptr, "col": col, "val": val, "g": device_graph(rowptr, col, None, n, cuda_device),
             "gv": device_graph(rowptr, col, val, n, cuda_device)}
    for m, seed in ((n, 1), (200, 2), (65, 3)):
        nodes = np.concatenate([[7], np.setdiff1d(np.random.default_rng(seed).permutation(n), [7], assume_unique=True)])[:m]
        check_node_subgraph(graph, nodes, True, None, True)
        check_node_subgraph(graph, nodes[::-1].copy(), False, "row", False)


@pytest.mark.parametrize("normalize", [None, "row"])
def test_contiguous_ranges_equal_induced_range(normalize, main_graph):
    from dgll_amd.sampling import node_subgraph
    from dgll_amd.sampling.community import induced_range

    g = main_graph["gv"]
    for start, end in ((0, N), (0, 1), (250, 520), (HUB, HUB + 1), (990, N), (40, 40)):
        want = induced_range(g, start, end, normalize)
        got = node_subgraph(g, torch.arange(start, end, device=g.device), normalize=normalize)
        assert torch.equal(got.rowptr, want.rowptr) and torch.equal(got.col, want.col)
        assert torch.equal(got.val.view(torch.int32), want.val.view(torch.int32))


def test_stale_tags_do_not_leak_and_runs_repeat(main_graph):
    from dgll_amd.sampling import SubgraphWorkspace, node_subgraph

    g = main_graph["gv"]
    ws = SubgraphWorkspace(N, g.device)
    a = random_nodes(700, 1, (HUB,))
    b = random_nodes(257, 2, (HUB2,), (HUB,))
    check_node_subgraph(main_graph, a, True, None, True, workspace=ws)
    sub_b, _ = check_node_subgraph(main_graph, b, True, None, True, workspace=ws)          # every tag of `a` is stale now
    fresh = node_subgraph(g, b, workspace=SubgraphWorkspace(N, g.device))
    assert torch.equal(sub_b.rowptr, fresh.rowptr) and torch.equal(sub_b.col, fresh.col) and torch.equal(sub_b.val, fresh.val)
    assert ws.epoch == 2
    again, eid2 = node_subgraph(g, b, return_eids=True, workspace=ws)                     # the same call twice: identical bits
    first, eid1 = node_subgraph(g, b, return_eids=True, workspace=ws)
    assert torch.equal(again.rowptr, first.rowptr) and torch.equal(again.col, first.col) and torch.equal(again.val, first.val)
    assert torch.equal(eid1, eid2)


def test_node_subgraph_refusals(main_graph, cuda_device):
    from dgll_amd.sampling import SubgraphWorkspace, node_subgraph

    g, n = main_graph["g"], N
    ws = SubgraphWorkspace(n, g.device)
    with pytest.raises(ValueError, match="duplicate"):
        node_subgraph(g, [3, 9, 3], workspace=ws)
    for bad in ([3, n], [-1, 4]):
        with pytest.raises(ValueError, match="outside"):
            node_subgraph(g, bad, workspace=ws)
    bad_col = main_graph["col"].copy()
    bad_col[main_graph["rowptr"][9]] = n                                                    # a column id == N
    with pytest.raises(ValueError, match="column"):
        node_subgraph(device_graph(main_graph["rowptr"], bad_col, None, n, cuda_device), [9, 4])
    bad_col[main_graph["rowptr"][HUB] + 700] = n                                            # and inside a long row
    with pytest.raises(ValueError, match="column"):
        node_subgraph(device_graph(main_graph["rowptr"], bad_col, None, n, cuda_device), [HUB, 4])
    with pytest.raises(ValueError, match="workspace"):
        node_subgraph(g, [1], workspace=SubgraphWorkspace(n + 1, g.device))
    check_node_subgraph(main_graph, np.array([n - 1, 3, 9]), False, "row", True, workspace=ws)      # and it still works afterwards


# ---- ShaDow -----------------------------------------------------------------------------------------------------------------------
def pick_seeds(count, seed):
    must = [N - 1] if count == 1 else [N - 1, HUB, 0, 7, 16, HUB2]
    return random_nodes(count, seed, must)


@pytest.mark.parametrize("count", [1, 64, 65, 257])
@pytest.mark.parametrize("fanouts", [[5, 2], [-1, 3]], ids=str)
def test_shadow_bit_equal(fanouts, count, main_graph):
    from dgll_amd.sampling import ShaDowKHopSampler

    seeds = pick_seeds(count, 300 + count)
    s = ShaDowKHopSampler(fanouts, main_graph["g"])
    inp, out, sub = s.sample_seeded(None, seeds, 0xABCDEF + count)
    want_inp, want = ref.shadow(main_graph["rowptr"], main_graph["col"], seeds, fanouts, 0xABCDEF + count)
    assert out is seeds and inp.dtype == torch.int64 and np.array_equal(inp.cpu().numpy(), want_inp)
    assert sub.n_rows == len(want_inp) and np.array_equal(inp[:count].cpu().numpy(), seeds)     # the seeds are the leading rows
    assert_sub_equal(sub, None, want, len(want_inp))
    inp2, _, sub2 = s.sample_seeded(None, seeds, 0xABCDEF + count)                              # determinism
    assert torch.equal(inp, inp2) and torch.equal(sub.rowptr, sub2.rowptr) and torch.equal(sub.col, sub2.col) and torch.equal(sub.val, sub2.val)


@pytest.mark.parametrize("normalize", ["row", None])
def test_shadow_weighted(normalize, main_graph):
    from dgll_amd.sampling import ShaDowKHopSampler

    rowptr, col = main_graph["rowptr"], main_graph["col"]
    w = wref.build_weights(rowptr, 21)
    seeds = pick_seeds(65, 17)
    s = ShaDowKHopSampler([5, 2], main_graph["g"], prob=torch.as_tensor(w), normalize=normalize)
    inp, _, sub = s.sample_seeded(None, seeds, 555)
    want_inp, want = ref.shadow(rowptr, col, seeds, [5, 2], 555, normalize=normalize, weights=w)
    assert np.array_equal(inp.cpu().numpy(), want_inp)
    assert_sub_equal(sub, None, want, len(want_inp))
    assert s.graph.nnz == int((w > 0).sum()) < len(col)                   # induced on the filtered graph


def test_shadow_sample_draws_numpy_seeds(main_graph):
    from dgll_amd.sampling import ShaDowKHopSampler

    s = ShaDowKHopSampler([5, 2], main_graph["g"])
    seeds = pick_seeds(64, 3)
    np.random.seed(4)
    a = [s.sample(None, seeds) for _ in range(2)]
    np.random.seed(4)
    b = [s.sample(None, seeds) for _ in range(2)]
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[2].col, y[2].col) for x, y in zip(a, b)) and not torch.equal(a[0][0], a[1][0])
    inp, _, sub = s.sample_seeded(None, np.zeros(0, np.int64), 1)         # no seeds: an empty subgraph
    assert inp.numel() == 0 and (sub.n_rows, sub.n_cols, sub.nnz) == (0, 0, 0) and sub.rowptr.tolist() == [0]


# ---- GraphSAINT -------------------------------------------------------------------------------------------------------------------
SAINT_CASES = [("node", 1), ("node", 64), ("node", 4096), ("edge", 1), ("edge", 64), ("edge", 4096),
               ("walk", (1, 1)), ("walk", (64, 4)), ("walk", (300, 8))]


@pytest.mark.parametrize("mode,budget", SAINT_CASES, ids=str)
def test_saint_bit_equal(mode, budget, main_graph):
    from dgll_amd.sampling import SAINTSampler

    rowptr, col, val = main_graph["rowptr"], main_graph["col"], main_graph["val"]
    seed = 0x5A1A7 + (budget if mode != "walk" else budget[0])
    s = SAINTSampler(mode, budget, main_graph["gv"])
    nodes, sub = s.sample_seeded(None, seed)
    want_nodes, want = ref.saint(rowptr, col, val, mode, budget, seed, "row")
    got = nodes.cpu().numpy()
    assert nodes.dtype == torch.int64 and np.array_equal(got, want_nodes)
    assert np.all(np.diff(got) > 0)                                       # ascending and unique
    if mode == "node":
        assert np.all(np.diff(rowptr)[got] > 0)                           # never a node of degree 0
    assert_sub_equal(sub, None, want, len(want_nodes))
    nodes2, sub2 = s.sample_seeded(None, seed)                            # determinism, on the same workspace
    assert torch.equal(nodes, nodes2) and torch.equal(sub.rowptr, sub2.rowptr) and torch.equal(sub.col, sub2.col) and torch.equal(sub.val, sub2.val)
    n3, sub3 = SAINTSampler(mode, budget, main_graph["gv"], normalize=None).sample_seeded(None, seed)
    assert torch.equal(n3, nodes)
    assert_sub_equal(sub3, None, ref.node_subgraph(rowptr, col, val, want_nodes, None), len(want_nodes))


def test_saint_walk_with_dead_ends(cuda_device):
    """Half of the nodes have no entries: most walks end early and the rest of their row is -1."""
    from dgll_amd.sampling import SAINTSampler

    rng = np.random.default_rng(4)
    n = 515
    deg = np.where(np.arange(n) % 2 == 0, 0, rng.integers(1, 6, n))
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(n, d, replace=False)) for d in deg]).astype(np.int32)
    g = device_graph(rowptr, col, None, n, cuda_device)
    walks = ref.saint_draws(rowptr, col, "walk", (200, 6), 31)
    assert (walks == -1).any() and (walks[:, 1:] >= 0).any()
    nodes, sub = SAINTSampler("walk", (200, 6), g).sample_seeded(None, 31)
    want_nodes, want = ref.saint(rowptr, col, None, "walk", (200, 6), 31)
    assert np.array_equal(nodes.cpu().numpy(), want_nodes)
    assert_sub_equal(sub, None, want, len(want_nodes))


def test_saint_sample_ignores_indices(main_graph):
    from dgll_amd.sampling import SAINTSampler

    s = SAINTSampler("edge", 64)
    np.random.seed(9)
    a = s.sample(main_graph["g"], indices=torch.arange(5))
    np.random.seed(9)
    b = s.sample(None, indices=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].col, b[1].col) and a[1].n_rows == a[0].numel()
    bad = main_graph["col"].copy()
    bad[:] = N                                                            # every column out of range: the edge draw reports it
    with pytest.raises(ValueError, match="column"):
        SAINTSampler("edge", 64, device_graph(main_graph["rowptr"], bad, None, N, main_graph["g"].device)).sample_seeded(None, 1)


# ---- training numerics --------------------------------------------------------------------------------------------------------------
def load_example():
    spec = importlib.util.spec_from_file_location("subgraph_example_train", os.path.join(ROOT, "examples", "subgraph", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def dense64(want, m):
    rp, cl, vl, _ = want
    a = torch.zeros(m, m, dtype=torch.float64)
    rows = torch.as_tensor(np.repeat(np.arange(m), np.diff(rp)))
    a.index_put_((rows, torch.as_tensor(cl.astype(np.int64))), torch.as_tensor(vl.astype(np.float64)), accumulate=True)
    return a


@pytest.mark.parametrize("kind", ["shadow", "saint"])
def test_one_batch_matches_float64_autograd(kind, main_graph, cuda_device):
    """The example's SAGE-mean model (2 layers on the ShaDow batch, 3 on the GraphSAINT batch) on one batch subgraph against float64
    CPU autograd on the RESTATED subgraph: loss and parameter gradients within the relative 1e-4 of
    test_neighbor_gpu.py::test_one_batch_matches_float64_autograd and test_edge_pred_gpu.py (the same layers, fp32)."""
    from dgll_amd import ops
    from dgll_amd.sampling import SAINTSampler, ShaDowKHopSampler, layerwise

    rowptr, col = main_graph["rowptr"], main_graph["col"]
    torch.manual_seed(0)
    if kind == "shadow":
        seeds = pick_seeds(257, 5)
        nodes, _, sub = ShaDowKHopSampler([5, 2], main_graph["g"]).sample_seeded(None, seeds, 21)
        want_nodes, want = ref.shadow(rowptr, col, seeds, [5, 2], 21)
        rows, layers = torch.arange(len(seeds)), 2
    else:
        nodes, sub = SAINTSampler("node", 600, main_graph["g"]).sample_seeded(None, 21)
        want_nodes, want = ref.saint(rowptr, col, None, "node", 600, 21)
        rows, layers = torch.nonzero(torch.as_tensor(want_nodes % 2 == 0)).flatten(), 3
    assert np.array_equal(nodes.cpu().numpy(), want_nodes)
    layerwise.record_stream([sub], nodes, torch.cuda.current_stream(cuda_device))
    m = len(want_nodes)
    x = torch.randn(m, 50)
    labels = torch.randint(0, 7, (m,))
    model = load_example().SageMean(50, 64, 7, layers=layers).to(cuda_device)
    logits = model(sub, x.to(cuda_device))
    loss = ops.cross_entropy(logits[rows.to(cuda_device)], labels[rows].to(cuda_device))
    loss.backward()
    a = dense64(want, m)
    P = {k: v.detach().cpu().double().requires_grad_() for k, v in model.named_parameters()}
    h = x.double()
    for i in range(layers):
        h = h @ P["w_self.%d.weight" % i].T + P["w_self.%d.bias" % i] + (a @ h) @ P["w_neigh.%d.weight" % i].T
        if i + 1 < layers:
            h = torch.relu(h)
    want_loss = torch.nn.functional.cross_entropy(h[rows], labels[rows])
    want_loss.backward()
    ratios = {"loss": abs(loss.item() - want_loss.item()) / abs(want_loss.item()), "logits": rel(logits.detach().cpu(), h.detach())}
    for k, prm in model.named_parameters():
        ratios[k] = rel(prm.grad.cpu(), P[k].grad)
    print(kind, " ".join("%s %.3g" % kv for kv in ratios.items()))
    for k, r in ratios.items():
        assert r < 1e-4, (k, r)


@pytest.mark.parametrize("sampler", ["shadow", "saint-node", "saint-edge", "saint-walk"])
def test_example_runs(sampler):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "subgraph", "train.py"), "--sampler", sampler, "--nodes", "4000",
                          "--avg-degree", "20", "--batch", "256", "--budget", "500", "--roots", "200", "--length", "3", "--batches", "5",
                          "--epochs", "2"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    losses = [float(line.split("loss")[1].split()[0]) for line in res.stdout.splitlines() if line.startswith("epoch")]
    assert len(losses) == 2 and all(np.isfinite(losses)), res.stdout


# ---- the other kernel paths -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense_graph(cuda_device):
    """A parent that averages more than 64 entries a row, so both passes take the wavefront-per-row instantiation of the lane-group
    kernel: 300 nodes of 70 .. 130 entries (random columns: unsorted rows, parallel entries, self-loops), rows of 0, 1, 63, 64, 65
    and exactly dgll_hip_sg_long_row() entries, and node 150 with 2 * dgll_hip_sg_long_row() + 3 (the workgroup kernel)."""
    from dgll_amd import _lib

    long_row = int(_lib.lib.dgll_hip_sg_long_row())
    rng = np.random.default_rng(33)
    n = 300
    deg = rng.integers(70, 131, n)
    deg[[5, 6, 7, 8, 9, 10]] = [0, 1, 63, 64, 65, long_row]
    deg[150] = 2 * long_row + 3
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    assert rowptr[-1] > 64 * n
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    val = rng.random(len(col)).astype(np.float32) + np.float32(0.5)
    return {"rowptr": rowptr, "col": col, "val": val, "n": n, "g": device_graph(rowptr, col, None, n, cuda_device),
            "gv": device_graph(rowptr, col, val, n, cuda_device)}


@pytest.mark.parametrize("m", [0, 1, 2, 63, 64, 65, 129, 300])
def test_dense_parent_wavefront_per_row(m, dense_graph):
    """Bit equality on the dense parent for every setting: values x normalize x eids, node sets in random order that hold the special
    rows first (M = 1: the row of 65 entries alone; M = 2 adds the row of exactly the threshold)."""
    n = dense_graph["n"]
    must = [9, 10, 150, 5, 6, 7, 8]
    rest = np.setdiff1d(np.random.default_rng(m).permutation(n), must, assume_unique=True)
    nodes = np.concatenate([np.asarray(must, np.int64), rest])[:m]
    if m > 2:
        nodes = np.random.default_rng(m + 1).permutation(nodes)
    for with_val in (False, True):
        for normalize in (None, "row"):
            for eids in (False, True):
                check_node_subgraph(dense_graph, nodes, with_val, normalize, eids)


def test_dense_parent_identity_and_samplers(dense_graph):
    from dgll_amd.sampling import SAINTSampler, ShaDowKHopSampler

    g, n = dense_graph["gv"], dense_graph["n"]
    sub, _ = check_node_subgraph(dense_graph, np.arange(n), True, None, True)
    assert torch.equal(sub.rowptr, g.rowptr) and torch.equal(sub.col, g.col) and torch.equal(sub.val, g.val)
    rowptr, col, val = dense_graph["rowptr"], dense_graph["col"], dense_graph["val"]
    nodes, sub = SAINTSampler("edge", 64, g).sample_seeded(None, 77)
    want_nodes, want = ref.saint(rowptr, col, val, "edge", 64, 77, "row")
    assert np.array_equal(nodes.cpu().numpy(), want_nodes)
    assert_sub_equal(sub, None, want, len(want_nodes))
    seeds = np.array([150, 9, 5, 299, 0])
    inp, _, sub = ShaDowKHopSampler([3, 2], dense_graph["g"]).sample_seeded(None, seeds, 78)
    want_inp, want = ref.shadow(rowptr, col, seeds, [3, 2], 78)
    assert np.array_equal(inp.cpu().numpy(), want_inp)
    assert_sub_equal(sub, None, want, len(want_inp))


def test_grid_stride_of_both_row_kernels(cuda_device):
    """M = N = 40 003 listed rows of a sparse parent: the lane-group kernel (16 lanes a row, at most 2048 workgroups of 16 rows) and
    the workgroup kernel (at most 2048 windows of 16 rows) both go round their grid-stride loops, which start at row 32 768.  Rows
    above the threshold sit in the first pass of the grid and in the second, at both ends of a window and next to each other."""
    from dgll_amd import _lib

    long_row = int(_lib.lib.dgll_hip_sg_long_row())
    rng = np.random.default_rng(51)
    n = 40003
    deg = rng.integers(0, 7, n)
    perm = rng.permutation(n)
    long_at = [100, 32767, 32768, 32783, 32784, 36000, 36001, n - 1]         # positions in the node list
    deg[perm[long_at]] = long_row + 1 + np.arange(len(long_at)) * 37
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    val = rng.random(len(col)).astype(np.float32)
    graph = {"rowptr": rowptr, "col": col, "val": val, "g": device_graph(rowptr, col, None, n, cuda_device),
             "gv": device_graph(rowptr, col, val, n, cuda_device)}
    sub, want = check_node_subgraph(graph, perm, True, None, True)
    assert sub.nnz == len(col)                                               # every node listed: every entry kept
    check_node_subgraph(graph, perm, False, "row", False)
    keep = np.sort(rng.choice(n, 36500, replace=False))                      # a proper subset that still strides: entries are dropped
    sub, want = check_node_subgraph(graph, perm[keep], True, "row", True)
    assert 0 < sub.nnz < len(col)
