"""Device neighbour sampler (dgll_amd/csrc/neighbor.hip) on the MI355X: bit-equality with the numpy restatement, the block contract,
batch independence of a node's draw, determinism, edge cases, training numerics on the blocks, the mini-batch pipeline and the
example.

Graphs.  The main graph has 1003 nodes (no multiple of 32 or 64: bitmap and marker tails), degrees 0, 1, f - 1, f, f + 1 for every
fan-out used, 63, 64, 65, self-loops, node N - 1 among seeds and neighbours, and sources that are destinations.  A graph of 1003
nodes with unique columns cannot hold a row of 5000 in-neighbours, so its hub has 1000 and the hub of 5000 in-neighbours lives in a
second graph of 6007 nodes (again no multiple of 32): it is copied whole under f = -1 and sampled under f = 25 / 10 there."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import neighbor_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

FANOUTS = [[1], [5, 2], [25, 10, 10], [-1, 3], [64]]
SEED_COUNTS = [1, 63, 64, 65, 257, 600]
DEGREES = [0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 24, 25, 26, 63, 64, 65]


def build_graph(n, hub, hub_degree, seed):
    """In-neighbour CSR (sorted, unique columns): node v has degree DEGREES[v % 16], `hub` has hub_degree."""
    rng = np.random.default_rng(seed)
    rows = []
    for v in range(n):
        d = hub_degree if v == hub else DEGREES[v % len(DEGREES)]
        forced = []
        if d >= 1 and v % 7 == 0:
            forced.append(v)                      # self-loop
        if d >= 3 and v != n - 1:
            forced.append(n - 1)                  # the last node as a neighbour
        pool = np.setdiff1d(np.arange(n), forced)
        rows.append(np.sort(np.concatenate([np.asarray(forced, np.int64), rng.choice(pool, d - len(forced), replace=False)])))
        assert len(rows[-1]) == d
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rowptr, np.concatenate(rows).astype(np.int32), n


def device_graph(rowptr, col, n, device):
    from dgll_amd.graph import CSRGraph

    return CSRGraph(torch.as_tensor(rowptr), torch.as_tensor(col), None, n, n).to(device)


@pytest.fixture(scope="module")
def main_graph(cuda_device):
    rowptr, col, n = build_graph(1003, hub=500, hub_degree=1000, seed=5)
    return rowptr, col, n, device_graph(rowptr, col, n, cuda_device)


@pytest.fixture(scope="module")
def hub_graph(cuda_device):
    rowptr, col, n = build_graph(6007, hub=4000, hub_degree=5000, seed=6)
    return rowptr, col, n, device_graph(rowptr, col, n, cuda_device)


def pick_seeds(n, count, must, seed):
    rest = np.setdiff1d(np.random.default_rng(seed).permutation(n), must, assume_unique=True)
    out = np.concatenate([np.asarray(must, np.int64), rest])[:count]
    return np.random.default_rng(seed + 1).permutation(out)


def as_dicts(input_nodes, blocks):
    """Device blocks as the restatement's dicts; a block's sources are the destinations of the block outside it."""
    out, src = [], input_nodes.cpu().numpy()
    for b in blocks:
        out.append({"rowptr": b.rowptr.cpu().numpy(), "col": b.col.cpu().numpy(), "val": None if b.val is None else b.val.cpu().numpy(),
                    "n_rows": b.n_rows, "n_cols": b.n_cols, "src": src, "dst": src[:b.n_rows]})
        src = src[:b.n_rows]
    return out


def assert_bit_equal(got_inp, got_blocks, want_inp, want_blocks):
    assert got_inp.dtype == torch.int64 and np.array_equal(got_inp.cpu().numpy(), want_inp)
    assert len(got_blocks) == len(want_blocks)
    for g, w in zip(got_blocks, want_blocks):
        assert g.rowptr.dtype == torch.int64 and g.col.dtype == torch.int32
        assert (g.n_rows, g.n_cols) == (w["n_rows"], w["n_cols"])
        assert np.array_equal(g.rowptr.cpu().numpy(), w["rowptr"])
        assert np.array_equal(g.col.cpu().numpy(), w["col"])
        if w["val"] is None:
            assert g.val is None
        else:
            assert g.val.dtype == torch.float32 and np.array_equal(g.val.cpu().numpy().view(np.uint32), w["val"].view(np.uint32))


def run_case(graph, fanouts, seeds, seed, norm="mean"):
    from dgll_amd.sampling import NeighborSampler

    rowptr, col, n, g = graph
    s = NeighborSampler(fanouts, g, norm=norm)
    inp, out, blocks = s.sample_seeded(None, seeds, seed)
    want_inp, want = ref.sample_blocks(rowptr, col, seeds, fanouts, seed, norm)
    assert out is seeds and blocks[-1].n_rows == len(seeds)
    assert_bit_equal(inp, blocks, want_inp, want)
    ref.check_invariants(rowptr, col, seeds, fanouts, want_inp, want, norm)
    ref.check_invariants(rowptr, col, seeds, fanouts, inp.cpu().numpy(), as_dicts(inp, blocks), norm)
    return inp, blocks


@pytest.mark.parametrize("count", SEED_COUNTS)
@pytest.mark.parametrize("fanouts", FANOUTS, ids=str)
def test_bit_equal_to_the_restatement(fanouts, count, main_graph):
    n = main_graph[2]
    must = [n - 1] if count == 1 else [n - 1, 500, 0, 7, 16, 498]      # the last node, the hub, self-loops, an isolated node, a hub source
    seeds = pick_seeds(n, count, must, 100 + count)
    run_case(main_graph, fanouts, seeds, 0x1234567890ABCDEF + count)


@pytest.mark.parametrize("count", [65, 257])
@pytest.mark.parametrize("fanouts", [[-1, 3], [25, 10, 10]], ids=str)
def test_hub_of_5000_in_neighbours(fanouts, count, hub_graph):
    """The hub is a seed, so it is a destination of every layer: copied whole under -1 (5000 entries, flat passes), sampled under
    25 and 10."""
    rowptr, col, n, _ = hub_graph
    assert rowptr[4001] - rowptr[4000] == 5000
    seeds = pick_seeds(n, count, [4000, n - 1], 7)
    inp, blocks = run_case(hub_graph, fanouts, seeds, 99)
    outer = blocks[0]
    hub_row = int(np.nonzero(inp[:outer.n_rows].cpu().numpy() == 4000)[0][0])
    assert int(outer.rowptr[hub_row + 1] - outer.rowptr[hub_row]) == (5000 if fanouts[0] < 0 else fanouts[0])


def test_no_values_without_norm(main_graph):
    seeds = pick_seeds(main_graph[2], 65, [1002, 500], 3)
    run_case(main_graph, [5, 2], seeds, 4, norm=None)


def test_a_draw_does_not_depend_on_the_batch(main_graph):
    from dgll_amd.sampling import NeighborSampler

    rowptr, col, n, g = main_graph
    s = NeighborSampler([10], g)
    big = pick_seeds(n, 600, [n - 1, 500, 26, 65], 11)
    inp_b, _, blk_b = s.sample_seeded(None, big, 31)
    src_b, b = inp_b.cpu().numpy(), blk_b[0]
    for v in (500, 26, 65, n - 1, int(big[599])):
        inp_1, _, blk_1 = s.sample_seeded(None, [v], 31)
        alone = set(inp_1.cpu().numpy()[blk_1[0].col.cpu().numpy()].tolist())
        r = int(np.nonzero(big == v)[0][0])
        inside = set(src_b[b.col[int(b.rowptr[r]):int(b.rowptr[r + 1])].cpu().numpy()].tolist())
        assert alone == inside == set(ref.draw(rowptr, col, v, 10, 31, 0))


def same(a, b):
    return torch.equal(a[0], b[0]) and all(torch.equal(x.rowptr, y.rowptr) and torch.equal(x.col, y.col) and torch.equal(x.val, y.val)
                                           for x, y in zip(a[2], b[2]))


def test_same_seed_same_bits_other_seed_other_sample(cuda_device):
    from dgll_amd.sampling import NeighborSampler

    nbrs = np.arange(5000, 5012)
    n = 5012
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:4097] = 12
    rowptr = np.cumsum(rowptr)
    g = device_graph(rowptr, np.tile(nbrs, 4096).astype(np.int32), n, cuda_device)
    seeds = np.arange(4096)
    s1, s2 = NeighborSampler([5], g), NeighborSampler([5], g)
    a = s1.sample_seeded(None, seeds, 77)
    assert same(a, s1.sample_seeded(None, seeds, 77)) and same(a, s2.sample_seeded(None, seeds, 77))
    assert not same(a, s1.sample_seeded(None, seeds, 78))
    np.random.seed(4)
    seq = [s1.sample(None, seeds) for _ in range(3)]
    np.random.seed(4)
    assert all(same(x, s2.sample(None, seeds)) for x in seq) and not same(seq[0], seq[1])
    # the device draws the restatement's subsets: the same uniformity statistic as tests/test_neighbor_host.py
    counts = np.bincount(a[0].cpu().numpy()[a[2][0].col.cpu().numpy()] - 5000, minlength=12)
    exp = 4096 * 5 / 12
    assert float(((counts - exp) ** 2 / exp).sum()) < 31.26


def test_edge_cases(main_graph, cuda_device):
    from dgll_amd.sampling import NeighborSampler

    rowptr, col, n, g = main_graph
    s = NeighborSampler([5, 2], g)
    inp, out, blocks = s.sample_seeded(None, np.zeros(0, np.int64), 1)             # no seeds: empty blocks of consistent shapes
    assert inp.numel() == 0 and inp.dtype == torch.int64 and len(blocks) == 2
    for b in blocks:
        assert (b.n_rows, b.n_cols, b.nnz) == (0, 0, 0) and b.rowptr.tolist() == [0] and b.col.dtype == torch.int32 and b.val.numel() == 0
    isolated = np.arange(0, n, 16)[:20][::-1].copy()                                # degree 0, every one
    assert not (rowptr[isolated + 1] - rowptr[isolated]).any()
    inp, blocks = run_case(main_graph, [5, 2], isolated, 2)
    assert np.array_equal(inp.cpu().numpy(), isolated) and all(b.nnz == 0 and b.n_rows == b.n_cols == 20 for b in blocks)
    with pytest.raises(ValueError, match="duplicate"):
        s.sample_seeded(None, [3, 9, 3], 1)
    for bad in ([3, n], [-1, 4]):
        with pytest.raises(ValueError, match="outside"):
            s.sample_seeded(None, bad, 1)
    bad_col = col.copy()
    bad_col[rowptr[9]] = n + 5                                                      # a column id of the graph itself out of range
    with pytest.raises(ValueError, match="outside"):
        NeighborSampler([-1], device_graph(rowptr, bad_col, n, cuda_device)).sample_seeded(None, [9], 1)
    with pytest.raises(ValueError, match="outside"):
        NeighborSampler([64], device_graph(rowptr, bad_col, n, cuda_device)).sample_seeded(None, [9], 1)
    run_case(main_graph, [5, 2], np.array([n - 1, 3, 9]), 1)                        # and the sampler still works afterwards


def load_example():
    spec = importlib.util.spec_from_file_location("neighbor_example_train", os.path.join(ROOT, "examples", "neighbor", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def test_one_batch_matches_float64_autograd(hub_graph, cuda_device):
    """The example's two-layer SAGE-mean model on one batch against float64 CPU autograd on the same blocks; tolerance 1e-4 as
    test_layerwise_gpu.py::test_one_batch_matches_float64_autograd (fp32)."""
    from dgll_amd import ops
    from dgll_amd.sampling import NeighborSampler, layerwise

    rowptr, col, n, g = hub_graph
    torch.manual_seed(0)
    s = NeighborSampler([10, 25], g)
    seeds = pick_seeds(n, 1023, [4000, n - 1], 21)
    inp, _, blocks = s.sample_seeded(None, seeds, 21)
    layerwise.record_stream(blocks, inp, torch.cuda.current_stream(cuda_device))
    x_all = torch.randn(n, 50)
    labels = torch.randint(0, 7, (1023,))
    model = load_example().SageMean(50, 128, 7).to(cuda_device)
    logits = model(blocks, x_all[inp.cpu()].to(cuda_device))
    ops.cross_entropy(logits, labels.to(cuda_device)).backward()
    dense = lambda b: torch.sparse_csr_tensor(b.rowptr.cpu(), b.col.long().cpu(), b.val.double().cpu(), (b.n_rows, b.n_cols)).to_dense()   # noqa: E731
    P = {k: v.detach().cpu().double().requires_grad_() for k, v in model.named_parameters()}
    h = x_all[inp.cpu()].double()
    for i, b in enumerate(blocks):
        h = h[:b.n_rows] @ P["w_self.%d.weight" % i].T + P["w_self.%d.bias" % i] + (dense(b) @ h) @ P["w_neigh.%d.weight" % i].T
        if i == 0:
            h = torch.relu(h)
    torch.nn.functional.cross_entropy(h, labels).backward()
    assert rel(logits.detach().cpu(), h.detach()) < 1e-4
    for k, prm in model.named_parameters():
        assert rel(prm.grad.cpu(), P[k].grad) < 1e-4, k


def test_pipeline_equals_serial_sampling(hub_graph, cuda_device):
    """MiniBatchPipeline with per-batch seeds (sampler_threads, fast_sampler.batch_seed) over 8 batches yields the blocks of serial
    sample_seeded calls, and the features of their input nodes."""
    from dgll_amd.cache import GraphCacheServer
    from dgll_amd.data import DGraph
    from dgll_amd.dataloader import DataLoader
    from dgll_amd.pipeline import MiniBatchPipeline
    from dgll_amd.sampling import NeighborSampler, layerwise
    from dgll_amd.sampling.fast_sampler import batch_seed

    rowptr, col, n, g = hub_graph
    x = torch.randn(n, 16)
    y = torch.arange(n) % 4
    dg = DGraph.from_csr(rowptr, col.astype(np.int64), labels=y, features=x)
    s = NeighborSampler([4, 4], dg)
    assert torch.equal(s.graph.rowptr.cpu(), torch.as_tensor(rowptr)) and torch.equal(s.graph.col.cpu(), torch.as_tensor(col))
    srv = GraphCacheServer(x, gpuid=0)
    srv.auto_cache(torch.as_tensor(np.diff(rowptr)), capacity=2000)
    train = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:8 * 100 - 30]
    serial = [s.sample_seeded(dg, train[i:i + 100], batch_seed(5, 2, i // 100)) for i in range(0, len(train), 100)]
    loader = DataLoader(dg, train, s, batch_size=100)
    pipe = MiniBatchPipeline(loader, cache=srv, labels=y, queue_size=2, device=cuda_device, sampler_threads=2, base_seed=5, epoch=2)
    cur = torch.cuda.current_stream(cuda_device)
    got = 0
    for b, want in zip(pipe, serial):
        layerwise.record_stream(b.subgraphs, b.input_nodes, cur)
        assert same((b.input_nodes, None, b.subgraphs), want)
        assert torch.equal(b.features[0].cpu(), x[b.input_nodes.cpu()])
        assert torch.equal(b.labels.cpu(), y[want[1]])
        got += 1
    assert got == len(serial) == 8


def test_example_trains():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "neighbor", "train.py"), "--nodes", "20000", "--epochs", "3"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    losses = [float(line.split("loss")[1].split()[0]) for line in res.stdout.splitlines() if line.startswith("epoch")]
    assert len(losses) == 3 and losses[-1] < losses[0], losses
