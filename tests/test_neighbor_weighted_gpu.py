"""Edge-weighted device neighbour sampling (NeighborSampler(prob=...), dgll_hip_nb_sample_weighted) on the MI355X: bit-equality with
the numpy restatement (tests/neighbor_weighted_ref.py) wherever the restatement's keys are far enough apart -- asserted first, on
the restatement alone --, the block contract on the filtered graph, the workgroup kernel of the long rows, the distribution of the
kept sets, batch independence, determinism, the untouched uniform path, edge cases, the pipeline and the example.

The fan-out lists run the lane-group kernel at both widths (16 lanes for f <= 16, the wavefront above) and, through the hub of 5000
in-neighbours and the rows of dgll_hip_nb_long_row() + 1 entries, the workgroup kernel.  One seed serves every case of a graph: a
node's keys depend on (seed, layer, node, row) only, so the restatement computes them once."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import neighbor_ref as ref
import neighbor_weighted_ref as wref
from conftest import ROOT
from test_neighbor_gpu import as_dicts, assert_bit_equal, pick_seeds, same

pytestmark = pytest.mark.gpu

FANOUTS = [[1], [5, 2], [25, 10, 10], [-1, 3], [64]]
SEED_COUNTS = [1, 65, 600]
MAIN_SEED, LONG_SEED = 0x1234567890ABCDEF, 99


def device_graph(rowptr, col, w, n, device):
    from dgll_amd.graph import CSRGraph

    return CSRGraph(torch.as_tensor(rowptr), torch.as_tensor(col), None if w is None else torch.as_tensor(w), n, n).to(device)


@pytest.fixture(scope="module")
def main_graph(cuda_device):
    """1003 nodes, degrees 0 .. 65 and a hub of 1000; weights 2^-20 .. 2^31, a third of the rows with zero weights (not the hub and
    not the last node, which is the seed of the one-seed cases)."""
    rowptr, col, n = wref.build_graph(1003, {500: 1000}, seed=5)
    w = wref.build_weights(rowptr, 7, keep_whole=(500, 1002))
    return rowptr, col, w, n, device_graph(rowptr, col, w, n, cuda_device)


@pytest.fixture(scope="module")
def long_graph(cuda_device):
    """6007 nodes: a hub of 5000 in-neighbours, rows of exactly L and L + 1 entries (L = dgll_hip_nb_long_row()), no zero weights
    in those three rows."""
    from dgll_amd import _lib

    L = int(_lib.lib.dgll_hip_nb_long_row())
    rowptr, col, n = wref.build_graph(6007, {4000: 5000, 4001: L, 4003: L + 1}, seed=6)
    w = wref.build_weights(rowptr, 8, keep_whole=(4000, 4001, 4003))
    for v in (4000, 4001, 4003):
        assert (w[rowptr[v]:rowptr[v + 1]] > 0).all()
    return rowptr, col, w, n, device_graph(rowptr, col, w, n, cuda_device), L


def run_case(graph, fanouts, seeds, seed, norm="mean", prob="weight"):
    from dgll_amd.sampling import NeighborSampler

    rowptr, col, w, n, g = graph[:5]
    want_inp, want, min_gap, (frp, fcol, fw) = wref.sample_blocks(rowptr, col, w, seeds, fanouts, seed, norm)
    print("smallest relative key gap of the restatement", min_gap)
    assert min_gap > wref.MIN_GAP                                    # the precondition of bit equality, on the restatement alone
    ref.check_invariants(frp, fcol, seeds, fanouts, want_inp, want, norm)
    s = NeighborSampler(fanouts, g, prob=torch.as_tensor(w) if prob == "tensor" else prob, norm=norm)
    assert np.array_equal(s.graph.rowptr.cpu().numpy(), frp) and np.array_equal(s.graph.col.cpu().numpy(), fcol)
    assert np.array_equal(s.graph.val.cpu().numpy(), fw)             # the filtered graph stays reachable
    inp, out, blocks = s.sample_seeded(None, seeds, seed)
    assert out is seeds and blocks[-1].n_rows == len(seeds)
    assert_bit_equal(inp, blocks, want_inp, want)
    ref.check_invariants(frp, fcol, seeds, fanouts, inp.cpu().numpy(), as_dicts(inp, blocks), norm)
    return inp, blocks


def main_must(rowptr, w, n):
    """The last node, the hub, a self-loop, an isolated node, and a row whose weights are all 0."""
    pos = np.array([(w[rowptr[v]:rowptr[v + 1]] > 0).sum() for v in range(n)])
    all_zero = int(np.nonzero((np.diff(rowptr) >= 2) & (pos == 0))[0][0])
    return [n - 1, 500, 0, 7, 16, all_zero]


@pytest.mark.parametrize("count", SEED_COUNTS)
@pytest.mark.parametrize("fanouts", FANOUTS, ids=str)
def test_bit_equal_to_the_restatement(fanouts, count, main_graph):
    rowptr, col, w, n, _ = main_graph
    must = main_must(rowptr, w, n)
    seeds = pick_seeds(n, count, must[:1] if count == 1 else must, 100 + count)
    run_case(main_graph, fanouts, seeds, MAIN_SEED)


def test_the_graph_has_the_rows_the_cases_need(main_graph):
    rowptr, col, w, n, _ = main_graph
    deg = np.diff(rowptr)
    pos = np.array([(w[rowptr[v]:rowptr[v + 1]] > 0).sum() for v in range(n)])
    assert w[w > 0].max() / w[w > 0].min() > 2.0 ** 45 and ((pos == 0) & (deg >= 2)).any()
    for f in (1, 2, 3, 5, 10, 25, 64):
        for k in (f - 1, f, f + 1):                                  # fewer than f, exactly f, f + 1 positive weights, zeros present
            assert (pos == k).any() and (deg == k).any(), (f, k)     # by zeros or by degree
            assert k == 65 or ((pos == k) & (deg > k)).any(), (f, k)  # zeros present (the hub, the only longer row, has none)


def test_prob_tensor_and_no_values(main_graph):
    rowptr, col, w, n, g = main_graph
    seeds = pick_seeds(n, 65, [n - 1, 500], 3)
    run_case(main_graph, [5, 2], seeds, MAIN_SEED, norm=None, prob="tensor")


@pytest.mark.parametrize("fanouts", [[25, 10, 10], [64]], ids=str)
def test_long_rows(fanouts, long_graph):
    """The hub of 5000 and the row of L + 1 entries go to the workgroup kernel, the row of L entries stays with the lane groups."""
    rowptr, col, w, n, _, L = long_graph
    assert [int(rowptr[v + 1] - rowptr[v]) for v in (4000, 4001, 4003)] == [5000, L, L + 1]
    seeds = pick_seeds(n, 24, [4000, 4001, 4003, n - 1], 7)
    inp, blocks = run_case(long_graph, fanouts, seeds, LONG_SEED)
    outer, dst = blocks[0], inp[:blocks[0].n_rows].cpu().numpy()
    for v in (4000, 4001, 4003):                                     # seeds are destinations of every layer
        r = int(np.nonzero(dst == v)[0][0])
        assert int(outer.rowptr[r + 1] - outer.rowptr[r]) == fanouts[0]


def test_kept_sets_follow_plackett_luce(cuda_device):
    """One launch over 20 000 rows that list the same 7 neighbours: the zero-weight one never appears, the 20 kept sets have
    Plackett-Luce counts, and they are the restatement's sets (whose statistic test_neighbor_weighted_host.py checks too)."""
    from dgll_amd.sampling import NeighborSampler

    rowptr, col, w, n = wref.dist_graph()
    want, min_gap = wref.dist_reference()
    assert min_gap > wref.MIN_GAP
    s = NeighborSampler([wref.DIST_FANOUT], device_graph(rowptr, col, w, n, cuda_device), prob="weight")
    inp, _, blocks = s.sample_seeded(None, np.arange(wref.DIST_ROWS), wref.DIST_SEED)
    b = blocks[0]
    assert b.nnz == wref.DIST_ROWS * wref.DIST_FANOUT and torch.equal(b.rowptr.cpu(), torch.arange(wref.DIST_ROWS + 1) * wref.DIST_FANOUT)
    ids = inp.cpu().numpy()[b.col.cpu().numpy()].reshape(wref.DIST_ROWS, wref.DIST_FANOUT) - wref.DIST_ROWS
    sets = [tuple(sorted(int(i) for i in row)) for row in ids]
    wref.check_set_counts(sets)
    assert sets == want


def test_a_draw_does_not_depend_on_the_batch(main_graph):
    from dgll_amd.sampling import NeighborSampler

    rowptr, col, w, n, g = main_graph
    frp, fcol, fw = wref.drop_zero_weights(rowptr, col, w)
    s = NeighborSampler([10], g, prob="weight")
    big = pick_seeds(n, 600, [n - 1, 500, 26, 65], 11)
    inp_b, _, blk_b = s.sample_seeded(None, big, 31)
    src_b, b = inp_b.cpu().numpy(), blk_b[0]
    for v in (500, 26, 65, n - 1, int(big[599])):
        inp_1, _, blk_1 = s.sample_seeded(None, [v], 31)
        alone = set(inp_1.cpu().numpy()[blk_1[0].col.cpu().numpy()].tolist())
        r = int(np.nonzero(big == v)[0][0])
        inside = set(src_b[b.col[int(b.rowptr[r]):int(b.rowptr[r + 1])].cpu().numpy()].tolist())
        ids, gap = wref.draw(frp, fcol, fw, v, 10, 31, 0)
        assert gap is None or gap > wref.MIN_GAP
        assert alone == inside == set(ids)


def test_same_seed_same_bits_other_seed_other_sample(main_graph):
    from dgll_amd.sampling import NeighborSampler

    g, n = main_graph[4], main_graph[3]
    seeds = pick_seeds(n, 600, [n - 1, 500], 13)
    s1, s2 = NeighborSampler([25, 10], g, prob="weight"), NeighborSampler([25, 10], g, prob="weight")
    a = s1.sample_seeded(None, seeds, 77)
    assert same(a, s1.sample_seeded(None, seeds, 77)) and same(a, s2.sample_seeded(None, seeds, 77))
    assert not same(a, s1.sample_seeded(None, seeds, 78))
    np.random.seed(4)
    seq = [s1.sample(None, seeds) for _ in range(3)]
    np.random.seed(4)
    assert all(same(x, s2.sample(None, seeds)) for x in seq) and not same(seq[0], seq[1])


def test_uniform_path_untouched(main_graph):
    """prob=None on the weighted graph: the uniform sampler's blocks, the graph bound as it is."""
    from dgll_amd.sampling import NeighborSampler

    rowptr, col, w, n, g = main_graph
    seeds = pick_seeds(n, 65, [n - 1, 500, 0], 5)
    s = NeighborSampler([25, 10, 10], g)
    assert s.graph is g and s.prob is None
    inp, _, blocks = s.sample_seeded(None, seeds, 42)
    want_inp, want = ref.sample_blocks(rowptr, col, seeds, [25, 10, 10], 42)
    assert_bit_equal(inp, blocks, want_inp, want)


def test_edge_cases(main_graph, cuda_device):
    from dgll_amd.sampling import NeighborSampler

    rowptr, col, w, n, g = main_graph
    s = NeighborSampler([5, 2], g, prob="weight")
    inp, out, blocks = s.sample_seeded(None, np.zeros(0, np.int64), 1)             # no seeds: empty blocks of consistent shapes
    assert inp.numel() == 0 and inp.dtype == torch.int64 and len(blocks) == 2
    for b in blocks:
        assert (b.n_rows, b.n_cols, b.nnz) == (0, 0, 0) and b.rowptr.tolist() == [0] and b.col.dtype == torch.int32 and b.val.numel() == 0
    isolated = np.arange(0, n, 16)[:20][::-1].copy()                                # degree 0, every one
    assert not (rowptr[isolated + 1] - rowptr[isolated]).any()
    inp, blocks = run_case(main_graph, [5, 2], isolated, MAIN_SEED)
    assert np.array_equal(inp.cpu().numpy(), isolated) and all(b.nnz == 0 and b.n_rows == b.n_cols == 20 for b in blocks)
    pos = np.array([(w[rowptr[v]:rowptr[v + 1]] > 0).sum() for v in range(n)])
    zero_rows = np.nonzero((np.diff(rowptr) >= 2) & (pos == 0))[0]                  # neighbours, but every weight 0
    assert len(zero_rows) >= 3
    for fanouts in ([5, 2], [-1, 3]):
        inp, blocks = run_case(main_graph, fanouts, zero_rows, MAIN_SEED)
        assert np.array_equal(inp.cpu().numpy(), zero_rows) and all(b.nnz == 0 and b.n_rows == b.n_cols == len(zero_rows) for b in blocks)
    with pytest.raises(ValueError, match="duplicate"):
        s.sample_seeded(None, [3, 9, 3], 1)
    with pytest.raises(ValueError, match="outside"):
        s.sample_seeded(None, [3, n], 1)
    with pytest.raises(ValueError, match="values"):
        NeighborSampler([5], device_graph(rowptr, col, None, n, cuda_device), prob="weight")
    for bad in (w[:-1], -w, np.where(np.arange(len(w)) == 5, np.nan, w)):
        with pytest.raises(ValueError, match="weight"):
            NeighborSampler([5], g, prob=bad)
    run_case(main_graph, [5, 2], np.array([n - 1, 3, 9]), MAIN_SEED)                # and the sampler still works afterwards


def test_pipeline_equals_serial_sampling(long_graph, cuda_device):
    """MiniBatchPipeline with per-batch seeds over 4 batches yields the blocks of serial sample_seeded calls (shaped on
    test_neighbor_gpu.test_pipeline_equals_serial_sampling)."""
    from dgll_amd.cache import GraphCacheServer
    from dgll_amd.data import DGraph
    from dgll_amd.dataloader import DataLoader
    from dgll_amd.pipeline import MiniBatchPipeline
    from dgll_amd.sampling import NeighborSampler, layerwise
    from dgll_amd.sampling.fast_sampler import batch_seed

    rowptr, col, w, n, g, _ = long_graph
    x = torch.randn(n, 16)
    y = torch.arange(n) % 4
    dg = DGraph.from_csr(rowptr, col.astype(np.int64), labels=y, features=x)
    s = NeighborSampler([4, 4], g, prob="weight")
    srv = GraphCacheServer(x, gpuid=0)
    srv.auto_cache(torch.as_tensor(np.diff(rowptr)), capacity=2000)
    train = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:4 * 100 - 30]
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
    assert got == len(serial) == 4


def test_example_trains_weighted():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "neighbor", "train.py"), "--nodes", "20000", "--epochs", "3",
                          "--weighted"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    losses = [float(line.split("loss")[1].split()[0]) for line in res.stdout.splitlines() if line.startswith("epoch")]
    assert len(losses) == 3 and losses[-1] < losses[0], losses
