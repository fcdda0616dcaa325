"""Link prediction on the MI355X (dgll_amd/csrc/edge_pred.hip): the edge sampler bit-equal to the numpy restatement
(tests/edge_pred_ref.py) -- pairs, negatives, capped count, output nodes, blocks after exclusion, incidence --, its invariants and
determinism, pair_dot against float64 within the fp32 accumulation bound, one training batch against float64 autograd, the example.

Graph: the 1003-node recipe of test_neighbor_gpu.build_graph (degrees 0 .. 65, a hub of 1000 in-neighbours, self-loops, N no
multiple of 32; node N - 1 is a source of 13 rows in 16, which is what makes filtered negatives of its edges run out of attempts)."""
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import edge_pred_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

N, HUB = 1003, 500
BATCHES = [1, 63, 64, 65, 257]
NEGATIVES = [0, 1, 5]
FANOUTS = [[5, 2], [-1, 3]]


@functools.lru_cache(maxsize=None)
def host_graph():
    return ref.build_graph(N, hub=HUB, hub_degree=1000, seed=5)


@pytest.fixture(scope="module")
def graph(cuda_device):
    from dgll_amd.graph import CSRGraph

    rowptr, col, n = host_graph()
    return CSRGraph(torch.as_tensor(rowptr), torch.as_tensor(col), None, n, n).to(cuda_device)


@functools.lru_cache(maxsize=None)
def pick_edges(count):
    """A batch with entry 0, entry nnz - 1, two entries of the hub row, a self-loop edge, a duplicated edge and (half of it) edges whose
    source is node N - 1; one edge: the first of those."""
    rowptr, col, n = host_graph()
    nnz = len(col)
    from_last = np.nonzero(col == n - 1)[0]
    if count == 1:
        return from_last[:1].copy()
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    loop = int(np.nonzero(rows == col)[0][3])
    must = np.asarray([0, nnz - 1, rowptr[HUB], rowptr[HUB] + 777, loop, loop], np.int64)
    rng = np.random.default_rng(count)
    rest = np.concatenate([rng.choice(from_last, count // 2, replace=False), rng.integers(0, nnz, count)])
    return rng.permutation(np.concatenate([must, rest])[:count])


@functools.lru_cache(maxsize=None)
def restatement(count, negatives, filter_existing, fanouts):
    """The restatement of one batch WITHOUT exclusion, computed once and left unchanged (exclusion is applied per case)."""
    rowptr, col, n = host_graph()
    return ref.sample(rowptr, col, n, pick_edges(count), list(fanouts), 0xC0FFEE + count, negatives, filter_existing)


def as_dicts(input_nodes, blocks):
    out, src = [], input_nodes.cpu().numpy()
    for b in blocks:
        out.append({"rowptr": b.rowptr.cpu().numpy(), "col": b.col.cpu().numpy(), "val": None if b.val is None else b.val.cpu().numpy(),
                    "n_rows": b.n_rows, "n_cols": b.n_cols, "src": src[:b.n_cols], "dst": src[:b.n_rows]})
        src = src[:b.n_rows]
    return out


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("exclude", [None, "self", "reverse"])
@pytest.mark.parametrize("filter_existing", [False, True])
@pytest.mark.parametrize("negatives", NEGATIVES)
@pytest.mark.parametrize("count", BATCHES)
@pytest.mark.parametrize("fanouts", FANOUTS, ids=str)
def test_bit_equal_to_the_restatement(fanouts, count, negatives, filter_existing, exclude, graph):
    from dgll_amd.sampling import EdgePredictionSampler, NeighborSampler

    rowptr, col, n = host_graph()
    eids = pick_edges(count)
    want = restatement(count, negatives, filter_existing, tuple(fanouts))
    s = EdgePredictionSampler(NeighborSampler(fanouts, graph), negatives=negatives, filter_existing=filter_existing, exclude=exclude)
    inp, batch, blocks = s.sample_seeded(None, eids, 0xC0FFEE + count)
    assert batch.output_nodes.dtype == torch.int64 and batch.pairs.dtype == torch.int32
    assert (batch.n_pos, batch.n_neg) == (count, count * negatives) and tuple(batch.pairs.shape) == (count * (1 + negatives), 2)
    out, pairs = batch.output_nodes.cpu().numpy(), batch.pairs.cpu().numpy()
    assert np.array_equal(out, want["output_nodes"]) and np.array_equal(pairs, want["pairs"])
    assert np.array_equal(out[pairs], want["gpairs"])
    assert batch.capped == want["capped"]
    if filter_existing and negatives == 5 and count >= 63:
        assert batch.capped > 0                                                   # edges from node N - 1: the capped path ran
    if not filter_existing or negatives == 0:
        assert batch.capped == 0
    assert torch.equal(batch.labels().cpu(), torch.cat([torch.ones(count), torch.zeros(count * negatives)]))
    want_blocks = [ref.exclude(b, want["gpairs"][:count], exclude) for b in want["blocks"]]
    assert np.array_equal(inp.cpu().numpy(), want["input_nodes"]) and len(blocks) == len(want_blocks)
    for g, w in zip(blocks, want_blocks):
        assert g.rowptr.dtype == torch.int64 and g.col.dtype == torch.int32 and g.val.dtype == torch.float32
        assert (g.n_rows, g.n_cols) == (w["n_rows"], w["n_cols"])
        assert np.array_equal(g.rowptr.cpu().numpy(), w["rowptr"]) and np.array_equal(g.col.cpu().numpy(), w["col"])
        assert np.array_equal(bits(g.val.cpu().numpy()), bits(w["val"]))
    for got, w in zip(batch.incidence(), ref.incidence(want["pairs"], len(out))):
        assert np.array_equal(got.cpu().numpy(), w) and got.dtype == (torch.int64 if w.dtype == np.int64 else torch.int32)
    ref.check_invariants(rowptr, col, n, out, pairs, count, as_dicts(inp, blocks), filter_existing, exclude, want["capped_flags"])
    if exclude is not None and fanouts[0] < 0:     # the outer block holds every in-neighbour of every endpoint: each positive is in it
        assert sum(b.nnz for b in blocks) < sum(len(b["col"]) for b in want["blocks"])


def test_the_restatement_meets_the_cases_the_batches_are_built_for():
    rowptr, col, n = host_graph()
    e = pick_edges(257)
    rows = np.asarray([ref.row_of(rowptr, x) for x in e])
    assert 0 in e and len(col) - 1 in e and (rows == HUB).sum() >= 2 and (rows == col[e]).any() and len(np.unique(e)) < len(e)
    assert (col[e] == n - 1).sum() >= 128
    assert all(restatement(c, 5, True, (5, 2))["capped"] > 0 for c in BATCHES if c >= 63)
    assert col[pick_edges(1)[0]] == n - 1


def test_same_seed_same_bits_other_seed_other_negatives(graph):
    from dgll_amd.sampling import EdgePredictionSampler, NeighborSampler

    eids = pick_edges(257)

    def run(s, seed):
        inp, b, blocks = s.sample_seeded(None, eids, seed)
        return inp, b, blocks, b.output_nodes[b.pairs.long()]

    def same(a, b):
        return (torch.equal(a[0], b[0]) and torch.equal(a[1].pairs, b[1].pairs) and torch.equal(a[1].output_nodes, b[1].output_nodes)
                and a[1].capped == b[1].capped
                and all(torch.equal(x.rowptr, y.rowptr) and torch.equal(x.col, y.col) and torch.equal(x.val, y.val) for x, y in zip(a[2], b[2])))

    mk = lambda: EdgePredictionSampler(NeighborSampler([5, 2], graph), negatives=5, filter_existing=True, exclude="reverse")   # noqa: E731
    s1, s2 = mk(), mk()
    a = run(s1, 77)
    assert same(a, run(s1, 77)) and same(a, run(s2, 77))
    c = run(s1, 78)
    assert torch.equal(a[3][:257], c[3][:257]) and not torch.equal(a[3][257:], c[3][257:])     # the positives stay, the negatives move
    np.random.seed(4)
    seq = [s1.sample(None, eids) for _ in range(2)]
    np.random.seed(4)
    again = s2.sample(None, eids)
    assert torch.equal(seq[0][1].pairs, again[1].pairs) and torch.equal(seq[0][0], again[0])
    assert not torch.equal(seq[0][1].output_nodes[seq[0][1].pairs.long()], seq[1][1].output_nodes[seq[1][1].pairs.long()])
    # a pair's negatives do not depend on the batch
    one = EdgePredictionSampler(NeighborSampler([5, 2], graph), negatives=5, filter_existing=True).sample_seeded(None, eids[10:11], 77)[1]
    assert torch.equal(one.output_nodes[one.pairs.long()][1:], a[3][257 + 50:257 + 55])


def test_edge_cases(graph, cuda_device):
    from dgll_amd.graph import CSRGraph
    from dgll_amd.sampling import EdgePredictionSampler, NeighborSampler

    rowptr, col, n = host_graph()
    s = EdgePredictionSampler(NeighborSampler([5, 2], graph), negatives=2, exclude="self")
    inp, batch, blocks = s.sample_seeded(None, np.zeros(0, np.int64), 1)          # no edges: an empty batch of consistent shapes
    assert len(batch) == 0 and batch.output_nodes.numel() == 0 and tuple(batch.pairs.shape) == (0, 2) and inp.numel() == 0
    assert len(blocks) == 2 and all(b.nnz == 0 and b.n_rows == 0 for b in blocks)
    for bad in ([3, len(col)], [-1, 4]):
        with pytest.raises(ValueError, match="edge id"):
            s.sample_seeded(None, bad, 1)
    bad_col = col.copy()
    bad_col[rowptr[9]] = n + 5
    sb = EdgePredictionSampler(NeighborSampler([5], CSRGraph(torch.as_tensor(rowptr), torch.as_tensor(bad_col), None, n, n).to(cuda_device)))
    with pytest.raises(ValueError, match="column id"):
        sb.sample_seeded(None, [int(rowptr[9])], 1)
    swapped = col.copy()
    swapped[[rowptr[20], rowptr[20] + 1]] = swapped[[rowptr[20] + 1, rowptr[20]]]                 # one row out of order
    unsorted = CSRGraph(torch.as_tensor(rowptr), torch.as_tensor(swapped), None, n, n).to(cuda_device)
    with pytest.raises(ValueError, match="ascending"):
        EdgePredictionSampler(NeighborSampler([5], unsorted), filter_existing=True)
    EdgePredictionSampler(NeighborSampler([5], unsorted), filter_existing=False).sample_seeded(None, [0, 5], 1)      # unfiltered: no order needed
    inp, batch, blocks = s.sample_seeded(None, [0, 7, 7], 3)                      # and the sampler still works after the refusals
    want = ref.sample(rowptr, col, n, [0, 7, 7], [5, 2], 3, 2, False, "self")
    assert np.array_equal(batch.pairs.cpu().numpy(), want["pairs"]) and np.array_equal(inp.cpu().numpy(), want["input_nodes"])
    assert all(np.array_equal(b.col.cpu().numpy(), w["col"]) for b, w in zip(blocks, want["blocks"]))


# ---- pair_dot ---------------------------------------------------------------------------------------------------------------------
M = 301


@functools.lru_cache(maxsize=None)
def dot_case(n_pairs, feat, dtype_name):
    """Operands as stored (float64 views), pairs, score gradient and the float64 results with their absolute sums."""
    rng = np.random.default_rng(1000 * n_pairs + feat)
    dtype = getattr(torch, dtype_name)
    h = torch.from_numpy(rng.standard_normal((M, feat)).astype(np.float32)).to(dtype)
    pairs = rng.integers(0, M - 1, (n_pairs, 2)).astype(np.int32)                # node M - 1 is in no pair
    if n_pairs >= 64:
        pairs[1], pairs[2] = (5, 5), (7, 7)
    g = rng.standard_normal(n_pairs).astype(np.float32)
    h64 = h.double().numpy()
    a, b = h64[pairs[:, 0]], h64[pairs[:, 1]]
    score, score_abs = (a * b).sum(1), np.abs(a * b).sum(1)
    grad, grad_abs, deg = np.zeros((M, feat)), np.zeros((M, feat)), np.zeros(M)
    for slot in (0, 1):
        np.add.at(grad, pairs[:, slot], g[:, None].astype(np.float64) * h64[pairs[:, 1 - slot]])
        np.add.at(grad_abs, pairs[:, slot], np.abs(g[:, None].astype(np.float64) * h64[pairs[:, 1 - slot]]))
        np.add.at(deg, pairs[:, slot], 1)
    return h, pairs, g, score, score_abs, grad, grad_abs, deg


@pytest.mark.parametrize("layout", ["packed", "padded"])
@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("feat", [1, 7, 47, 64, 100, 256, 602])
@pytest.mark.parametrize("n_pairs", [1, 64, 65, 1000])
def test_pair_dot_against_float64(n_pairs, feat, dtype_name, layout, cuda_device):
    """Forward |err| <= (F + 2) 2^-24 sum|a_i b_i|; backward |err| <= (deg_i + 2) 2^-24 sum|g h| per element, plus 2^-8 |value| for a
    bf16 result's final rounding (bf16's unit roundoff: that term alone can be reached, the accumulation term is the slack -- enough
    up to 512 incidence entries per node, the cases have a few dozen at most); the backward bit-identical across two runs.
    Measured on an MI355X, largest err / bound over all cases: forward 0.32, backward 0.996 (bf16; fp32 below 0.5)."""
    from dgll_amd import ops

    h_cpu, pairs, g, score, score_abs, grad, grad_abs, deg = dot_case(n_pairs, feat, dtype_name)
    if layout == "padded":                        # rows on a wider pitch, NaN behind the last column: read as they are, padding masked
        per = 16 // h_cpu.element_size()
        store = torch.full((M, (feat + per - 1) // per * per + per), float("nan"), dtype=h_cpu.dtype, device=cuda_device)
        store[:, :feat] = h_cpu.to(cuda_device)
        h = store[:, :feat]
        assert ops.rows16_ok(h)
    else:
        h = h_cpu.to(cuda_device)
    h.requires_grad_()
    p_dev, g_dev = torch.as_tensor(pairs).to(cuda_device), torch.as_tensor(g).to(cuda_device)
    out = ops.pair_dot(h, p_dev)
    assert out.dtype == torch.float32 and tuple(out.shape) == (n_pairs,)
    err = np.abs(out.detach().cpu().double().numpy() - score)
    bound = (feat + 2) * 2.0 ** -24 * score_abs
    print("forward: max err / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)
    (gh,) = torch.autograd.grad(out, h, g_dev)
    assert gh.dtype == h.dtype and tuple(gh.shape) == (M, feat)
    berr = np.abs(gh.cpu().double().numpy() - grad)
    bbound = (deg[:, None] + 2) * 2.0 ** -24 * grad_abs + (2.0 ** -8 * np.abs(grad) if dtype_name == "bfloat16" else 0.0)
    print("backward: max err / bound", float((berr / np.maximum(bbound, 1e-300)).max()))
    assert np.all(berr <= bbound)
    assert not gh[M - 1].any() and deg[M - 1] == 0                                # a node in no pair: a zero gradient row
    (gh2,) = torch.autograd.grad(ops.pair_dot(h, p_dev), h, g_dev)
    assert torch.equal(gh.view(torch.int16 if dtype_name == "bfloat16" else torch.int32),
                       gh2.view(torch.int16 if dtype_name == "bfloat16" else torch.int32))


def test_pair_dot_refuses_bad_pairs(cuda_device):
    from dgll_amd import ops
    from dgll_amd.sampling import PairBatch

    h = torch.randn(8, 16, device=cuda_device)
    for bad in (torch.tensor([[0, 8]]), torch.tensor([[-1, 2]])):
        with pytest.raises(ValueError, match="outside"):
            ops.pair_dot(h, bad.to(cuda_device))
    with pytest.raises(ValueError, match=r"\[P, 2\]"):
        ops.pair_dot(h, torch.zeros(3, 3, dtype=torch.int32, device=cuda_device))
    with pytest.raises(ValueError, match="output nodes"):
        ops.pair_dot(h, PairBatch(torch.arange(5, device=cuda_device), torch.zeros((1, 2), dtype=torch.int32, device=cuda_device), 1, 0))
    with pytest.raises(TypeError):
        ops.pair_dot(h.double(), torch.tensor([[0, 1]], device=cuda_device))
    assert ops.pair_dot(h, torch.zeros((0, 2), dtype=torch.int32, device=cuda_device)).numel() == 0


# ---- training numerics and the example ----------------------------------------------------------------------------------------------
def load_example():
    spec = importlib.util.spec_from_file_location("linkpred_example_train", os.path.join(ROOT, "examples", "linkpred", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def test_one_batch_matches_float64_autograd(graph, cuda_device):
    """The example's two-layer SAGE-mean model, pair_dot and BCE on one sampled batch against float64 CPU autograd on the same blocks and
    pairs; relative error of the scores and of every parameter gradient below 1e-4, the bar of test_neighbor_gpu.py (fp32)."""
    from dgll_amd import ops
    from dgll_amd.sampling import EdgePredictionSampler, NeighborSampler, layerwise

    torch.manual_seed(0)
    s = EdgePredictionSampler(NeighborSampler([10, 25], graph), negatives=5, filter_existing=True, exclude="reverse")
    inp, batch, blocks = s.sample_seeded(None, pick_edges(257), 21)
    cur = torch.cuda.current_stream(cuda_device)
    layerwise.record_stream(blocks, inp, cur)
    batch.record_stream(cur)
    x_all = torch.randn(N, 50)
    model = load_example().SageMean(50, 128, 64).to(cuda_device)
    scores = ops.pair_dot(model(blocks, x_all[inp.cpu()].to(cuda_device)), batch)
    torch.nn.functional.binary_cross_entropy_with_logits(scores, batch.labels()).backward()
    dense = lambda b: torch.sparse_csr_tensor(b.rowptr.cpu(), b.col.long().cpu(), b.val.double().cpu(), (b.n_rows, b.n_cols)).to_dense()   # noqa: E731
    P = {k: v.detach().cpu().double().requires_grad_() for k, v in model.named_parameters()}
    h = x_all[inp.cpu()].double()
    for i, b in enumerate(blocks):
        h = h[:b.n_rows] @ P["w_self.%d.weight" % i].T + P["w_self.%d.bias" % i] + (dense(b) @ h) @ P["w_neigh.%d.weight" % i].T
        if i == 0:
            h = torch.relu(h)
    pairs = batch.pairs.cpu().long()
    want = (h[pairs[:, 0]] * h[pairs[:, 1]]).sum(1)
    torch.nn.functional.binary_cross_entropy_with_logits(want, batch.labels().cpu().double()).backward()
    print("scores", rel(scores.detach().cpu(), want.detach()))
    assert rel(scores.detach().cpu(), want.detach()) < 1e-4
    for k, prm in model.named_parameters():
        print(k, rel(prm.grad.cpu(), P[k].grad))
        assert rel(prm.grad.cpu(), P[k].grad) < 1e-4, k


def test_example_trains():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "linkpred", "train.py"), "--nodes", "4000", "--epochs", "2",
                          "--batches", "15", "--batch", "256", "--eval-edges", "2000"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = [line for line in res.stdout.splitlines() if line.startswith("epoch")]
    losses = [float(line.split("loss")[1].split()[0]) for line in lines]
    aucs = [float(line.split("auc")[1].split()[0]) for line in lines]
    print(res.stdout)
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(0.0 <= a <= 1.0 for a in aucs), aucs
