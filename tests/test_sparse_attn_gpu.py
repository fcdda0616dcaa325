"""Sparse dot-product attention on the GPU: ops_attn.sparse_attention (forward and its three gradients) and nn.DotGatConv /
TransformerConv against the float64 restatement of attn_ref.py (`sparse_attention_reference`: per-edge tensors, autograd).  For bf16
the reference runs on the bf16-rounded inputs, so only accumulation order and the output rounding differ.

Bars (test_gat_strided_gpu.py): fp32 forward max |err| <= 1e-4 max|ref|, fp32 gradients <= 2e-3 max|ref|; bf16
forward <= 2e-2 max|ref|, bf16 gradients relative L2 <= 1.5e-2."""
import copy

import numpy as np
import pytest
import torch

from attn_ref import sparse_attention_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("out", "dq", "dk", "dv")


@pytest.fixture(scope="module")
def rmat():
    from dgll_amd import synth

    g = synth.rmat_graph(10, 10, symmetric=True, self_loops=True).to(DEV)
    assert g.n_rows == 1024 and int(g.degrees().max()) > 300
    return g


@pytest.fixture(scope="module")
def edge_graph():
    """70 x 90: rows 0 empty, 1 one entry, 2 exactly 64, 3 65, 4 one column five times, 5 LONG_ROW, 6 LONG_ROW + 1, 7 3000 entries
    (columns drawn with repetition), then short rows; the last row is empty and source 89 is never referenced."""
    from dgll_amd import CSRGraph, ops_attn

    rng = np.random.RandomState(5)
    rows = [[], [17], list(rng.permutation(89)[:64]), list(rng.permutation(89)[:65]), [33] * 5,
            list(rng.randint(0, 89, ops_attn.LONG_ROW)), list(rng.randint(0, 89, ops_attn.LONG_ROW + 1)), list(rng.randint(0, 89, 3000))]
    rows += [list(rng.randint(0, 89, rng.randint(1, 12))) for _ in range(61)] + [[]]
    assert len(rows) == 70 and all(c < 89 for r in rows for c in r)
    rowptr = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
    col = torch.tensor([int(c) for r in rows for c in r], dtype=torch.int32)
    return CSRGraph(rowptr, col, None, 70, 90).to(DEV)


def _inputs(graph, heads, D, dtype, seed=0, q_scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen)        # noqa: E731
    q = (rnd(graph.n_rows, heads * D) * q_scale).to(dtype).to(DEV)
    k = rnd(graph.n_cols, heads * D).to(dtype).to(DEV)
    v = rnd(graph.n_cols, heads * D).to(dtype).to(DEV)
    g = rnd(graph.n_rows, heads * D).to(dtype).to(DEV)
    return q, k, v, g


def _reference(graph, q, k, v, g, heads, scale):
    """(out, dq, dk, dv) in float64 as 2-D matrices, and the logits."""
    D = q.shape[1] // heads
    q64, k64, v64 = (t.detach().double().requires_grad_() for t in (q, k, v))
    out, s = sparse_attention_reference(graph.rowptr, graph.col, q64.view(-1, heads, D), k64.view(-1, heads, D), v64.view(-1, heads, D), scale)
    out = out.reshape(graph.n_rows, heads * D)
    grads = torch.autograd.grad(out, (q64, k64, v64), g.double())
    return (out.detach(),) + tuple(grads), s.detach()


def _device(graph, q, k, v, g, heads, scale=None):
    from dgll_amd import ops_attn

    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    out = ops_attn.sparse_attention(graph, q, k, v, heads, scale)
    assert out.dtype == q.dtype and out.shape == (graph.n_rows, q.shape[1])
    grads = torch.autograd.grad(out, (q, k, v), g)
    return (out.detach(),) + tuple(grads)


def _check(got, want, dtype, label=""):
    bad = []
    for name, a, b in zip(NAMES, got, want):
        a, b = a.double(), b.double()
        assert bool(torch.isfinite(a).all()), "%s %s: not finite" % (label, name)
        err_max = ((a - b).abs().max() / b.abs().max()).item()
        err_l2 = ((a - b).norm() / b.norm()).item()
        if dtype == torch.float32:
            bar, err = (1e-4 if name == "out" else 2e-3), err_max
        else:
            bar, err = (2e-2, err_max) if name == "out" else (1.5e-2, err_l2)
        print("%s %-5s max/max %.3e  rel-l2 %.3e  bar %.1e" % (label, name, err_max, err_l2, bar))
        if not err <= bar:
            bad.append((name, err, bar))
    assert not bad, "%s: %s" % (label, bad)


# the (heads, D, dtype) set of test_gatv2_gpu.CASES: idle lanes, idle heads, two column blocks, one head, 16 rows per wavefront
CASES = [(1, 8, torch.float32), (5, 8, torch.float32), (8, 8, torch.float32), (4, 64, torch.float32), (8, 128, torch.float32),
         (1, 48, torch.bfloat16), (3, 24, torch.bfloat16), (8, 32, torch.bfloat16), (8, 64, torch.bfloat16)]


@pytest.mark.parametrize("heads,D,dtype", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_forward_and_gradients_on_rmat(rmat, heads, D, dtype):
    q, k, v, g = _inputs(rmat, heads, D, dtype, seed=heads * 1000 + D)
    want, _ = _reference(rmat, q, k, v, g, heads, D ** -0.5)
    _check(_device(rmat, q, k, v, g, heads), want, dtype, "rmat %dx%d" % (heads, D))        # scale=None: D ** -0.5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_edge_case_rows(edge_graph, dtype):
    heads, D = 8, 32
    q, k, v, g = _inputs(edge_graph, heads, D, dtype, seed=11)
    want, _ = _reference(edge_graph, q, k, v, g, heads, D ** -0.5)
    got = _device(edge_graph, q, k, v, g, heads, D ** -0.5)
    _check(got, want, dtype, "edge rows")
    out, dk, dv = got[0], got[2], got[3]
    assert out[0].abs().max().item() == 0.0 and out[69].abs().max().item() == 0.0       # the empty rows
    assert dk[89].abs().max().item() == 0.0 and dv[89].abs().max().item() == 0.0        # the source no row references
    assert all(bool(torch.isfinite(t).all()) for t in got)


def test_large_logits(rmat):
    """max |s_ij| between 100 and 300: a softmax without max subtraction overflows fp32 (exp(89) is its largest finite value)."""
    heads, D = 4, 16
    q, k, v, g = _inputs(rmat, heads, D, torch.float32, seed=21)
    _, s = _reference(rmat, q, k, v, g, heads, D ** -0.5)
    q = q * (120.0 / s.abs().max().item())          # s is homogeneous of degree 1 in q
    want, s = _reference(rmat, q, k, v, g, heads, D ** -0.5)
    assert 100.0 <= s.abs().max().item() <= 300.0
    _check(_device(rmat, q, k, v, g, heads, D ** -0.5), want, torch.float32, "large logits")


def test_zero_queries_give_the_mean(rmat):
    """q = 0: every alpha_ij is 1 / deg(i) -- the mean aggregation of an existing kernel."""
    from dgll_amd import ops, ops_attn

    heads, D = 4, 16
    q, k, v, _ = _inputs(rmat, heads, D, torch.float32, seed=31)
    out = ops_attn.sparse_attention(rmat, torch.zeros_like(q), k, v, heads)
    unit = rmat.with_values(torch.ones(rmat.nnz, dtype=torch.float32, device=DEV))
    mean = ops.spmm(unit, v, reduce="mean")
    assert (out - mean).abs().max().item() <= 1e-5 * mean.abs().max().item()


def test_shared_key_and_value(rmat):
    """k is v: one gather per edge; the same output as separate clones, and the single input gradient is dk + dv."""
    from dgll_amd import ops_attn

    heads, D = 4, 16
    q, k, _, g = _inputs(rmat, heads, D, torch.float32, seed=51)
    out_u, dq_u, dk, dv = _device(rmat, q, k, k.clone(), g, heads)
    qs, ks = q.clone().requires_grad_(), k.clone().requires_grad_()
    out = ops_attn.sparse_attention(rmat, qs, ks, ks, heads)
    gq, gk = torch.autograd.grad(out, (qs, ks), g)
    want, _ = _reference(rmat, q, k, k, g, heads, D ** -0.5)
    both, both_ref = dk + dv, want[2] + want[3]
    assert (out - out_u).abs().max().item() <= 1e-4 * out_u.abs().max().item()
    assert (out.double() - want[0]).abs().max().item() <= 1e-4 * want[0].abs().max().item()
    assert (gk - both).abs().max().item() <= 2e-3 * both.abs().max().item()
    assert (gk.double() - both_ref).abs().max().item() <= 2e-3 * both_ref.abs().max().item()
    assert (gq - dq_u).abs().max().item() <= 2e-3 * dq_u.abs().max().item()


def test_gradients_are_skipped_where_not_needed(rmat):
    """Only q needs a gradient: the cols pass is skipped and dq is that of the full backward, bit for bit."""
    from dgll_amd import ops_attn

    heads, D = 8, 32
    q, k, v, g = _inputs(rmat, heads, D, torch.bfloat16, seed=61)
    full = _device(rmat, q, k, v, g, heads)
    qs = q.clone().requires_grad_()
    out = ops_attn.sparse_attention(rmat, qs, k, v, heads)
    (gq,) = torch.autograd.grad(out, (qs,), g)
    assert torch.equal(out.detach(), full[0]) and torch.equal(gq, full[1])


def test_reruns_are_bit_identical(rmat):
    heads, D = 8, 32
    q, k, v, g = _inputs(rmat, heads, D, torch.bfloat16, seed=41)
    a = _device(rmat, q, k, v, g, heads)
    b = _device(rmat, q, k, v, g, heads)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), name


def test_argument_checks_and_empty_graphs(rmat):
    from dgll_amd import CSRGraph, ops_attn

    x = torch.ones(1024, 16, device=DEV)
    with pytest.raises(ValueError, match="one dtype and width"):
        ops_attn.sparse_attention(rmat, x, x[:, :8], x, 2)
    with pytest.raises(ValueError, match="one dtype and width"):
        ops_attn.sparse_attention(rmat, x, x.bfloat16(), x, 2)
    with pytest.raises(ValueError, match="sources"):
        ops_attn.sparse_attention(rmat, x, x[:1000], x[:1000], 2)
    with pytest.raises(ValueError, match="divide"):
        ops_attn.sparse_attention(rmat, x, x, x, 3)
    with pytest.raises(ValueError, match="16-byte vectors"):
        ops_attn.sparse_attention(rmat, x, x, x, 8)                 # D = 2
    with pytest.raises(ValueError, match="16-byte vectors"):
        ops_attn.sparse_attention(rmat, x.bfloat16(), x.bfloat16(), x.bfloat16(), 4)       # D = 4 bf16 columns
    wide = torch.ones(1024, 260, device=DEV)
    with pytest.raises(ValueError, match="at most"):
        ops_attn.sparse_attention(rmat, wide, wide, wide, 1)        # 65 vectors: a head no longer fits a wavefront
    with pytest.raises(TypeError):
        ops_attn.sparse_attention(rmat, x.double(), x.double(), x.double(), 2)
    # nothing to gather: zeros, with zero gradients
    empty = CSRGraph(torch.zeros(6, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None, 5, 7).to(DEV)
    q, k = torch.randn(5, 16, device=DEV, requires_grad=True), torch.randn(7, 16, device=DEV, requires_grad=True)
    out = ops_attn.sparse_attention(empty, q, k, k, 2)
    assert out.shape == (5, 16) and out.abs().max().item() == 0.0
    gq, gk = torch.autograd.grad(out.sum(), (q, k))
    assert gq.abs().max().item() == 0.0 and gk.abs().max().item() == 0.0
    none = CSRGraph(torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None, 0, 7).to(DEV)
    assert ops_attn.sparse_attention(none, q[:0], k, k, 2).shape == (0, 16)


def _layer_against_host(layer, graph, feat_dev, out_shape):
    """Forward and every gradient of the device layer against a float64 copy on the host path, at the fp32 bars."""
    host = copy.deepcopy(layer).double().cpu()
    layer = layer.to(DEV)
    pair = isinstance(feat_dev, tuple)
    leaf = (feat_dev[0] if pair else feat_dev).detach().clone().requires_grad_()
    leaf_h = leaf.detach().double().cpu().requires_grad_()
    n_dst = graph.n_rows
    out = layer(graph, (leaf, leaf[:n_dst]) if pair else leaf)
    out_h = host(graph.to("cpu"), (leaf_h, leaf_h[:n_dst]) if pair else leaf_h)
    assert out.shape == out_h.shape == out_shape
    err = (out.detach().double().cpu() - out_h.detach()).abs().max().item() / out_h.abs().max().item()
    print("layer %-18s %.3e" % ("out", err))
    assert err <= 1e-4
    gen = torch.Generator().manual_seed(7)
    g = torch.randn(out.shape, generator=gen)
    names = ["input"] + [n for n, _ in layer.named_parameters()]
    got = torch.autograd.grad(out, [leaf] + list(layer.parameters()), g.to(DEV))
    want = torch.autograd.grad(out_h, [leaf_h] + list(host.parameters()), g.double())
    ref = dict(zip(names, want))
    for name, a, b in zip(names, got, want):
        scale = b.abs().max().item()
        if name == "lin_key.bias":
            # Its true gradient is identically 0: a constant added to every key moves all logits of a row alike and the softmax
            # does not see it.  The float64 reference holds only its own rounding noise (asserted), which is no scale to measure
            # against.  The gradient is the column sums of dk -- the sums that form lin_key.weight's gradient, with ones for the
            # input -- so it is held to that gradient's bar.
            scale = ref["lin_key.weight"].abs().max().item()
            assert b.abs().max().item() <= 1e-12 * scale
        err = (a.double().cpu() - b).abs().max().item() / scale
        print("layer %-18s %.3e" % (name, err))
        assert err <= 2e-3, name


def _layers():
    from dgll_amd.nn.Convolution import DotGatConv, TransformerConv

    return {"dotgat": (lambda fin: DotGatConv(fin, 6, 3), lambda n: (n, 3, 6)),             # heads of 6 columns: padded to 8
            "transformer": (lambda fin: TransformerConv(fin, 6, heads=3, beta=True), lambda n: (n, 18))}


@pytest.mark.parametrize("kind", ["dotgat", "transformer"])
def test_layer_matches_its_host_path(rmat, kind):
    make, shape = _layers()[kind]
    torch.manual_seed(61)
    _layer_against_host(make(20), rmat, torch.randn(1024, 20).to(DEV), shape(1024))


@pytest.mark.parametrize("kind", ["dotgat", "transformer"])
def test_layer_on_a_sampled_block(rmat, kind):
    from dgll_amd.sampling.neighbor import NeighborSampler

    make, shape = _layers()[kind]
    torch.manual_seed(71)
    sampler = NeighborSampler([6], rmat)
    input_nodes, _, blocks = sampler.sample_seeded(None, torch.arange(0, 200, device=DEV), 71)
    block = blocks[0]
    assert block.n_rows == 200 and block.n_cols > block.n_rows
    h_src = torch.randn(1024, 20)[input_nodes.cpu()].to(DEV)
    layer = make(20)
    _layer_against_host(layer, block, (h_src, h_src[:200]), shape(200))
    # one tensor on a block: its first rows are the destinations -- the same output as the pair
    with torch.no_grad():
        layer = layer.to(DEV)
        single, both = layer(block, h_src), layer(block, (h_src, h_src[:200]))
    assert single.shape == both.shape and (single - both).abs().max().item() <= 1e-4 * both.abs().max().item()


def test_forward_backward_can_be_captured(rmat):
    from dgll_amd import ops_attn

    heads, D = 8, 32
    q, k, v, g = _inputs(rmat, heads, D, torch.bfloat16, seed=81)
    q, k, v = (t.requires_grad_() for t in (q, k, v))

    def step():
        out = ops_attn.sparse_attention(rmat, q, k, v, heads)
        return (out.detach(),) + tuple(torch.autograd.grad(out, (q, k, v), g))

    eager = [t.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static = step()
    for _ in range(2):
        for t in static:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(NAMES, static, eager):
            assert torch.equal(a, b), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_training_on_planted_communities(dtype):
    """40 Adam steps of the two-layer TransformerConv model; on the host path in fp32 this seed and learning rate take the loss from
    1.25 to below 1e-3 at accuracy 1.0."""
    from dgll_amd import synth
    from dgll_amd.nn.Convolution import GraphTransformer

    n, k = 400, 4
    gen = torch.Generator().manual_seed(3)
    labels = torch.arange(n) % k
    prob = torch.where(labels[:, None] == labels[None, :], torch.tensor(0.05), torch.tensor(0.005))
    src, dst = (torch.rand(n, n, generator=gen) < prob).nonzero(as_tuple=True)
    graph = synth.build_graph(src, dst, n, symmetric=True, self_loops=True, weighted=False).to(DEV)
    x = (torch.nn.functional.one_hot(labels, k).float().repeat(1, 4) + torch.randn(n, 4 * k, generator=gen)).to(dtype).to(DEV)
    labels = labels.to(DEV)
    torch.manual_seed(3)
    model = GraphTransformer(4 * k, 8, k, 4).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=0.02)
    losses = []
    for _ in range(40):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(graph, x).float(), labels)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    acc = (model(graph, x).argmax(1) == labels).float().mean().item()
    print("loss %.4f -> %.4f, accuracy %.3f" % (losses[0], losses[-1], acc))
    assert losses[-1] < 0.5 * losses[0] and acc >= 0.9
