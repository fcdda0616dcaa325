"""The Gaussian-mixture op on the GPU: dgll_amd.ops_gmm.gmm_expand through autograd (Z and all four gradients, sum and mean) against
the float64 entry-by-entry restatement of gmm_ref.py on the cases, graphs and pinned seeds of test_gmm_emulated.py; the
hard-assignment limit, where everything must be EXACT; the transposed pass reading each duplicate entry's own pseudo row; the passes
that run for each of the 16 sets of wanted gradients, and reruns; more entries than slabs; the peak memory of a forward and backward;
nn.GMMConv against its own host path, nn.MoNet training, and a captured forward and backward.  For bf16 the reference runs on the
bf16-rounded x and gradient.

Bars, each against max |ref| of its tensor: fp32 forward max |err| <= 1e-4, fp32 gradients <= 2e-3; bf16 forward
<= 2e-2, bf16 gradients relative L2 <= 1.5e-2.  grad_mu and grad_inv_sigma are sums over all entries: the float64 reference of every
case must have max(sum_e |term|) / max |sum_e term| <= 50 for the pinned seed (asserted: a precondition on the seed, not a skip)."""
import functools
import itertools

import pytest
import torch

import gmm_ref
from test_edge_feat_gpu import FIVE, FIVE_COL, _check, _ids, _kinds
from test_gmm_emulated import CASES, SEEDS, graph_of, well_conditioned
from test_pna_emulated import _graph

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("grad_x", "grad_pseudo", "grad_mu", "grad_inv_sigma")


@functools.lru_cache(maxsize=None)
def _case(F, K, dim, dtype):
    """the graph, the inputs and, per reduction, the float64 reference (Z, grad_x, grad_pseudo, grad_mu, grad_inv_sigma): computed once"""
    cpu = graph_of(F)
    ins = gmm_ref.inputs(cpu, F, K, dim, dtype, SEEDS[(F, K, dim)])
    x, pseudo, mu, sigma, g = ins
    want = {}
    for reduce in ("sum", "mean"):
        grads = gmm_ref.gradients(cpu.rowptr, cpu.col, x, pseudo, mu, sigma, g, reduce)
        well_conditioned(grads[4], "%s %s" % ((F, K, dim), reduce))
        want[reduce] = (gmm_ref.expand(cpu.rowptr, cpu.col, x, pseudo, mu, sigma, reduce),) + grads[:4]
    return cpu, ins, want


def _run(graph, ins, reduce, needs=(True,) * 4):
    from dgll_amd import ops_gmm

    x, pseudo, mu, sigma, g = ins
    leaves = [t.to(DEV).requires_grad_(n) for t, n in zip((x, pseudo, mu, sigma), needs)]
    z = ops_gmm.gmm_expand(graph, *leaves, reduce=reduce)
    if z.requires_grad:                                         # (no gradient wanted: there is no backward)
        z.backward(g.to(DEV))
    return z.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("F,K,dim,dtype", CASES, ids=_ids)
def test_op_against_the_reference(F, K, dim, dtype):
    cpu, ins, want = _case(F, K, dim, dtype)
    graph = cpu.to(DEV)
    fwd, grad = _kinds(dtype)
    for reduce, ref in want.items():
        z, grads = _run(graph, ins, reduce)
        assert z.dtype == dtype and tuple(z.shape) == (cpu.n_rows, K * F)
        assert grads[0].dtype == dtype and all(t.dtype == torch.float32 for t in grads[1:])
        assert tuple(grads[1].shape) == (cpu.nnz, dim) and tuple(grads[2].shape) == (K, dim) and tuple(grads[3].shape) == (K, dim)
        for key, got, w in zip(("Z",) + NAMES, [z] + grads, ref):
            _check("%s %s" % (reduce, key), got, w, fwd if key == "Z" else grad)
        # rows without entries give zeros; the source no row references gets no gradient
        assert z[0].abs().max().item() == 0.0 and z[-1].abs().max().item() == 0.0 and grads[0][-1].abs().max().item() == 0.0


def test_pseudo_of_another_dtype_gets_its_gradient_in_that_dtype():
    cpu, (x, pseudo, mu, sigma, g), want = _case(24, 3, 3, torch.float32)
    z, grads = _run(cpu.to(DEV), (x, pseudo.double(), mu.double(), sigma, g), "sum")
    assert grads[1].dtype == torch.float64 and grads[2].dtype == torch.float64 and grads[3].dtype == torch.float32
    for key, got, w in zip(("Z",) + NAMES, [z] + grads, want["sum"]):
        _check(key, got, w, "fwd32" if key == "Z" else "grad32")


@pytest.mark.parametrize("K", [3, 9])
@pytest.mark.parametrize("F,dtype", [(8, torch.float32), (8, torch.bfloat16), (260, torch.float32)], ids=_ids)
def test_hard_assignment_limit_is_exact(F, dtype, K):
    """pseudo on integer grid points, mu on K distinct grid points, inv_sigma = 32, every entry on one kernel's mu: the on-kernel
    weight is exp2(-0) = 1 and the off-kernel exponent is at most -0.5 * 32^2 * log2(e) = -738 in base 2, so the fp32 weight is exactly
    0.  With dyadic x and gradient every sum is exact in fp32: Z and grad_x EQUAL the float64 one-hot aggregation (rounded once to the
    storage dtype) and the three other gradients are exactly 0."""
    cpu = graph_of(F)
    gen = torch.Generator().manual_seed(7)
    grid = torch.tensor([[k % 3, k // 3] for k in range(K)], dtype=torch.float32)
    owner = torch.randint(0, K, (cpu.nnz,), generator=gen)
    pseudo, mu, sigma = grid[owner], grid.clone(), torch.full((K, 2), 32.0)
    x = (torch.randint(-8, 9, (cpu.n_cols, F), generator=gen).float() / 8).to(dtype)
    g = (torch.randint(-8, 9, (cpu.n_rows, K * F), generator=gen).float() / 8).to(dtype)
    w64 = gmm_ref.weights(pseudo, mu, sigma)
    hot = torch.nn.functional.one_hot(owner, K).bool()
    assert bool((w64[hot] == 1.0).all()) and w64[~hot].max().item() < 2.0 ** -200        # the precondition of the limit
    row = gmm_ref.row_index(cpu.rowptr)
    want_z = torch.zeros(cpu.n_rows, K, F, dtype=torch.float64).index_put_((row, owner), x.double()[cpu.col.long()], accumulate=True)
    want_gx = torch.zeros(cpu.n_cols, F, dtype=torch.float64).index_add_(0, cpu.col.long(), g.double().view(-1, K, F)[row, owner])
    z, grads = _run(cpu.to(DEV), (x, pseudo, mu, sigma, g), "sum")
    assert torch.equal(z.double().cpu(), want_z.reshape(cpu.n_rows, K * F).to(dtype).double())
    assert torch.equal(grads[0].double().cpu(), want_gx.to(dtype).double())
    for name, t in zip(NAMES[1:], grads[1:]):
        assert t.abs().max().item() == 0.0, name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_the_transposed_pass_reads_each_duplicates_own_pseudo_row(dtype):
    """With the output gradient on the five-times row alone and one kernel, grad_x of its column is that gradient times the sum of the
    five weights: five DIFFERENT rows of pseudo, read through perm."""
    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    _, perm = graph.transpose()
    assert not torch.equal(perm.cpu(), torch.arange(cpu.nnz))
    F, K, dim = 8, 1, 2
    x, pseudo, mu, sigma, g = gmm_ref.inputs(cpu, F, K, dim, dtype, 21)
    lo = int(cpu.rowptr[FIVE])
    assert cpu.col[lo:lo + 5].tolist() == [FIVE_COL] * 5 and int(cpu.rowptr[FIVE + 1]) == lo + 5
    w5 = gmm_ref.weights(pseudo[lo:lo + 5], mu, sigma)[:, 0]
    assert len({tuple(r) for r in pseudo[lo:lo + 5].tolist()}) == 5 and len(set(w5.tolist())) == 5
    only = torch.zeros_like(g)
    only[FIVE] = g[FIVE]
    _, grads = _run(graph, (x, pseudo, mu, sigma, only), "sum", (True, False, False, False))
    want = torch.zeros(cpu.n_cols, F, dtype=torch.float64)
    want[FIVE_COL] = g[FIVE].double() * w5.sum()
    _check("grad_x", grads[0], want, _kinds(dtype)[1])
    rest = torch.ones(cpu.n_cols, dtype=torch.bool)
    rest[FIVE_COL] = False
    assert grads[0].cpu()[rest].abs().max().item() == 0.0


def test_only_the_wanted_gradients_are_computed_and_reruns_give_the_same_bits():
    from dgll_amd import ops

    cpu, ins, _ = _case(24, 3, 3, torch.float32)
    graph = cpu.to(DEV)
    full = _run(graph, ins, "mean")
    again = _run(graph, ins, "mean")
    assert torch.equal(full[0], again[0]) and all(torch.equal(p, q) for p, q in zip(full[1], again[1]))      # no atomics
    for needs in itertools.product((True, False), repeat=4):                        # (x, pseudo, mu, inv_sigma)
        with ops.LaunchTimer() as timer:
            z, grads = _run(graph, ins, "mean", needs)
        tags = [tag[0] for tag, _, _ in timer.records]
        param = 1 if any(needs[1:]) else 0
        assert tags.count("gmm_expand") == 1
        assert tags.count("gmm_contract") == (1 if needs[0] else 0), (needs, tags)
        assert tags.count("typed_dots") == param and tags.count("gmm_param") == param, (needs, tags)
        assert torch.equal(z, full[0])
        for need, got, ref in zip(needs, grads, full[1]):
            assert (got is None) == (not need)
            if need:
                assert torch.equal(got, ref), needs


def test_empty_graphs_give_zeros_with_zero_gradients():
    from dgll_amd import CSRGraph, ops_gmm

    for n_dst, reduce in ((3, "sum"), (3, "mean"), (0, "sum")):
        g = CSRGraph(torch.zeros(n_dst + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None, n_dst, 5).to(DEV)
        x, ps, mu, sg = (torch.randn(*s, device=DEV, requires_grad=True) for s in ((5, 8), (0, 2), (3, 2), (3, 2)))
        z = ops_gmm.gmm_expand(g, x, ps, mu, sg, reduce)
        assert tuple(z.shape) == (n_dst, 24) and (n_dst == 0 or z.abs().max().item() == 0.0)
        z.sum().backward()
        assert all(t.grad.shape == t.shape and (t.numel() == 0 or t.grad.abs().max().item() == 0.0) for t in (x, ps, mu, sg))


def test_more_entries_than_slabs():
    """param_raw with one slab (a single workgroup strides over every entry), two, and the default agree with the reference, and every
    element of every slab is written: the slabs start as NaN."""
    from dgll_amd import ops_gmm

    cpu, (x, pseudo, mu, sigma, g), want = _case(24, 9, 2, torch.float32)
    K, dim = 9, 2
    p = torch.zeros(cpu.nnz, 12)
    p[:, :K] = gmm_ref.edge_dots(cpu.rowptr, cpu.col, x, g, K).float()
    p, ps, m, s = (t.to(DEV) for t in (p, pseudo, mu, sigma))
    default = max(1, -(-cpu.nnz // 256))
    assert default > 2
    for partials in (1, 2, default, default + 3):               # (the last: workgroups past the entries write zero slabs)
        slabs = torch.full((partials, 2, K, dim), float("nan"), device=DEV)
        gm, gs, gp = ops_gmm.param_raw(p, ps, m, s, want_pseudo=True, partials=partials, slabs=slabs)
        assert bool(torch.isfinite(slabs).all())
        for key, got, w in zip(NAMES[1:], (gp, gm, gs), want["sum"][2:]):
            _check("partials %d %s" % (partials, key), got, w, "grad32")
    gm, gs, gp = ops_gmm.param_raw(p, ps, m, s)
    assert gp is None
    _check("default grad_mu", gm, want["sum"][3], "grad32")


def test_nothing_of_the_size_of_nnz_by_f_is_allocated():
    """256 nodes of degree 256 (nnz = 2^16), F = 64 fp32, K = 3, dim = 2: one [nnz, F] array is 16 MiB, and DGL's message tensor
    [nnz, K, out] three of them.  The peak of a forward and backward above what is allocated before them (all four gradients wanted)
    stays under a QUARTER of one [nnz, F] array: by construction 16 B (P) + 8 B (grad_pseudo) per entry of 256 B, plus node-sized
    arrays.  A condition, not a measurement; the figure is printed."""
    from dgll_amd import CSRGraph, ops_gmm

    n, deg, F, K, dim = 256, 256, 64, 3, 2
    gen = torch.Generator().manual_seed(5)
    col = torch.randint(0, n, (n * deg,), generator=gen).to(torch.int32)
    graph = CSRGraph(torch.arange(n + 1, dtype=torch.int64) * deg, col, None, n, n).to(DEV)
    nnz = graph.nnz
    assert nnz == 2 ** 16
    graph.transpose()
    ins = [t.to(DEV) for t in (torch.randn(n, F, generator=gen), torch.rand(nnz, dim, generator=gen) * 2 - 1,
                               0.5 * torch.randn(K, dim, generator=gen), 0.5 + 1.5 * torch.rand(K, dim, generator=gen))]
    go = torch.randn(n, K * F, generator=gen).to(DEV)
    one = nnz * F * 4

    def peak():
        leaves = [t.clone().requires_grad_() for t in ins]
        ops_gmm.gmm_expand(graph, *leaves).backward(go)                             # once outside the measurement: lazy initialisation
        for t in leaves:
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        ops_gmm.gmm_expand(graph, *leaves).backward(go)
        torch.cuda.synchronize()
        assert all(t.grad is not None for t in leaves)
        return torch.cuda.max_memory_allocated() - before

    used = peak()
    print("peak above the inputs: %d bytes (%.2f MiB); one [nnz, F] array %d bytes" % (used, used / 2 ** 20, one))
    assert used < one // 4, (used, one)


# ---- the layers ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("in_feats,residual", [(5, True), (6, True), ((5, 4), True), (8, False)], ids=_ids)
def test_gmmconv_against_its_own_host_path(in_feats, residual, reduce):
    """fp32, a sampler block (24 destinations of 30 sources): widths that need padding, the one-launch residual, the identity residual,
    a pair of widths, no residual; outputs, parameter gradients and the gradients of the features and of pseudo."""
    import copy

    from dgll_amd.nn import GMMConv

    torch.manual_seed(11)
    cpu = _graph(full=True)
    K, dim, out = 3, 2, 6
    host = GMMConv(in_feats, out, dim, K, aggregator_type=reduce, residual=residual, allow_zero_in_degree=True)
    with torch.no_grad():
        host.mu.copy_(0.5 * torch.randn(K, dim))
        host.inv_sigma.copy_(0.5 + 1.5 * torch.rand(K, dim))
        host.bias.copy_(torch.randn(out))
    dev = copy.deepcopy(host).to(DEV)
    pair = isinstance(in_feats, tuple)
    fs, fd = in_feats if pair else (in_feats, in_feats)
    feats = [torch.randn(cpu.n_cols, fs)] + ([torch.randn(cpu.n_rows, fd)] if pair else [])
    pseudo = torch.rand(cpu.nnz, dim) * 2 - 1
    go = torch.randn(cpu.n_rows, out)

    def run(layer, graph, where):
        leaves = [t.to(where).requires_grad_() for t in feats + [pseudo]]
        h = layer(graph, tuple(leaves[:-1]) if pair else leaves[0], leaves[-1])
        return h, torch.autograd.grad(h, leaves + list(layer.parameters()), go.to(where))

    want, want_grads = run(host, cpu, "cpu")
    got, got_grads = run(dev, cpu.to(DEV), DEV)
    assert got.is_cuda and got.dtype == torch.float32
    _check("out", got, want, "fwd32")
    names = ["feat"] * len(feats) + ["pseudo"] + [n for n, _ in host.named_parameters()]
    for name, p, q in zip(names, got_grads, want_grads):
        _check("grad " + name, p, q, "grad32")


def test_monet_trains():
    from dgll_amd import CSRGraph
    from dgll_amd.nn import MoNet

    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(3)
    n, deg, classes = 512, 8, 4
    labels = torch.randint(0, classes, (n,), generator=gen)
    col = torch.randint(0, n, (n * deg,), generator=gen).to(torch.int32)
    graph = CSRGraph(torch.arange(n + 1, dtype=torch.int64) * deg, col, None, n, n).to(DEV)
    x = (1.0 + 0.5 * torch.randn(n, 12, generator=gen)).to(DEV)
    y = labels.to(DEV)
    model = MoNet(12, 16, classes, dim=2, n_kernels=3, n_layers=2, aggregator_type="mean", residual=True).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=5e-3)
    losses = []
    for _ in range(10):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(graph, x), y)               # degree_pseudo by default
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print(losses)
    assert all(v == v and abs(v) != float("inf") for v in losses) and losses[-1] < losses[0], losses
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_forward_backward_can_be_captured(reduce):
    """One forward and backward of the op (all four gradients: EXPAND, CONTRACT, the dots pass and PARAM) captured into a graph replays
    to the bits of the eager run -- the shape of the capture tests of the other fused ops."""
    from dgll_amd import ops_gmm

    cpu, (x, pseudo, mu, sigma, g), _ = _case(24, 3, 3, torch.float32)
    graph = cpu.to(DEV)
    graph.transpose()                                                               # the cached structure, built outside the capture
    leaves = [t.to(DEV).requires_grad_() for t in (x, pseudo, mu, sigma)]
    go = g.to(DEV)

    def step():
        z = ops_gmm.gmm_expand(graph, *leaves, reduce=reduce)
        return (z.detach(),) + tuple(torch.autograd.grad(z, leaves, go))

    eager = [t.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured, stream=side):
        static = step()
    for _ in range(2):
        for t in static:
            t.zero_()
        captured.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("Z",) + NAMES, static, eager):
            assert torch.equal(a, b), name
