"""PNA on the GPU: dgll_amd.ops_agg.multi_aggregate (forward and both gradients) and nn.PNAConv against the float64 per-edge
restatements of pna_ref.py (explicit messages, torch segment ops, autograd; no decomposition).  For bf16 the reference runs on the
bf16-rounded inputs, so only accumulation order and the output rounding differ.

Bars (as test_mp_gpu.py states them): fp32 forward max |err| <= 1e-4 max |ref|, fp32 gradients <= 2e-3 max |ref|;
bf16 forward <= 2e-2 max |ref|, bf16 gradients relative L2 <= 1.5e-2 -- applied PER aggregator x scaler block against that block's own
max |ref| (a wrong std must not hide behind a large sum): the backward is linear in the output gradient, so it runs once per block
with the other blocks' gradient zeroed.

Inputs of every std / var gradient check keep distinct values apart (pna_ref.spread_features): the smallest non-zero row variance is at
least (2 / n_src)^2 in float64, which the tests assert; cast to bf16 the same generator produces genuine ties, which exercise the tie
rule and the exact-zero branch of the variance's gradient."""
import numpy as np
import pytest
import torch

import pna_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
DEFAULT_AGGS, DEFAULT_SCALERS = ("mean", "max", "min", "std"), ("identity", "amplification", "attenuation")
ONE, FIVE = 1, 4        # rows of the edge-case graph: one entry; one column five times


@pytest.fixture(scope="module")
def rmat():
    from dgll_amd import synth

    g = synth.rmat_graph(10, 10, symmetric=True, self_loops=True).to(DEV)
    assert g.n_rows == 1024 and int(g.degrees().max()) > 300
    return g


@pytest.fixture(scope="module")
def edge_graph():
    """The 70 x 90 graph of test_mp_gpu.py, rebuilt: rows 0 empty, 1 one entry, 2 exactly 64, 3 65, 4 one column five times, 5 LONG_ROW,
    6 LONG_ROW + 1, 7 3000 entries (columns drawn with repetition), then short rows; the last row is empty and source 89 is never
    referenced."""
    from dgll_amd import CSRGraph, ops_agg

    rng = np.random.RandomState(5)
    rows = [[], [17], list(rng.permutation(89)[:64]), list(rng.permutation(89)[:65]), [33] * 5,
            list(rng.randint(0, 89, ops_agg.LONG_ROW)), list(rng.randint(0, 89, ops_agg.LONG_ROW + 1)), list(rng.randint(0, 89, 3000))]
    rows += [list(rng.randint(0, 89, rng.randint(1, 12))) for _ in range(61)] + [[]]
    assert len(rows) == 70 and all(c < 89 for r in rows for c in r)
    rowptr = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
    col = torch.tensor([int(c) for r in rows for c in r], dtype=torch.int32)
    return CSRGraph(rowptr, col, None, 70, 90).to(DEV)


def _check(label, name, got, want, kind):
    """kind: 'fwd32' / 'grad32' max |err| over max |ref| at 1e-4 / 2e-3; 'fwd16' the same at 2e-2; 'grad16' relative L2 at 1.5e-2.  A
    reference that is zero but for its own float64 rounding residue (the gradient of var / std with respect to y: below 1e-10 with inputs
    and gradients of order 1) must be met with exact zeros."""
    a, b = got.detach().double().cpu(), want.detach().double().cpu()
    assert a.shape == b.shape, (label, name, a.shape, b.shape)
    assert bool(torch.isfinite(a).all()), "%s %s: not finite" % (label, name)
    if b.abs().max().item() < 1e-10:
        assert a.abs().max().item() == 0.0, (label, name)
        return
    err_max = ((a - b).abs().max() / b.abs().max()).item()
    err_l2 = ((a - b).norm() / b.norm()).item()
    bar, err = {"fwd32": (1e-4, err_max), "grad32": (2e-3, err_max), "fwd16": (2e-2, err_max), "grad16": (1.5e-2, err_l2)}[kind]
    print("%s %-12s max/max %.3e  rel-l2 %.3e  bar %.1e" % (label, name, err_max, err_l2, bar))
    assert err <= bar, (label, name, err, bar)


def _kinds(dtype):
    return ("fwd32", "grad32") if dtype == torch.float32 else ("fwd16", "grad16")


def _inputs(graph, F, dtype, n_blocks, seed):
    """(x64 before rounding, x, y, grad_out) on the CPU"""
    gen = torch.Generator().manual_seed(seed)
    x64 = pna_ref.spread_features(graph.n_cols, F, seed)
    y = torch.randn(graph.n_rows, F, generator=gen).to(dtype)
    go = torch.randn(graph.n_rows, n_blocks * F, generator=gen).to(dtype)
    return x64, x64.to(dtype), y, go


def _against_reference(graph, F, dtype, aggs, scalers, delta, with_y, label, seed):
    """multi_aggregate, forward and every gradient, per block against pna_ref; returns what the exactness checks look at."""
    from dgll_amd import ops_agg

    fwd, grad = _kinds(dtype)
    n_blocks = len(aggs) * len(scalers)
    x64, x, y, go = _inputs(graph, F, dtype, n_blocks, seed)
    rp, col = graph.rowptr.cpu(), graph.col.cpu()
    floor = (2.0 / graph.n_cols) ** 2
    parts = {}
    pna_ref.multi_aggregate_reference(rp, col, x64, None, ("var",), ("identity",), 1.0, parts)
    assert parts["var"][parts["var"] > 0].min().item() >= floor        # distinct values stay apart (float64, before rounding)
    xr = x.double().requires_grad_()
    yr = y.double().requires_grad_() if with_y else None
    parts = {}
    want = pna_ref.multi_aggregate_reference(rp, col, xr, yr, aggs, scalers, delta, parts)
    if dtype == torch.float32:
        assert parts["var"][parts["var"] > 0].min().item() >= floor * (1 - 1e-5)

    xg = x.to(DEV).requires_grad_()
    yg = y.to(DEV).requires_grad_() if with_y else None
    gg = go.to(DEV)
    out = ops_agg.multi_aggregate(graph, xg, yg, aggs, scalers, delta)
    assert out.dtype == dtype and tuple(out.shape) == (graph.n_rows, n_blocks * F)
    leaves_g, leaves_r = ((xg, yg), (xr, yr)) if with_y else ((xg,), (xr,))
    for k in range(n_blocks):
        name = "%s*%s" % (scalers[k // len(aggs)][:3], aggs[k % len(aggs)])
        sl = slice(k * F, (k + 1) * F)
        _check(label, name, out[:, sl], want[:, sl], fwd)
        mask_g = torch.zeros_like(gg)
        mask_g[:, sl] = gg[:, sl]
        mask_r = torch.zeros_like(want)
        mask_r[:, sl] = go.double()[:, sl]
        got = torch.autograd.grad(out, leaves_g, mask_g, retain_graph=True)
        ref = torch.autograd.grad(want, leaves_r, mask_r, retain_graph=True)
        for what, a, b in zip(("gx", "gy"), got, ref):
            _check(label, what + " " + name, a, b, grad)
    got = torch.autograd.grad(out, leaves_g, gg)
    ref = torch.autograd.grad(want, leaves_r, go.double())
    for what, a, b in zip(("gx", "gy"), got, ref):
        _check(label, what, a, b, grad)
    return out.detach().cpu(), want.detach(), [t.cpu() for t in got], parts, x


@pytest.mark.parametrize("F,dtype", [(8, torch.float32), (20, torch.float32), (64, torch.float32), (256, torch.float32), (320, torch.float32),
                                     (8, torch.bfloat16), (24, torch.bfloat16), (64, torch.bfloat16), (512, torch.bfloat16),
                                     (520, torch.bfloat16),
                                     (72, torch.float32), (128, torch.float32),                             # 32 lanes a row: idle lanes, full
                                     (72, torch.bfloat16), (136, torch.bfloat16), (256, torch.bfloat16)],   # 16 lanes; 32: idle lanes, full
                         ids=lambda v: str(v).replace("torch.", ""))
def test_default_aggregators_on_rmat(rmat, F, dtype):
    """idle lanes, a vector count that is no power of two, one full row of lanes, exactly one and more than one column block; every
    lane width (8, 16, 32, 64 lanes a row) in both dtypes"""
    _against_reference(rmat, F, dtype, DEFAULT_AGGS, DEFAULT_SCALERS, 1.3, True, "rmat F=%d" % F, 100 + F)


def _raw(graph, x, aggs, scalers, delta):
    """forward_raw with stats and arg on the CPU"""
    from dgll_amd import ops_agg

    out, stats, arg = ops_agg.forward_raw(graph, x.to(DEV), None, tuple(ops_agg.AGGREGATORS[a] for a in aggs),
                                          tuple(ops_agg.SCALERS[s] for s in scalers), delta, want_stats=True, want_arg=True)
    return out.cpu(), stats.cpu(), arg.cpu()


@pytest.mark.parametrize("with_y", [False, True], ids=["noy", "y"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_all_aggregators_on_edge_case_rows(edge_graph, dtype, with_y):
    from dgll_amd import ops_agg

    F, aggs, scalers, delta = 32, pna_ref.AGGREGATORS, pna_ref.SCALERS, 1.7
    out, want, grads, parts, x = _against_reference(edge_graph, F, dtype, aggs, scalers, delta, with_y, "edge", 7)
    block = lambda t, a: t[:, aggs.index(a) * F:(aggs.index(a) + 1) * F]       # noqa: E731  (under the identity scaler)
    # rows of equal entries: var exactly 0 and std exactly sqrt(1e-30); the empty rows: zeros in every block; the unreferenced source
    tiny = torch.sqrt(torch.tensor(1e-30, dtype=torch.float32)).to(dtype)
    for r in (ONE, FIVE):
        assert block(out, "var")[r].abs().max().item() == 0.0 and torch.equal(block(out, "std")[r], tiny.expand(F))
    for r in (0, 69):
        assert out[r].abs().max().item() == 0.0
        if with_y:
            assert grads[1][r].abs().max().item() == 0.0
    assert grads[0][89].abs().max().item() == 0.0
    if with_y:
        return
    # without y: the max / min blocks are entries of x bit for bit, and arg is the reference's (ties, which bf16 has, included)
    raw_out, stats, arg = _raw(edge_graph, x, aggs, scalers, delta)
    assert torch.equal(raw_out, out)
    assert torch.equal(block(out, "max"), block(want, "max").to(dtype)) and torch.equal(block(out, "min"), block(want, "min").to(dtype))
    assert torch.equal(arg.long(), torch.cat([parts["argmax"], parts["argmin"]], 1))
    assert stats[ONE, F:].abs().max().item() == 0.0 and stats[FIVE, F:].abs().max().item() == 0.0
    assert bool((arg[0] == -1).all()) and bool((arg[69] == -1).all()) and stats[0].abs().max().item() == 0.0
    # the exact zero of the variance's gradient: the coefficient rows of the rows of equal entries
    codes = (tuple(ops_agg.AGGREGATORS[a] for a in aggs), tuple(ops_agg.SCALERS[s] for s in scalers))
    go = torch.randn(70, len(aggs) * len(scalers) * F, device=DEV).to(dtype)
    coef, _ = ops_agg.rows_raw(edge_graph, go, stats.to(DEV), codes[0], codes[1], delta, want_grad_y=False)
    assert coef[ONE, F:2 * F].abs().max().item() == 0.0 and coef[FIVE, F:2 * F].abs().max().item() == 0.0
    assert coef[0].abs().max().item() == 0.0


def test_ordered_subset(rmat, monkeypatch):
    """aggregators=("std", "min"), scalers=("attenuation",): the block order is the caller's, and FORWARD allocates the side arrays only
    where a gradient of x is needed and the subset uses them."""
    from dgll_amd import ops_agg

    out, want, _, _, _ = _against_reference(rmat, 24, torch.float32, ("std", "min"), ("attenuation",), 0.8, True, "subset", 31)
    swapped = pna_ref.multi_aggregate_reference(rmat.rowptr.cpu(), rmat.col.cpu(), _inputs(rmat, 24, torch.float32, 2, 31)[1].double(),
                                                _inputs(rmat, 24, torch.float32, 2, 31)[2].double(), ("min", "std"), ("attenuation",), 0.8)
    assert torch.equal(want[:, :24], swapped[:, 24:]) and not torch.equal(want[:, :24], swapped[:, :24])
    seen = []
    real = ops_agg.forward_raw

    def spy(*args, **kwargs):
        res = real(*args, **kwargs)
        seen.append((res[1] is not None, res[2] is not None))
        return res

    monkeypatch.setattr(ops_agg, "forward_raw", spy)
    x = torch.randn(1024, 16, device=DEV)
    y = torch.randn(1024, 16, device=DEV)
    ops_agg.multi_aggregate(rmat, x, y)                                                         # no gradient: nothing
    ops_agg.multi_aggregate(rmat, x, y.clone().requires_grad_())                                # y alone: nothing
    ops_agg.multi_aggregate(rmat, x.clone().requires_grad_(), y, ("mean", "sum"))               # x, but neither var nor max
    ops_agg.multi_aggregate(rmat, x.clone().requires_grad_(), y, ("std", "mean"))               # stats alone
    ops_agg.multi_aggregate(rmat, x.clone().requires_grad_(), y, ("max",), ("identity",))       # arg alone
    ops_agg.multi_aggregate(rmat, x.clone().requires_grad_(), y, ("std", "min"), ("attenuation",))
    assert seen == [(False, False), (False, False), (False, False), (True, False), (False, True), (True, True)]


def _step(graph, x, y, g, aggs=DEFAULT_AGGS):
    from dgll_amd import ops_agg

    out = ops_agg.multi_aggregate(graph, x, y, aggs, DEFAULT_SCALERS, 1.3)
    return (out.detach(),) + tuple(torch.autograd.grad(out, (x, y), g))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_reruns_and_strided_inputs_give_the_same_bits(rmat, edge_graph, dtype):
    for graph in (rmat, edge_graph):
        _, x, y, go = _inputs(graph, 64, dtype, 18, 3)
        x, y, go = x.to(DEV).requires_grad_(), y.to(DEV).requires_grad_(), go.to(DEV)
        first = _step(graph, x, y, go, pna_ref.AGGREGATORS)
        again = _step(graph, x, y, go, pna_ref.AGGREGATORS)
        for name, a, b in zip(("out", "gx", "gy"), first, again):
            assert torch.equal(a, b), name
        wide = torch.zeros(graph.n_cols, 96, dtype=dtype, device=DEV)
        wide[:, 16:80] = x.detach()
        view = wide[:, 16:80].requires_grad_()                      # a column slice of a wider matrix: rows on a 16-byte pitch, read in place
        for name, a, b in zip(("out", "gx", "gy"), first, _step(graph, view, y, go, pna_ref.AGGREGATORS)):
            assert torch.equal(a, b), name
        odd = torch.zeros(graph.n_cols, 67, dtype=dtype, device=DEV)
        odd[:, 3:] = x.detach()
        view = odd[:, 3:].requires_grad_()                          # an unaligned slice: copied once
        for name, a, b in zip(("out", "gx", "gy"), first, _step(graph, view, y, go, pna_ref.AGGREGATORS)):
            assert torch.equal(a, b), name


def test_gradients_are_skipped_where_not_needed(rmat):
    from dgll_amd import ops, ops_agg

    _, x, y, go = _inputs(rmat, 32, torch.float32, 12, 5)
    x, y, go = x.to(DEV), y.to(DEV), go.to(DEV)
    full = _step(rmat, x.clone().requires_grad_(), y.clone().requires_grad_(), go)
    for need_x, need_y, tags in ((True, False, {"magg_forward": 1, "magg_rows": 1, "magg_cols": 1}), (False, True, {"magg_forward": 1, "magg_rows": 1}),
                                 (False, False, {"magg_forward": 1})):
        xs, ys = x.clone().requires_grad_(need_x), y.clone().requires_grad_(need_y)
        with ops.LaunchTimer() as timer:
            out = ops_agg.multi_aggregate(rmat, xs, ys, DEFAULT_AGGS, DEFAULT_SCALERS, 1.3)
            leaves = [t for t in (xs, ys) if t.requires_grad]
            grads = torch.autograd.grad(out, leaves, go) if leaves else ()
        assert torch.equal(out.detach(), full[0])
        for t, g in zip(leaves, grads):
            assert torch.equal(g, full[1] if t is xs else full[2])
        counts = {}
        for tag, (n, _) in timer.summary().items():
            counts[tag[0]] = counts.get(tag[0], 0) + n
        assert counts == tags, counts


def test_forward_backward_can_be_captured(rmat):
    """The shape of test_mp_gpu.py::test_forward_backward_can_be_captured; the inputs change between the replays."""
    _, x, y, g = _inputs(rmat, 64, torch.bfloat16, 12, 81)
    x, y, g = x.to(DEV).requires_grad_(), y.to(DEV).requires_grad_(), g.to(DEV)
    rmat.transpose()                                # the cached structure: built outside the capture, on a single stream

    def step():
        return _step(rmat, x, y, g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured, stream=side):
        static = step()
    for seed in (82, 83):
        fresh = _inputs(rmat, 64, torch.bfloat16, 12, seed)[1:]
        with torch.no_grad():
            for t, new in zip((x, y, g), fresh):
                t.copy_(new.to(DEV))
        eager = [t.clone() for t in step()]
        for t in static:
            t.zero_()
        captured.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("out", "gx", "gy"), static, eager):
            assert torch.equal(a, b), name


def test_nothing_to_gather():
    """nnz == 0 or no rows: zeros, with zero gradients, and no launch."""
    from dgll_amd import CSRGraph, ops, ops_agg

    empty = CSRGraph(torch.zeros(6, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None, 5, 7).to(DEV)
    none = CSRGraph(torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None, 0, 7).to(DEV)
    x = torch.randn(7, 16, device=DEV, requires_grad=True)
    y = torch.randn(5, 16, device=DEV, requires_grad=True)
    with ops.LaunchTimer() as timer:
        out = ops_agg.multi_aggregate(empty, x, y)
        assert out.shape == (5, 12 * 16) and out.abs().max().item() == 0.0
        gx, gy = torch.autograd.grad(out.sum(), (x, y))
        assert gx.abs().max().item() == 0.0 and gy.abs().max().item() == 0.0
        assert ops_agg.multi_aggregate(empty, x, None, ("std",), ("identity",)).shape == (5, 16)
        assert ops_agg.multi_aggregate(none, x, y[:0]).shape == (0, 12 * 16)
    assert timer.summary() == {}


# ---- nn.PNAConv -----------------------------------------------------------------------------------------------------------------------

def _layer_against_reference(graph, in_size, towers, dtype, training, label, seed):
    """PNAConv (fp32 parameters, activations of `dtype`) on the GPU against pna_ref.pna_conv_reference on the rounded inputs: the output
    and every parameter gradient at the bars (U.weight and U.bias, one affine map, as one vector: ahead of a batch norm in training mode
    the bias has no gradient but rounding residue); then a state_dict round trip into a fresh layer."""
    from dgll_amd.nn.Convolution import PNAConv

    fwd, grad = _kinds(dtype)
    torch.manual_seed(seed)
    layer = PNAConv(in_size, in_size, DEFAULT_AGGS, DEFAULT_SCALERS, 1.2, dropout=0.0, num_towers=towers)
    for tower in layer.towers:
        tower.batchnorm.running_mean.normal_()
        tower.batchnorm.running_var.uniform_(0.5, 2.0)
    layer.train(training)
    h_src = torch.randn(graph.n_cols, in_size).to(dtype)
    h_dst = torch.randn(graph.n_rows, in_size).to(dtype) if graph.n_rows != graph.n_cols else h_src
    g = torch.randn(graph.n_rows, in_size).to(dtype)
    rp, col = graph.rowptr.cpu(), graph.col.cpu()
    sd = {k: v.detach().clone().double().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in layer.state_dict().items()}
    want = pna_ref.pna_conv_reference(sd, rp, col, h_src.double(), h_dst.double(), DEFAULT_AGGS, DEFAULT_SCALERS, 1.2, towers, True, None, training)
    row = pna_ref.rows_of(rp)                       # distinct messages stay apart: the smallest non-zero variance of a row's messages
    for msg in pna_ref.edge_messages({k: v.detach() for k, v in sd.items()}, rp, col, h_src.double(), h_dst.double(), towers):
        parts = {}
        pna_ref.reduce_messages(msg, row, col.long(), graph.n_rows, ("var",), ("identity",), 1.0, parts)
        assert parts["var"][parts["var"] > 0].min().item() >= 1e-8
    want.backward(g.double())

    layer = layer.to(DEV)
    feat = h_src.to(DEV) if h_dst is h_src else (h_src.to(DEV), h_dst.to(DEV))
    got = layer(graph, feat)
    assert got.dtype == dtype and tuple(got.shape) == (graph.n_rows, in_size)
    _check(label, "out", got, want, fwd)
    got.backward(g.to(DEV))
    grads = {n: p.grad for n, p in layer.named_parameters()}
    missed = []                                     # every figure is printed before the first assertion fails
    for name in grads:
        if name.endswith("U.bias"):
            continue
        a, b = grads[name].flatten(), sd[name].grad.flatten()
        if name.endswith("U.weight"):
            a = torch.cat([a, grads[name[:-6] + "bias"].flatten()])
            b = torch.cat([b, sd[name[:-6] + "bias"].grad.flatten()])
        try:
            _check(label, name, a, b, grad)
        except AssertionError as err:
            missed.append(str(err))
    assert not missed, missed
    fresh = PNAConv(in_size, in_size, DEFAULT_AGGS, DEFAULT_SCALERS, 1.2, dropout=0.0, num_towers=towers).to(DEV)
    fresh.load_state_dict(layer.state_dict())
    fresh.train(False)
    layer.train(False)
    with torch.no_grad():
        assert torch.equal(fresh(graph, feat), layer(graph, feat))


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("in_size,towers", [(32, 1), (32, 2), (20, 2)], ids=["1tower", "2towers", "padded"])
def test_pnaconv_fp32_on_edge_case_rows(edge_graph, in_size, towers, training):
    _layer_against_reference(edge_graph, in_size, towers, torch.float32, training, "layer fp32", 3)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_pnaconv_bf16_on_rmat(rmat, training):
    # seed 9: the first from 4 upwards at which the smallest non-zero variance of a row's float64 messages is >= 1e-8 (4.7e-8)
    _layer_against_reference(rmat, 64, 4, torch.bfloat16, training, "layer bf16", 9)


def test_pnaconv_on_a_rectangular_block(rmat):
    """The first 200 rows of the rmat as a block: (feat_src, feat_dst) and feat_src alone (its first 200 rows are the destinations)
    give equal results."""
    from dgll_amd import CSRGraph
    from dgll_amd.nn.Convolution import PNAConv

    n_dst = 200
    end = int(rmat.rowptr[n_dst])
    block = CSRGraph(rmat.rowptr[:n_dst + 1].clone(), rmat.col[:end].clone(), None, n_dst, 1024)
    torch.manual_seed(9)
    layer = PNAConv(32, 32, DEFAULT_AGGS, DEFAULT_SCALERS, 1.1, num_towers=2).to(DEV)
    feat = torch.randn(1024, 32, device=DEV)
    pair = layer(block, (feat, feat[:n_dst].clone()))
    alone = layer(block, feat)
    assert tuple(pair.shape) == (n_dst, 32) and torch.equal(pair, alone)


def test_pna_trains_on_planted_communities():
    """30 Adam steps of the PNA model on the planted communities of test_mp_gpu.py::test_agnn_trains_on_planted_communities, at that
    test's threshold: the final loss below half the first, accuracy >= 0.9 (on the host path in fp32 this seed takes the loss below
    0.05 at accuracy 1.0)."""
    from dgll_amd import ops_agg, synth
    from dgll_amd.nn.Convolution import PNA

    n, k = 400, 4
    gen = torch.Generator().manual_seed(3)
    labels = torch.arange(n) % k
    prob = torch.where(labels[:, None] == labels[None, :], torch.tensor(0.05), torch.tensor(0.005))
    src, dst = (torch.rand(n, n, generator=gen) < prob).nonzero(as_tuple=True)
    graph = synth.build_graph(src, dst, n, symmetric=True, self_loops=True, weighted=False).to(DEV)
    x = (torch.nn.functional.one_hot(labels, k).float().repeat(1, 4) + torch.randn(n, 4 * k, generator=gen)).to(DEV)
    labels = labels.to(DEV)
    torch.manual_seed(3)
    model = PNA(4 * k, 16, k, n_layers=2, delta=ops_agg.pna_delta(graph), num_towers=2).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(graph, x).float(), labels)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    model.eval()
    acc = (model(graph, x).argmax(1) == labels).float().mean().item()
    print("loss %.4f -> %.4f, accuracy %.3f" % (losses[0], losses[-1], acc))
    assert losses[-1] < 0.5 * losses[0] and acc >= 0.9
