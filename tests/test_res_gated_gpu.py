"""ResGated aggregation on the GPU: dgll_amd.ops_res_gated.res_gated_sum (the output and the three gradients, sum and mean) against
the float64 per-edge restatement of res_gated_ref.py, on the graphs and widths of test_res_gated_emulated.py; the memory condition
(nothing of the size of the edge list is allocated); nn.ResGatedGraphConv and ResGatedGCN against their own host path on copied
parameters.  For bf16 the reference runs on the bf16-rounded inputs.

Bars: fp32 forward max |err| <= 1e-4 max |ref|, fp32 gradients <= 2e-3 max |ref|; bf16 forward <= 2e-2 max |ref|,
bf16 gradients relative L2 <= 1.5e-2.  No element is excluded (res_gated_ref.py)."""
import copy
import itertools

import numpy as np
import pytest
import torch

import res_gated_ref
from test_edge_feat_gpu import _sampler_block
from test_gated_gpu import _smooth
from test_pna_emulated import _graph

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIVE, FIVE_COL = 4, 11      # the row of the full graph that lists one column five times, and that column
WIDTHS = [(4, torch.float32), (24, torch.float32), (260, torch.float32), (8, torch.bfloat16), (48, torch.bfloat16), (520, torch.bfloat16)]
_ids = lambda v: str(v).replace("torch.", "")       # noqa: E731
_REF = {}


def _check(name, got, want, kind):
    a, b = got.detach().double().cpu(), want.detach().double().cpu()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert bool(torch.isfinite(a).all()), "%s: not finite" % name
    err_max = ((a - b).abs().max() / b.abs().max()).item()
    err_l2 = ((a - b).norm() / b.norm()).item()
    bar, err = {"fwd32": (1e-4, err_max), "grad32": (2e-3, err_max), "fwd16": (2e-2, err_max), "grad16": (1.5e-2, err_l2)}[kind]
    print("%-34s max/max %.3e  rel-l2 %.3e  bar %.1e" % (name, err_max, err_l2, bar))
    assert err <= bar, (name, err, bar)


def _kinds(dtype):
    return ("fwd32", "grad32") if dtype == torch.float32 else ("fwd16", "grad16")


def _inputs(graph, F, dtype, seed):
    """k, q, v and the output gradient, as stored"""
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, F, generator=gen).to(dtype) for n in (graph.n_rows, graph.n_cols, graph.n_cols, graph.n_rows)]


def _reference(cpu, ins):
    x64 = [t.double() for t in ins]
    return {mean: (res_gated_ref.forward(cpu.rowptr, cpu.col, *x64[:3], mean=mean),
                   res_gated_ref.gradients(cpu.rowptr, cpu.col, *x64[:3], x64[3], mean=mean)) for mean in (False, True)}


def _case(F, dtype):
    """the graph, the inputs and the float64 reference of one width, computed once"""
    if (F, dtype) not in _REF:
        cpu = _graph(full=F < 260)
        ins = _inputs(cpu, F, dtype, F + 5)
        _REF[(F, dtype)] = (cpu, ins, _reference(cpu, ins))
    return _REF[(F, dtype)]


def _op(graph, ins, needs=(True, True, True), reduce="sum", go=None):
    """res_gated_sum and its backward on the GPU -> (out, [grad_k, grad_q, grad_v])"""
    from dgll_amd import ops_res_gated

    leaves = [t.to(DEV).requires_grad_(n) for t, n in zip(ins[:3], needs)]
    out = ops_res_gated.res_gated_sum(graph, *leaves, reduce=reduce)
    if any(needs):
        out.backward((ins[3] if go is None else go).to(DEV))
    return out.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("F,dtype", WIDTHS, ids=_ids)
def test_op_against_the_reference(F, dtype, reduce):
    cpu, ins, want = _case(F, dtype)
    want_out, want_grads = want[reduce == "mean"]
    fwd, grad = _kinds(dtype)
    out, grads = _op(cpu.to(DEV), ins, reduce=reduce)
    assert out.dtype == dtype and tuple(out.shape) == (cpu.n_rows, F)
    _check("out", out, want_out, fwd)
    for name, g, w in zip("kqv", grads, want_grads):
        assert g.dtype == dtype and g.shape == w.shape
        _check("grad_" + name, g, w, grad)
    # rows without entries give exact zeros in out and grad_k; the source no row references in grad_q and grad_v
    for r in (0, cpu.n_rows - 1):
        assert out[r].abs().max().item() == 0.0 and grads[0][r].abs().max().item() == 0.0
    assert grads[1][-1].abs().max().item() == 0.0 and grads[2][-1].abs().max().item() == 0.0


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("F,dtype", [(24, torch.float32), (48, torch.bfloat16)], ids=_ids)
def test_op_on_a_rectangular_sampler_block(F, dtype, reduce):
    cpu = _sampler_block()
    assert cpu.n_rows != cpu.n_cols
    ins = _inputs(cpu, F, dtype, 31)
    want_out, want_grads = _reference(cpu, ins)[reduce == "mean"]
    fwd, grad = _kinds(dtype)
    out, grads = _op(cpu.to(DEV), ins, reduce=reduce)
    _check("out", out, want_out, fwd)
    for name, g, w in zip("kqv", grads, want_grads):
        _check("grad_" + name, g, w, grad)
    assert out[7].abs().max().item() == 0.0 and grads[0][7].abs().max().item() == 0.0       # the block's empty row


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_the_transposed_pass_reads_the_right_rows(dtype):
    """The graph is not symmetric and A^T's entry order differs from A's.  With the output gradient on the five-times row alone,
    grad_q and grad_v are non-zero at that row's one column and exact zeros everywhere else, and grad_k is non-zero in that row alone."""
    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    gt, perm = graph.transpose()
    assert not torch.equal(perm.cpu(), torch.arange(cpu.nnz)) and gt.n_rows != graph.n_rows
    ins = _inputs(cpu, 8, dtype, 21)
    b = int(cpu.rowptr[FIVE])
    assert cpu.col[b:b + 5].tolist() == [FIVE_COL] * 5 and int(cpu.rowptr[FIVE + 1]) == b + 5
    only = torch.zeros_like(ins[3])
    only[FIVE] = ins[3][FIVE]
    _, (gk, gq, gv) = _op(graph, ins, go=only)
    want = res_gated_ref.gradients(cpu.rowptr, cpu.col, *(t.double() for t in ins[:3]), only.double())
    grad = _kinds(dtype)[1]
    for name, g, w in zip("kqv", (gk, gq, gv), want):
        _check("grad_" + name, g, w, grad)
    others = torch.ones(cpu.n_cols, dtype=torch.bool)
    others[FIVE_COL] = False
    assert gq.cpu()[others].abs().max().item() == 0.0 and gv.cpu()[others].abs().max().item() == 0.0
    assert gq[FIVE_COL].abs().min().item() > 0.0 and gv[FIVE_COL].abs().min().item() > 0.0
    assert gk.cpu()[torch.arange(cpu.n_rows) != FIVE].abs().max().item() == 0.0 and gk[FIVE].abs().min().item() > 0.0


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_pitched_operands_with_nan_in_the_padding(dtype, reduce):
    """every operand and the output gradient on a pitch wider than F, NaN behind the row: the same bits as from compact operands, and
    (raw pass) the padding of a pitched output is untouched"""
    from dgll_amd import _lib, ops_res_gated

    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    F, vec = 24, 8 if dtype == torch.bfloat16 else 4
    ins = _inputs(cpu, F, dtype, 13)

    def pitched(t):
        buf = torch.full((t.shape[0], F + 2 * vec), float("nan"), dtype=dtype, device=DEV)
        buf[:, :F] = t.to(DEV)
        return buf[:, :F]

    want_out, want_grads = _op(graph, ins, reduce=reduce)
    wide = [pitched(t) for t in ins]
    assert all(t.stride(0) == F + 2 * vec for t in wide)
    leaves = [t.detach().requires_grad_() for t in wide[:3]]
    out = ops_res_gated.res_gated_sum(graph, *leaves, reduce=reduce)
    out.backward(wide[3])
    assert torch.equal(out.detach(), want_out)
    for got, ref in zip(leaves, want_grads):
        assert torch.equal(got.grad, ref)
    if reduce == "sum":     # a raw cols pass into a pitched grad_q: the columns behind F keep their fill
        gq_buf = torch.full((cpu.n_cols, F + 2 * vec), 7.0, dtype=dtype, device=DEV)
        gv = torch.empty(cpu.n_cols, F, dtype=dtype, device=DEV)
        gt = graph.transpose()[0]
        ops_res_gated._launch(_lib.RES_GATED_COLS, gt, wide[1], k=wide[0], q=wide[1], v=wide[2], grad_out=wide[3], grad_q=gq_buf[:, :F],
                              grad_v=gv)
        assert torch.equal(gq_buf[:, :F], want_grads[1]) and bool((gq_buf[:, F:] == 7.0).all()) and torch.equal(gv, want_grads[2])
        assert torch.equal(ops_res_gated.forward_raw(graph, *wide[:3]), want_out)
        assert torch.equal(ops_res_gated.rows_raw(graph, *wide), want_grads[0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_saturated_gates(dtype):
    """rows whose gates are all open (k = +100), all closed (k = -100) and a row with both and ordinary columns: everything finite and
    inside the bars; a saturated gate is exactly 0 or 1 and s (1 - s) exactly 0"""
    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    ins = _inputs(cpu, 8, dtype, 17)
    open_row, closed_row, mixed_row = 2, 3, 5                                       # 64, 65 and 256 entries
    ins[0][open_row] = 100.0
    ins[0][closed_row] = -100.0
    ins[0][mixed_row, 0::3] = 100.0
    ins[0][mixed_row, 1::3] = -100.0
    fwd, grad = _kinds(dtype)
    want = _reference(cpu, ins)
    for reduce in ("sum", "mean"):
        want_out, want_grads = want[reduce == "mean"]
        out, grads = _op(graph, ins, reduce=reduce)
        _check("out", out, want_out, fwd)
        for name, g, w in zip("kqv", grads, want_grads):
            _check("grad_" + name, g, w, grad)
        assert out[closed_row].abs().max().item() == 0.0                            # every gate exactly 0
        for r in (open_row, closed_row):
            assert grads[0][r].abs().max().item() == 0.0
        assert grads[0][mixed_row, 0::3].abs().max().item() == 0.0 and grads[0][mixed_row, 1::3].abs().max().item() == 0.0
        assert out[mixed_row, 1::3].abs().max().item() == 0.0 and grads[0][mixed_row, 2::3].abs().min().item() > 0.0


def test_only_the_wanted_gradients_are_computed_and_reruns_give_the_same_bits():
    from dgll_amd import ops

    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    ins = _inputs(cpu, 24, torch.float32, 9)
    for reduce in ("sum", "mean"):
        full = _op(graph, ins, reduce=reduce)
        again = _op(graph, ins, reduce=reduce)
        assert torch.equal(full[0], again[0])                                       # no atomics: identical bits
        assert all(torch.equal(x, y) for x, y in zip(full[1], again[1]))
        for needs in itertools.product((True, False), repeat=3):                    # (k, q, v)
            with ops.LaunchTimer() as timer:
                out, grads = _op(graph, ins, needs=needs, reduce=reduce)
            tags = [tag[0] for tag, _, _ in timer.records]
            assert tags.count("res_gated_forward") == 1
            assert tags.count("res_gated_rows") == (1 if needs[0] else 0), (needs, tags)
            assert tags.count("res_gated_cols") == (1 if needs[1] or needs[2] else 0), (needs, tags)
            assert torch.equal(out, full[0])
            for need, got, ref in zip(needs, grads, full[1]):
                assert (got is None) == (not need)
                if need:
                    assert torch.equal(got, ref), needs


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_the_op_replays_from_a_captured_graph(reduce):
    from dgll_amd import ops_res_gated

    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    graph.transpose()                                                               # the cached structure and the inverse degrees,
    graph.inv_degrees()                                                             # built outside the capture
    ins = [t.to(DEV) for t in _inputs(cpu, 24, torch.float32, 3)]
    leaves = [t.requires_grad_() for t in ins[:3]]

    def step():
        out = ops_res_gated.res_gated_sum(graph, *leaves, reduce=reduce)
        return (out.detach(),) + tuple(torch.autograd.grad(out, leaves, ins[3]))

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
        for name, got, ref in zip(("out", "grad_k", "grad_q", "grad_v"), static, eager):
            assert torch.equal(got, ref), name


def test_empty_graphs_give_zeros_with_zero_gradients():
    from dgll_amd import CSRGraph, ops_res_gated

    for n_dst, reduce in ((3, "sum"), (3, "mean"), (0, "sum")):
        g = CSRGraph(torch.zeros(n_dst + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None, n_dst, 5).to(DEV)
        k, q, v = (torch.randn(n, 8, device=DEV, requires_grad=True) for n in (n_dst, 5, 5))
        out = ops_res_gated.res_gated_sum(g, k, q, v, reduce=reduce)
        assert tuple(out.shape) == (n_dst, 8) and (n_dst == 0 or out.abs().max().item() == 0.0)
        out.sum().backward()
        assert all(t.grad.shape == t.shape and (t.numel() == 0 or t.grad.abs().max().item() == 0.0) for t in (k, q, v))


def test_nothing_of_the_size_of_the_edge_list_is_allocated():
    """256 x 256, 64 entries a row (nnz = 16384), F = 64 fp32: one [nnz, F] array would be 4 MiB.  The peak of a forward and backward
    above what is allocated before them -- the output, the output gradient and the three gradients, 64 KiB each -- stays below a
    quarter of that, for the sum and for the mean.  A condition, not a measurement.  ops_gated.gated_sum with a zero c, the same
    aggregation up to its normalisation, does not meet it: its c and ehat are real per-edge arrays."""
    from dgll_amd import CSRGraph, ops_gated, ops_res_gated

    n, deg, F = 256, 64, 64
    rng = np.random.RandomState(5)
    col = torch.from_numpy(np.concatenate([rng.choice(n, deg, replace=False) for _ in range(n)]).astype(np.int32))
    graph = CSRGraph(torch.arange(n + 1, dtype=torch.int64) * deg, col, None, n, n).to(DEV)
    nnz = graph.nnz
    assert nnz == 16384
    graph.transpose()
    graph.inv_degrees()
    gen = torch.Generator().manual_seed(5)
    k, q, v, go = (torch.randn(n, F, generator=gen).to(DEV) for _ in range(4))
    bound = nnz * F * 4 // 4

    def peak(fn):
        leaves = [t.clone().requires_grad_() for t in (k, q, v)]
        fn(leaves).backward(go)                                                     # once outside the measurement: lazy initialisation
        for t in leaves:
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn(leaves).backward(go)
        torch.cuda.synchronize()
        assert all(t.grad is not None for t in leaves)
        return torch.cuda.max_memory_allocated() - before

    for reduce in ("sum", "mean"):
        used = peak(lambda leaves: ops_res_gated.res_gated_sum(graph, *leaves, reduce=reduce))
        print("res_gated_sum %-4s peak above the inputs %d bytes, bound %d" % (reduce, used, bound))
        assert used < bound, (reduce, used, bound)
    c = torch.zeros(nnz, F, device=DEV)
    used = peak(lambda leaves: ops_gated.gated_sum(graph, leaves[0], leaves[1], c, leaves[2])[0])
    print("gated_sum with a zero c: %d bytes" % used)
    assert used >= bound


# ---- the layer and the model against their host path ----------------------------------------------------------------------------------

def _against_the_host_path(module, cpu, feats, dtype, training, pair=False):
    """module(graph, feats) on the GPU in `dtype` (fp32 parameters) against a float64 copy on the host with the inputs as stored: the
    output, the parameter gradients (weight and bias of a Linear, one affine map, as one vector) and the input gradients at the bars
    (test_gated_gpu._against_the_host_path without the edge input).  Every figure is printed before the first assertion fails."""
    fwd, grad = _kinds(dtype)
    module.train(training)
    host = copy.deepcopy(module).double()
    ins = [t.to(dtype) for t in feats]
    ins64 = [t.double().requires_grad_() for t in ins]
    want = host(cpu, tuple(ins64) if pair else ins64[0])
    go = torch.randn(want.shape, generator=torch.Generator().manual_seed(11)).to(dtype)
    names = [n for n, _ in host.named_parameters()] + ["input%d" % i for i in range(len(ins))]
    ref = dict(zip(names, torch.autograd.grad(want, list(host.parameters()) + ins64, go.double())))

    module = module.to(DEV)
    ins_g = [t.to(DEV).requires_grad_() for t in ins]
    out = module(cpu.to(DEV), tuple(ins_g) if pair else ins_g[0])
    assert out.dtype == dtype and out.is_cuda and out.shape == want.shape
    got = dict(zip(names, torch.autograd.grad(out, list(module.parameters()) + ins_g, go.to(DEV))))
    label = "%s %s " % (type(module).__name__, _ids(dtype))
    missed = []

    def check(name, a, b, kind):
        try:
            _check(label + name, a, b, kind)
        except AssertionError as err:
            missed.append(str(err))

    check("out", out, want, fwd)
    for name in names:
        if name.endswith(".bias") and name[:-4] + "weight" in got:                  # a Linear's bias goes with its weight
            continue
        a, b = got[name].flatten().cpu(), ref[name].flatten()
        if name.endswith(".weight") and name[:-6] + "bias" in got:
            a, b = torch.cat([a, got[name[:-6] + "bias"].flatten().cpu()]), torch.cat([b, ref[name[:-6] + "bias"].flatten()])
        check("grad " + name, a, b, grad)
    assert not missed, missed


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("root_weight,bias,fout,aggr", [(True, True, 8, "add"), (True, False, 10, "mean"), (False, True, 10, "add"),
                                                        (False, False, 8, "mean")], ids=["skip-bias", "skip-F10-mean", "bias-F10", "bare-mean"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_resgatedgraphconv_against_its_host_path(dtype, root_weight, bias, fout, aggr, training):
    """a sampler block with a (src, dst) pair of different widths; out_channels = 10 is padded with zero weight rows and sliced"""
    from dgll_amd.nn.Convolution import ResGatedGraphConv

    cpu = _sampler_block()
    gen = torch.Generator().manual_seed(fout)
    x_src, x_dst = torch.randn(cpu.n_cols, 6, generator=gen), torch.randn(cpu.n_rows, 5, generator=gen)
    torch.manual_seed(fout)
    layer = ResGatedGraphConv((6, 5), fout, root_weight=root_weight, bias=bias, aggr=aggr)
    if bias:
        with torch.no_grad():
            layer.bias.copy_(torch.randn(fout, generator=gen))
    _against_the_host_path(layer, cpu, [x_src, x_dst], dtype, training, pair=True)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_resgatedgcn_model_against_its_host_path(dtype, training):
    """relu for fp32; for bf16 the smooth activation of test_gated_gpu._smooth, for the reason given there (a relu's gate flips on
    bf16-rounded inputs near 0, whatever the kernels do)"""
    from dgll_amd.nn.Convolution import ResGatedGCN

    cpu = _sampler_block(n_dst=150, n_src=150)
    x = torch.randn(150, 8, generator=torch.Generator().manual_seed(8))
    torch.manual_seed(8)
    _against_the_host_path(ResGatedGCN(8, 16, 8, layers=2, activation=_smooth(dtype)), cpu, [x], dtype, training)
