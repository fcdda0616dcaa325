"""Edge-gated aggregation on the GPU: dgll_amd.ops_gated.gated_sum (both outputs and the four gradients, with and without a gradient
through ehat) against the float64 per-edge restatement of gated_ref.py, on the graphs and widths of test_gated_emulated.py;
nn.GatedGCNConv and GatedGCN against their own host path on copied parameters.  For bf16 the reference runs on the bf16-rounded
inputs.

Bars: fp32 forward (out and ehat) max |err| <= 1e-4 max |ref|, fp32 gradients <= 2e-3 max |ref|; bf16 forward
<= 2e-2 max |ref|, bf16 gradients relative L2 <= 1.5e-2.  No element is excluded (gated_ref.py)."""
import copy

import pytest
import torch

import gated_ref
from test_edge_feat_gpu import _sampler_block
from test_pna_emulated import _graph

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-6
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
    """a, b, c, v, the output gradient and the gradient through ehat, as stored"""
    gen = torch.Generator().manual_seed(seed)
    rows = (graph.n_rows, graph.n_cols, graph.nnz, graph.n_cols, graph.n_rows, graph.nnz)
    return [torch.randn(n, F, generator=gen).to(dtype) for n in rows]


def _case(F, dtype):
    """the graph, the inputs and the float64 reference of one width, computed once"""
    if (F, dtype) not in _REF:
        cpu = _graph(full=F < 260)
        ins = _inputs(cpu, F, dtype, F + 5)
        x64 = [t.double() for t in ins]
        fwd = gated_ref.forward(cpu.rowptr, cpu.col, *x64[:4], EPS)
        grads = {with_ge: gated_ref.gradients(cpu.rowptr, cpu.col, *x64[:4], EPS, x64[4], x64[5] if with_ge else None)
                 for with_ge in (False, True)}
        _REF[(F, dtype)] = (cpu, ins, fwd, grads)
    return _REF[(F, dtype)]


def _op(graph, ins, needs=(True, True, True, True), with_ge=True, go=None, ge=None):
    """gated_sum and its backward on the GPU -> (out, ehat, [grad_a, grad_b, grad_c, grad_v])"""
    from dgll_amd import ops_gated

    leaves = [t.to(DEV).requires_grad_(n) for t, n in zip(ins[:4], needs)]
    out, ehat = ops_gated.gated_sum(graph, *leaves, EPS)
    go = ins[4] if go is None else go
    loss_outs, loss_grads = [out], [go.to(DEV)]
    if with_ge:
        loss_outs.append(ehat)
        loss_grads.append((ins[5] if ge is None else ge).to(DEV))
    if any(needs):
        torch.autograd.backward(loss_outs, loss_grads)
    return out.detach(), ehat.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("with_ge", [False, True], ids=["noge", "ge"])
@pytest.mark.parametrize("F,dtype", WIDTHS, ids=_ids)
def test_op_against_the_reference(F, dtype, with_ge):
    cpu, ins, (want_out, want_ehat), want_grads = _case(F, dtype)
    fwd, grad = _kinds(dtype)
    out, ehat, grads = _op(cpu.to(DEV), ins, with_ge=with_ge)
    assert out.dtype == dtype and tuple(out.shape) == (cpu.n_rows, F) and ehat.dtype == dtype and tuple(ehat.shape) == (cpu.nnz, F)
    _check("out", out, want_out, fwd)
    _check("ehat", ehat, want_ehat, fwd)
    for name, g, w in zip("abcv", grads, want_grads[with_ge]):
        assert g.dtype == dtype
        _check("grad_" + name, g, w, grad)
    # rows without entries give exact zeros in out and grad_a; the source no row references in grad_b and grad_v
    for r in (0, cpu.n_rows - 1):
        assert out[r].abs().max().item() == 0.0 and grads[0][r].abs().max().item() == 0.0
    assert grads[1][-1].abs().max().item() == 0.0 and grads[3][-1].abs().max().item() == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_the_transposed_pass_reads_each_duplicates_own_rows(dtype):
    """The graph is not symmetric and A^T's entry order differs from A's.  With the output gradient on the five-times row alone and none
    through ehat, grad_b of its column is the sum of exactly those five t rows (grad_c as stored), whose five c rows differ; every
    other row of grad_b and grad_v is exactly 0.  (All five entries gather the same v_j, so out_i = v_j S / (S + eps) and v_j - out_i is
    of order eps: t is a cancelled difference there, and it is held against the kernel's own stored t rows, not against float64;
    grad_v has no such difference and is held against the reference.)"""
    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    gt, perm = graph.transpose()
    assert not torch.equal(perm.cpu(), torch.arange(cpu.nnz)) and gt.n_rows != graph.n_rows
    ins = _inputs(cpu, 8, dtype, 21)
    b = int(cpu.rowptr[FIVE])
    assert cpu.col[b:b + 5].tolist() == [FIVE_COL] * 5 and int(cpu.rowptr[FIVE + 1]) == b + 5
    assert len({tuple(r) for r in ins[2][b:b + 5].tolist()}) == 5                   # five different c rows
    only = torch.zeros_like(ins[4])
    only[FIVE] = ins[4][FIVE]
    _, _, (ga, gb, gc, gv) = _op(graph, ins, with_ge=False, go=only)
    x64 = [t.double() for t in ins[:4]]
    want = gated_ref.gradients(cpu.rowptr, cpu.col, *x64, EPS, only.double())
    grad = _kinds(dtype)[1]
    _check("grad_v", gv, want[3], grad)
    _check("grad_b of the column", gb[FIVE_COL], gc[b:b + 5].double().sum(0), grad)
    assert len({tuple(r) for r in gc[b:b + 5].tolist()}) == 5
    others = torch.ones(cpu.n_cols, dtype=torch.bool)
    others[FIVE_COL] = False
    assert gb.cpu()[others].abs().max().item() == 0.0 and gv.cpu()[others].abs().max().item() == 0.0
    rest = torch.ones(cpu.nnz, dtype=torch.bool)
    rest[b:b + 5] = False
    assert gc.cpu()[rest].abs().max().item() == 0.0 and ga.cpu()[torch.arange(cpu.n_rows) != FIVE].abs().max().item() == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_pitched_operands_with_nan_in_the_padding(dtype):
    """every operand and both output gradients on a pitch wider than F, NaN behind the row: the same bits as from compact operands, and
    (raw passes) the padding of pitched outputs is untouched"""
    from dgll_amd import ops_gated

    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    F, vec = 24, 8 if dtype == torch.bfloat16 else 4
    ins = _inputs(cpu, F, dtype, 13)

    def pitched(t):
        buf = torch.full((t.shape[0], F + 2 * vec), float("nan"), dtype=dtype, device=DEV)
        buf[:, :F] = t.to(DEV)
        return buf[:, :F]

    want = _op(graph, ins)
    wide = [pitched(t) for t in ins]
    assert all(t.stride(0) == F + 2 * vec for t in wide)
    leaves = [t.detach().requires_grad_() for t in wide[:4]]
    out, ehat = ops_gated.gated_sum(graph, *leaves, EPS)
    torch.autograd.backward([out, ehat], [wide[4], wide[5]])
    assert torch.equal(out.detach(), want[0]) and torch.equal(ehat.detach(), want[1])
    for got, ref in zip(leaves, want[2]):
        assert torch.equal(got.grad, ref)
    # raw rows pass into a pitched grad_c: the columns behind F keep their fill
    out_r, ehat_r, inv_s, out32 = ops_gated.forward_raw(graph, *wide[:4], EPS)
    assert torch.equal(out_r, want[0]) and torch.equal(ehat_r, want[1])
    gc_buf = torch.full((cpu.nnz, F + 2 * vec), 7.0, dtype=dtype, device=DEV)
    d_ptr = gc_buf[:, :F]
    from dgll_amd import _lib
    ga = torch.empty(cpu.n_rows, F, dtype=dtype, device=DEV)
    ops_gated._launch(_lib.GATED_ROWS, graph, None, cpu.nnz, EPS, wide[4], v=wide[3], ehat=ehat_r, inv_s=inv_s, out32=out32,
                      grad_out=wide[4], grad_ehat=wide[5], grad_c=d_ptr, grad_a=ga)
    assert torch.equal(gc_buf[:, :F], want[2][2]) and bool((gc_buf[:, F:] == 7.0).all()) and torch.equal(ga, want[2][0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_saturated_gates(dtype):
    """rows whose gates are all open (c = +100), all closed (c = -100) and mixed: everything finite and inside the bars; a saturated
    gate is exactly 0 or 1, so with no gradient through ehat its t is an exact 0"""
    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    ins = _inputs(cpu, 8, dtype, 17)
    c = ins[2]
    rp = cpu.rowptr.tolist()
    open_row, closed_row, mixed_row = 2, 3, 5                                       # 64, 65 and 256 entries
    c[rp[open_row]:rp[open_row + 1]] = 100.0
    c[rp[closed_row]:rp[closed_row + 1]] = -100.0
    c[rp[mixed_row]:rp[mixed_row + 1]:2] = 100.0
    c[rp[mixed_row] + 1:rp[mixed_row + 1]:3] = -100.0
    x64 = [t.double() for t in ins]
    fwd, grad = _kinds(dtype)
    want_out, want_ehat = gated_ref.forward(cpu.rowptr, cpu.col, *x64[:4], EPS)
    for with_ge in (False, True):
        out, ehat, grads = _op(graph, ins, with_ge=with_ge)
        want = gated_ref.gradients(cpu.rowptr, cpu.col, *x64[:4], EPS, x64[4], x64[5] if with_ge else None)
        _check("out", out, want_out, fwd)
        _check("ehat", ehat, want_ehat, fwd)
        for name, g, w in zip("abcv", grads, want):
            _check("grad_" + name, g, w, grad)
        if not with_ge:
            for r in (open_row, closed_row):
                assert grads[2][rp[r]:rp[r + 1]].abs().max().item() == 0.0 and grads[0][r].abs().max().item() == 0.0
    assert out[closed_row].abs().max().item() == 0.0                                # every gate exactly 0: 0 / eps


def test_only_the_wanted_gradients_are_computed_and_reruns_give_the_same_bits():
    from dgll_amd import ops

    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    ins = _inputs(cpu, 24, torch.float32, 9)
    full = _op(graph, ins)
    again = _op(graph, ins)
    assert torch.equal(full[0], again[0]) and torch.equal(full[1], again[1])        # no atomics: identical bits
    assert all(torch.equal(x, y) for x, y in zip(full[2], again[2]))
    #            needs (a, b, c, v)            rows   cols
    for needs, rows, cols in (((True, False, False, False), True, False), ((False, False, True, False), True, False),
                              ((True, False, True, False), True, False), ((False, True, False, False), True, True),
                              ((False, False, False, True), True, True), ((False, True, True, True), True, True),
                              ((False, False, False, False), False, False)):
        with ops.LaunchTimer() as timer:
            out, ehat, grads = _op(graph, ins, needs=needs)
        tags = [tag[0] for tag, _, _ in timer.records]
        assert tags.count("gated_forward") == 1
        assert tags.count("gated_rows") == (1 if rows else 0) and tags.count("gated_cols") == (1 if cols else 0), (needs, tags)
        assert torch.equal(out, full[0]) and torch.equal(ehat, full[1])
        for need, got, ref in zip(needs, grads, full[2]):
            assert (got is None) == (not need)
            if need:
                assert torch.equal(got, ref), needs
    # a gradient through ehat alone (out unused): grad_c is ge, grad_a and grad_b its row and column sums, grad_v zero
    from dgll_amd import ops_gated
    leaves = [t.to(DEV).requires_grad_() for t in ins[:4]]
    _, ehat = ops_gated.gated_sum(graph, *leaves, EPS)
    ehat.backward(ins[5].to(DEV))
    assert torch.equal(leaves[2].grad.cpu(), ins[5]) and leaves[3].grad.abs().max().item() == 0.0
    _check("grad_a", leaves[0].grad, torch.zeros(cpu.n_rows, 24, dtype=torch.float64).index_add_(0, cpu.row_index(), ins[5].double()), "grad32")
    _check("grad_b", leaves[1].grad, torch.zeros(cpu.n_cols, 24, dtype=torch.float64).index_add_(0, cpu.col.long(), ins[5].double()), "grad32")


def test_the_op_replays_from_a_captured_graph():
    from dgll_amd import ops_gated

    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    graph.transpose()                                                               # the cached structure, built outside the capture
    ins = [t.to(DEV) for t in _inputs(cpu, 24, torch.float32, 3)]
    leaves = [t.requires_grad_() for t in ins[:4]]

    def step():
        out, ehat = ops_gated.gated_sum(graph, *leaves, EPS)
        return (out.detach(), ehat.detach()) + tuple(torch.autograd.grad((out, ehat), leaves, (ins[4], ins[5])))

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
        for name, got, ref in zip(("out", "ehat", "grad_a", "grad_b", "grad_c", "grad_v"), static, eager):
            assert torch.equal(got, ref), name


def test_empty_graphs_give_zeros_with_zero_gradients():
    from dgll_amd import CSRGraph, ops_gated

    g = CSRGraph(torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None, 3, 5).to(DEV)
    a, b, v = (torch.randn(n, 8, device=DEV, requires_grad=True) for n in (3, 5, 5))
    c = torch.randn(0, 8, device=DEV, requires_grad=True)
    out, ehat = ops_gated.gated_sum(g, a, b, c, v)
    assert tuple(out.shape) == (3, 8) and out.abs().max().item() == 0.0 and tuple(ehat.shape) == (0, 8)
    (out.sum() + ehat.sum()).backward()
    assert all(t.grad.abs().max().item() == 0.0 for t in (a, b, v)) and tuple(c.grad.shape) == (0, 8)


# ---- the layer and the model against their host path ----------------------------------------------------------------------------------

def _smooth(dtype):
    """The activation of the layer comparisons.  relu for fp32.  For bf16 a smooth one (silu): relu's gate is the sign of the batch-norm
    output, which on the GPU is formed from bf16-rounded sums (relative error 2^-9) and in the float64 host path from exact ones, so the
    elements within that error of 0 -- about one in a thousand -- open on one side and stay shut on the other, and each of them puts an
    error of the element's full size into the gradients: sqrt(1e-3 / 0.5), some 4 % in relative L2, whatever the kernels do.  That is a
    property of the number format, not of the layer; a smooth activation keeps the comparison about the layer."""
    return torch.nn.functional.relu if dtype == torch.float32 else torch.nn.functional.silu


def _against_the_host_path(module, cpu, feats, edge, dtype, training, pair=False):
    """module(graph, feats, edge) on the GPU in `dtype` (fp32 parameters) against a float64 copy on the host with the inputs as
    stored: every output, the parameter gradients (weight and bias of a Linear, one affine map, as one vector: ahead of a batch norm
    in training mode a bias has no gradient but rounding residue) and the input gradients at the bars.  Every figure is printed before
    the first assertion fails."""
    fwd, grad = _kinds(dtype)
    module.train(training)
    host = copy.deepcopy(module).double()
    ins = [t.to(dtype) for t in feats] + [edge.to(dtype)]
    ins64 = [t.double().requires_grad_() for t in ins]
    want = host(cpu, tuple(ins64[:-1]) if pair else ins64[0], ins64[-1])
    want = list(want) if isinstance(want, tuple) else [want]
    gen = torch.Generator().manual_seed(11)
    gos = [torch.randn(w.shape, generator=gen).to(dtype) for w in want]
    names = [n for n, _ in host.named_parameters()]
    want_grads = torch.autograd.grad(want, list(host.parameters()) + ins64, [g.double() for g in gos], allow_unused=True)

    module = module.to(DEV)
    ins_g = [t.to(DEV).requires_grad_() for t in ins]
    out = module(cpu.to(DEV), tuple(ins_g[:-1]) if pair else ins_g[0], ins_g[-1])
    out = list(out) if isinstance(out, tuple) else [out]
    assert all(o.dtype == dtype and o.is_cuda for o in out)
    got_grads = torch.autograd.grad(out, list(module.parameters()) + ins_g, [g.to(DEV) for g in gos], allow_unused=True)
    label = "%s %s " % (type(module).__name__, _ids(dtype))
    got = dict(zip(names + ["input%d" % i for i in range(len(ins))], got_grads))
    ref = dict(zip(names + ["input%d" % i for i in range(len(ins))], want_grads))
    missed = []

    def check(name, a, b, kind):
        try:
            _check(label + name, a, b, kind)
        except AssertionError as err:
            missed.append(str(err))

    for k, (o, w) in enumerate(zip(out, want)):
        check("out%d" % k, o, w, fwd)
    for name in got:
        assert (got[name] is None) == (ref[name] is None), name
        if ref[name] is None or (name.endswith(".bias") and "bn_" not in name):     # a Linear's bias goes with its weight
            continue
        a, b = got[name].flatten().cpu(), ref[name].flatten()
        if name.endswith(".weight") and name[:-6] + "bias" in got and "bn_" not in name:
            a, b = torch.cat([a, got[name[:-6] + "bias"].flatten().cpu()]), torch.cat([b, ref[name[:-6] + "bias"].flatten()])
        check("grad " + name, a, b, grad)
    if training and any(isinstance(m, torch.nn.BatchNorm1d) for m in module.modules()):
        for (name, x), (_, y) in zip(module.named_buffers(), host.named_buffers()):
            if name.endswith("running_mean") or name.endswith("running_var"):
                check(name, x, y, fwd)
    assert not missed, missed


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("widths", [(8, 8, 8), (8, 4, 8), (6, 5, 10)], ids=["residual", "no-residual", "F10"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_gatedgcnconv_against_its_host_path(dtype, widths, training):
    """a sampler block with a (src, dst) pair; output_feats = 10 is padded with zero weight rows and sliced"""
    from dgll_amd.nn.Convolution import GatedGCNConv

    cpu = _sampler_block()
    fin, fe, fout = widths
    gen = torch.Generator().manual_seed(fout + fe)
    h_src, h_dst = torch.randn(cpu.n_cols, fin, generator=gen), torch.randn(cpu.n_rows, fin, generator=gen)
    e = torch.randn(cpu.nnz, fe, generator=gen)
    torch.manual_seed(fout)
    layer = GatedGCNConv(fin, fe, fout, activation=_smooth(dtype))
    assert layer.residual == (widths == (8, 8, 8))
    _against_the_host_path(layer, cpu, [h_src, h_dst], e, dtype, training, pair=True)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_gatedgcn_model_against_its_host_path(dtype, training):
    from dgll_amd.nn.Convolution import GatedGCN

    cpu = _sampler_block(n_dst=150, n_src=150)
    gen = torch.Generator().manual_seed(8)
    x, attr = torch.randn(150, 8, generator=gen), torch.randn(cpu.nnz, 4, generator=gen)
    torch.manual_seed(8)
    _against_the_host_path(GatedGCN(8, 4, 16, 8, layers=2, activation=_smooth(dtype)), cpu, [x], attr, dtype, training)
