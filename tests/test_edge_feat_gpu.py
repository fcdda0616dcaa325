"""Edge-feature aggregation on the GPU: dgll_amd.ops_ef.u_op_e_sum (forward and both gradients, three ops, sum and mean) against the
float64 per-edge restatement of ef_ref.py, on the graphs and widths of test_edge_feat_emulated.py; nn.GINEConv, GINE and CFConv
against their own host path on the same parameters.  For bf16 the reference runs on the bf16-rounded inputs.

Bars: fp32 forward max |err| <= 1e-4 max |ref|, fp32 gradients <= 2e-3 max |ref|; bf16 forward <= 2e-2 max |ref|,
bf16 gradients relative L2 <= 1.5e-2.  No element is excluded (ef_ref.py says why the gates agree)."""
import copy

import numpy as np
import pytest
import torch

import ef_ref
from test_pna_emulated import _graph

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIVE, FIVE_COL = 4, 11      # the row of the full graph that lists one column five times, and that column
WIDTHS = [(4, torch.float32), (24, torch.float32), (260, torch.float32), (8, torch.bfloat16), (48, torch.bfloat16), (520, torch.bfloat16)]
_ids = lambda v: str(v).replace("torch.", "")       # noqa: E731


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
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(graph.n_cols, F, generator=gen).to(dtype), torch.randn(graph.nnz, F, generator=gen).to(dtype),
            torch.randn(graph.n_rows, F, generator=gen).to(dtype))


def _op_act(op):
    return ("add", "relu") if op == "add_relu" else (op, None)


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("op", ef_ref.OPS)
@pytest.mark.parametrize("F,dtype", WIDTHS, ids=_ids)
def test_op_against_the_reference(F, dtype, op, reduce):
    from dgll_amd import ops_ef

    cpu = _graph(full=F < 260)
    graph = cpu.to(DEV)
    fwd, grad = _kinds(dtype)
    x, e, go = _inputs(cpu, F, dtype, F + 3)
    xg, eg = x.to(DEV).requires_grad_(), e.to(DEV).requires_grad_()
    out = ops_ef.u_op_e_sum(graph, xg, eg, *_op_act(op), reduce=reduce)
    assert out.dtype == dtype and tuple(out.shape) == (cpu.n_rows, F)
    gx, ge = torch.autograd.grad(out, (xg, eg), go.to(DEV))
    want_gx, want_ge = ef_ref.gradients(cpu.rowptr, cpu.col, x.double(), e.double(), go.double(), op, reduce)
    name = "%s/%s " % (op, reduce)
    _check(name + "out", out, ef_ref.forward(cpu.rowptr, cpu.col, x.double(), e.double(), op, reduce), fwd)
    _check(name + "grad_x", gx, want_gx, grad)
    _check(name + "grad_e", ge, want_ge, grad)
    assert gx.dtype == dtype and ge.dtype == dtype
    # rows without entries give zeros; the source no row references gets no gradient
    assert out[0].abs().max().item() == 0.0 and out[-1].abs().max().item() == 0.0 and gx[-1].abs().max().item() == 0.0
    if op == "add_relu":            # the gates are the reference's, element for element: a closed gate writes an exact 0
        assert torch.equal(ge.cpu() != 0, want_ge != 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_the_transposed_pass_reads_each_duplicates_own_edge_row(dtype):
    """The graph is not symmetric and A^T's entry order differs from A's.  With the output gradient on the five-times row alone,
    grad_x of its column is that gradient times the sum of exactly those five e rows (mul) / the count of their open gates (add_relu)."""
    from dgll_amd import ops_ef

    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    gt, perm = graph.transpose()
    assert not torch.equal(perm.cpu(), torch.arange(cpu.nnz)) and gt.n_rows != graph.n_rows
    F = 8
    x, e, go = _inputs(cpu, F, dtype, 21)
    b = int(cpu.rowptr[FIVE])
    assert cpu.col[b:b + 5].tolist() == [FIVE_COL] * 5 and int(cpu.rowptr[FIVE + 1]) == b + 5
    assert len({tuple(r) for r in e[b:b + 5].tolist()}) == 5                         # five different e rows
    only = torch.zeros_like(go)
    only[FIVE] = go[FIVE]
    for op in ("mul", "add_relu"):
        xg = x.to(DEV).requires_grad_()
        out = ops_ef.u_op_e_sum(graph, xg, e.to(DEV), *_op_act(op))
        (gx,) = torch.autograd.grad(out, xg, only.to(DEV))
        dm = e[b:b + 5].double() if op == "mul" else (x[FIVE_COL].double() + e[b:b + 5].double() > 0).double()
        want = torch.zeros(cpu.n_cols, F, dtype=torch.float64)
        want[FIVE_COL] = go[FIVE].double() * dm.sum(0)
        _check("five-times column " + op, gx, want, _kinds(dtype)[1])
        others = torch.ones(cpu.n_cols, dtype=torch.bool)
        others[FIVE_COL] = False
        assert gx.cpu()[others].abs().max().item() == 0.0


@pytest.mark.parametrize("op", ef_ref.OPS)
def test_only_the_wanted_gradient_is_computed_and_reruns_give_the_same_bits(op):
    from dgll_amd import ops_ef

    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    x, e, go = _inputs(cpu, 24, torch.float32, 9)
    go = go.to(DEV)

    def run(need_x, need_e):
        xg, eg = x.to(DEV).requires_grad_(need_x), e.to(DEV).requires_grad_(need_e)
        out = ops_ef.u_op_e_sum(graph, xg, eg, *_op_act(op), reduce="mean")
        out.backward(go)
        return out.detach(), xg.grad, eg.grad

    out, gx, ge = run(True, True)
    out2, gx2, ge2 = run(True, True)
    assert torch.equal(out, out2) and torch.equal(gx, gx2) and torch.equal(ge, ge2)  # no atomics: identical bits
    out_x, gx_x, none_e = run(True, False)
    out_e, none_x, ge_e = run(False, True)
    assert none_e is None and none_x is None
    assert torch.equal(out_x, out) and torch.equal(out_e, out) and torch.equal(gx_x, gx) and torch.equal(ge_e, ge)


def test_empty_graphs_give_zeros_with_zero_gradients():
    from dgll_amd import CSRGraph, ops_ef

    g = CSRGraph(torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None, 3, 5).to(DEV)
    x = torch.randn(5, 8, device=DEV, requires_grad=True)
    e = torch.randn(0, 8, device=DEV, requires_grad=True)
    out = ops_ef.u_op_e_sum(g, x, e, "mul")
    assert tuple(out.shape) == (3, 8) and out.abs().max().item() == 0.0
    out.sum().backward()
    assert x.grad.abs().max().item() == 0.0 and tuple(e.grad.shape) == (0, 8)


def _sampler_block(n_dst=40, n_src=150, fanout=5, seed=4):
    """A block as NeighborSampler shapes it: the destinations are the first n_dst sources, up to `fanout` entries a row, one empty row."""
    from dgll_amd import CSRGraph

    rng = np.random.RandomState(seed)
    rows = [list(rng.randint(0, n_src, rng.randint(1, fanout + 1))) for _ in range(n_dst)]
    rows[7] = []
    rowptr = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
    return CSRGraph(rowptr, torch.tensor([int(c) for r in rows for c in r], dtype=torch.int32), None, n_dst, n_src)


def _layer_against_its_host_path(layer, cpu, feats, edge, go, dtype, pair=False):
    """layer(graph, feats, edge) on the GPU in `dtype` (fp32 parameters) against a float64 copy of the layer on the host with the
    inputs as stored: forward, parameter gradients and input gradients at the bars."""
    fwd, grad = _kinds(dtype)
    host = copy.deepcopy(layer).double()
    ins = [t.to(dtype) for t in feats] + [edge.to(dtype)]
    ins64 = [t.double().requires_grad_() for t in ins]
    want = host(cpu, tuple(ins64[:-1]) if pair else ins64[0], ins64[-1])
    names = [n for n, _ in host.named_parameters()]
    want_grads = torch.autograd.grad(want, list(host.parameters()) + ins64, go.to(dtype).double())

    layer = layer.to(DEV)
    ins_g = [t.to(DEV).requires_grad_() for t in ins]
    out = layer(cpu.to(DEV), tuple(ins_g[:-1]) if pair else ins_g[0], ins_g[-1])
    assert out.dtype == dtype and out.is_cuda
    got = torch.autograd.grad(out, list(layer.parameters()) + ins_g, go.to(dtype).to(DEV))
    label = "%s %s " % (type(layer).__name__, _ids(dtype))
    _check(label + "out", out, want, fwd)
    for name, a, b in zip(names + ["input%d" % i for i in range(len(ins))], got, want_grads):
        _check(label + "grad " + name, a, b, grad)


@pytest.mark.parametrize("width", [8, 6], ids=["F8", "F6"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_gineconv_on_a_sampler_block_with_a_src_dst_pair(dtype, width):
    """rectangular, (src, dst) features, a learned eps; width 6 is padded with zero columns and sliced"""
    from dgll_amd.nn.Convolution import GINEConv

    cpu = _sampler_block()
    gen = torch.Generator().manual_seed(width)
    h_src, h_dst = torch.randn(cpu.n_cols, width, generator=gen), torch.randn(cpu.n_rows, width, generator=gen)
    e, go = torch.randn(cpu.nnz, width, generator=gen), torch.randn(cpu.n_rows, width, generator=gen)
    _layer_against_its_host_path(GINEConv(None, 0.2, learn_eps=True), cpu, [h_src, h_dst], e, go, dtype, pair=True)


def test_gineconv_with_an_apply_func_on_the_full_graph():
    from dgll_amd.nn.Convolution import GINEConv

    cpu = _graph(full=True)
    gen = torch.Generator().manual_seed(1)
    h_src, h_dst = torch.randn(cpu.n_cols, 12, generator=gen), torch.randn(cpu.n_rows, 12, generator=gen)
    e, go = torch.randn(cpu.nnz, 12, generator=gen), torch.randn(cpu.n_rows, 5, generator=gen)
    torch.manual_seed(3)
    _layer_against_its_host_path(GINEConv(torch.nn.Linear(12, 5), 0.1, learn_eps=True), cpu, [h_src, h_dst], e, go, torch.float32, pair=True)


@pytest.mark.parametrize("hidden", [16, 6], ids=["H16", "H6"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_cfconv_against_its_host_path(dtype, hidden):
    """bf16: bf16 activations with fp32 parameters; hidden = 6 is padded with zero columns and sliced"""
    from dgll_amd.nn.Convolution import CFConv

    cpu = _sampler_block(n_dst=150, n_src=150)
    gen = torch.Generator().manual_seed(hidden)
    h, a, go = torch.randn(150, 8, generator=gen), torch.randn(cpu.nnz, 8, generator=gen), torch.randn(150, 8, generator=gen)
    torch.manual_seed(hidden)
    _layer_against_its_host_path(CFConv(8, 8, hidden, 8), cpu, [h], a, go, dtype)


def test_gine_model_against_its_host_path():
    from dgll_amd.nn.Convolution import GINE

    cpu = _sampler_block(n_dst=150, n_src=150)
    gen = torch.Generator().manual_seed(8)
    x, attr, go = torch.randn(150, 8, generator=gen), torch.randn(cpu.nnz, 4, generator=gen), torch.randn(150, 8, generator=gen)
    torch.manual_seed(8)
    _layer_against_its_host_path(GINE(8, 4, 16, 8, n_layers=2), cpu, [x], attr, go, torch.float32)
