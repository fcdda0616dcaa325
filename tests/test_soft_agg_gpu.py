"""Soft aggregation on the GPU: dgll_amd.ops_softagg (the output, grad_x, grad_e and the scalar gradient of t / p; both modes, with
and without e) against the float64 per-entry restatement of softagg_ref.py, on the graphs and widths of test_soft_agg_emulated.py;
the memory condition (nothing of the size of the edge list is allocated); a captured step that follows t changed in place;
nn.GENConv and DeeperGCN against their own float64 host path on copied parameters.  For bf16 the reference runs on the bf16-rounded
inputs.

Bars: fp32 forward max |err| <= 1e-4 max |ref|, fp32 gradients <= 2e-3 max |ref|; bf16 forward <= 2e-2 max |ref|,
bf16 gradients relative L2 <= 1.5e-2; grad_t / grad_p: |err| <= 2e-3 (fp32) / 1.5e-2 (bf16) of the reference's sum |g * d out / d theta|.
No element is excluded (softagg_ref.py)."""
import copy
import itertools

import numpy as np
import pytest
import torch

import softagg_ref
from test_edge_feat_gpu import _sampler_block
from test_pna_emulated import _graph

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-7
FIVE, FIVE_COL = 4, 11      # the row of the full graph that lists one column five times, and that column
WIDTHS = [(4, torch.float32), (24, torch.float32), (260, torch.float32), (8, torch.bfloat16), (48, torch.bfloat16), (520, torch.bfloat16)]
MODES = [("softmax", 1.0), ("softmax", -0.5), ("softmax", 8.0), ("power", 0.5), ("power", 2.0)]
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


def _check_scalar(name, got, want, dtype):
    """grad_t / grad_p against the reference's value, on the scale sum |g * d out / d theta|"""
    got, bar = float(got), (2e-3 if dtype == torch.float32 else 1.5e-2) * want["scale"]
    print("%-34s %.6e  ref %.6e  |err| %.3e  bar %.3e" % (name, got, want["grad_theta"], abs(got - want["grad_theta"]), bar))
    assert np.isfinite(got) and abs(got - want["grad_theta"]) <= bar, (name, got, want["grad_theta"], bar)


def _kinds(dtype):
    return ("fwd32", "grad32") if dtype == torch.float32 else ("fwd16", "grad16")


def _inputs(graph, F, dtype, seed):
    """x, e and the output gradient, as stored"""
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, F, generator=gen).to(dtype) for n in (graph.n_cols, graph.nnz, graph.n_rows)]


def _case(F, dtype, mode, theta, with_e):
    """the graph, the inputs and the float64 reference of one case, computed once"""
    key = (F, dtype, mode, theta, with_e)
    if key not in _REF:
        if (F, dtype) not in _REF:
            cpu = _graph(full=F < 260)
            _REF[(F, dtype)] = (cpu, _inputs(cpu, F, dtype, F + 5))
        cpu, ins = _REF[(F, dtype)]
        _REF[key] = (cpu, ins, softagg_ref.reference(cpu.rowptr, cpu.col, ins[0], ins[1] if with_e else None, theta, ins[2], mode, EPS))
    return _REF[key]


def _op(graph, ins, mode, theta, with_e=True, needs=(True, True, True), go=None, semi=False):
    """the op and its backward on the GPU -> (out, [grad_x, grad_e, grad_theta]); theta: a float, made a tensor on the device"""
    from dgll_amd import ops_softagg

    x = ins[0].to(DEV).requires_grad_(needs[0])
    e = ins[1].to(DEV).requires_grad_(needs[1]) if with_e else None
    th = torch.tensor([theta], device=DEV, requires_grad=needs[2])
    if mode == "softmax":
        out = ops_softagg.softmax_aggregate(graph, x, e, th, semi, EPS)
    else:
        out = ops_softagg.powermean_aggregate(graph, x, e, th, EPS)
    if out.requires_grad:
        out.backward((ins[2] if go is None else go).to(DEV))
    return out.detach(), [x.grad, None if e is None else e.grad, th.grad]


def _against(name, cpu, ins, want, got, dtype, with_e):
    out, (gx, ge, gth) = got
    fwd, grad = _kinds(dtype)
    assert out.dtype == dtype and tuple(out.shape) == (cpu.n_rows, ins[0].shape[1])
    _check(name + " out", out, want["out"], fwd)
    _check(name + " grad_x", gx, want["grad_x"], grad)
    if with_e:
        _check(name + " grad_e", ge, want["grad_e"], grad)
    if want["grad_theta"] is not None:
        assert gth.shape == (1,) and gth.dtype == torch.float32
        _check_scalar(name + " grad_theta", gth, want, dtype)


@pytest.mark.parametrize("with_e", [False, True], ids=["noe", "e"])
@pytest.mark.parametrize("mode,theta", MODES)
@pytest.mark.parametrize("F,dtype", WIDTHS, ids=_ids)
def test_op_against_the_reference(F, dtype, mode, theta, with_e):
    cpu, ins, want = _case(F, dtype, mode, theta, with_e)
    got = _op(cpu.to(DEV), ins, mode, theta, with_e)
    _against(mode, cpu, ins, want, got, dtype, with_e)
    out, (gx, _, _) = got
    for r in (0, cpu.n_rows - 1):                                                   # rows without entries give exact zeros
        assert out[r].abs().max().item() == 0.0
    assert gx[-1].abs().max().item() == 0.0                                         # the source no row references


@pytest.mark.parametrize("mode,theta", [("softmax", 2.0), ("power", 1.5)])
@pytest.mark.parametrize("F,dtype", [(24, torch.float32), (48, torch.bfloat16)], ids=_ids)
def test_op_on_a_rectangular_sampler_block(F, dtype, mode, theta):
    cpu = _sampler_block()
    assert cpu.n_rows != cpu.n_cols
    ins = _inputs(cpu, F, dtype, 31)
    want = softagg_ref.reference(cpu.rowptr, cpu.col, ins[0], ins[1], theta, ins[2], mode, EPS)
    got = _op(cpu.to(DEV), ins, mode, theta)
    _against("block " + mode, cpu, ins, want, got, dtype, True)
    assert got[0][7].abs().max().item() == 0.0                                      # the block's empty row


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_semi_grad_and_a_float_t(dtype):
    """semi_grad: grad_x and grad_e without the t (m - out) term and no gradient for t; t as a Python float: the same bits as from
    a tensor"""
    from dgll_amd import ops_softagg

    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    ins = _inputs(cpu, 24 if dtype == torch.float32 else 48, dtype, 6)
    want = softagg_ref.reference(cpu.rowptr, cpu.col, ins[0], ins[1], 2.0, ins[2], "softmax", EPS, semi_grad=True)
    got = _op(graph, ins, "softmax", 2.0, semi=True)
    _against("semi_grad", cpu, ins, want, got, dtype, True)
    assert got[1][2] is None
    full = _op(graph, ins, "softmax", 2.0)
    assert torch.equal(full[0], got[0]) and not torch.equal(full[1][0], got[1][0])
    assert torch.equal(ops_softagg.softmax_aggregate(graph, ins[0].to(DEV), ins[1].to(DEV), 2.0, eps=EPS), full[0])
    assert torch.equal(ops_softagg.powermean_aggregate(graph, ins[0].to(DEV), None, 1.5, EPS), _op(graph, ins, "power", 1.5, with_e=False)[0])


@pytest.mark.parametrize("mode,theta", [("softmax", 2.0), ("power", 1.5)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_the_transposed_pass_reads_the_right_rows(dtype, mode, theta):
    """The graph is not symmetric and A^T's entry order differs from A's.  With the output gradient on the five-times row alone,
    grad_x is non-zero at that row's one column (whose features are positive: every gate is open) and exact zeros everywhere else,
    and grad_e is non-zero in that row's five entries alone."""
    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    gt, perm = graph.transpose()
    assert not torch.equal(perm.cpu(), torch.arange(cpu.nnz)) and gt.n_rows != graph.n_rows
    ins = _inputs(cpu, 8, dtype, 21)
    b = int(cpu.rowptr[FIVE])
    assert cpu.col[b:b + 5].tolist() == [FIVE_COL] * 5 and int(cpu.rowptr[FIVE + 1]) == b + 5
    ins[0][FIVE_COL] = ins[0][FIVE_COL].abs() + 4.0                                 # x + e > 0 in all five entries
    only = torch.zeros_like(ins[2])
    only[FIVE] = ins[2][FIVE]
    want = softagg_ref.reference(cpu.rowptr, cpu.col, ins[0], ins[1], theta, only, mode, EPS)
    got = _op(graph, ins, mode, theta, go=only)
    _against(mode, cpu, ins, want, got, dtype, True)
    gx, ge = got[1][0].cpu(), got[1][1].cpu()
    others = torch.ones(cpu.n_cols, dtype=torch.bool)
    others[FIVE_COL] = False
    assert gx[others].abs().max().item() == 0.0 and gx[FIVE_COL].abs().min().item() > 0.0
    slots = torch.zeros(cpu.nnz, dtype=torch.bool)
    slots[b:b + 5] = True
    assert ge[~slots].abs().max().item() == 0.0 and ge[slots].abs().min().item() > 0.0


@pytest.mark.parametrize("mode,theta", [("softmax", 2.0), ("power", 1.5)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_pitched_operands_with_nan_in_the_padding(dtype, mode, theta):
    """x, e and the output gradient on a pitch wider than F, NaN behind the row: the same bits as from compact operands, and (raw
    pass) the padding of a pitched grad_x is untouched"""
    from dgll_amd import _lib, ops_softagg

    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    F, vec = 24, 8 if dtype == torch.bfloat16 else 4
    ins = _inputs(cpu, F, dtype, 13)
    want_out, want_grads = _op(graph, ins, mode, theta)

    def pitched(t):
        buf = torch.full((t.shape[0], F + 2 * vec), float("nan"), dtype=dtype, device=DEV)
        buf[:, :F] = t.to(DEV)
        return buf[:, :F]

    wide = [pitched(t) for t in ins]
    assert all(t.stride(0) == F + 2 * vec for t in wide)
    x, e = wide[0].detach().requires_grad_(), wide[1].detach().requires_grad_()
    th = torch.tensor([theta], device=DEV, requires_grad=True)
    op = ops_softagg.softmax_aggregate if mode == "softmax" else ops_softagg.powermean_aggregate
    out = op(graph, x, e, th, eps=EPS)
    out.backward(wide[2])
    assert torch.equal(out.detach(), want_out)
    for got, ref in zip((x.grad, e.grad, th.grad), want_grads):
        assert torch.equal(got, ref)
    code = _lib.SOFT_AGG_SOFTMAX if mode == "softmax" else _lib.SOFT_AGG_POWER
    out, stats = ops_softagg.forward_raw(graph, code, wide[0], wide[1], th.detach(), EPS)
    assert torch.equal(out, want_out)
    gx_buf = torch.full((cpu.n_cols, F + 2 * vec), 7.0, dtype=dtype, device=DEV)
    gt, perm = graph.transpose()
    ops_softagg._launch(_lib.SOFT_AGG_COLS, code, gt, wide[0], th.detach(), EPS, perm=perm, nnz=graph.nnz, x=wide[0], e=wide[1], stats=stats,
                        grad_out=wide[2], grad_x=gx_buf[:, :F])
    assert torch.equal(gx_buf[:, :F], want_grads[0]) and bool((gx_buf[:, F:] == 7.0).all())


@pytest.mark.parametrize("mode,theta", [("softmax", 2.0), ("power", 1.5)])
def test_only_the_wanted_gradients_are_computed_and_reruns_give_the_same_bits(mode, theta):
    from dgll_amd import ops

    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    ins = _inputs(cpu, 24, torch.float32, 9)
    full = _op(graph, ins, mode, theta)
    again = _op(graph, ins, mode, theta)
    assert torch.equal(full[0], again[0])                                           # no atomics: identical bits, grad_theta included
    assert all(torch.equal(a, b) for a, b in zip(full[1], again[1]))
    for with_e in (True, False):
        ref = full if with_e else _op(graph, ins, mode, theta, with_e=False)
        for needs in itertools.product((True, False), repeat=3):                    # (x, e, theta)
            if not with_e and needs[1]:
                continue
            with ops.LaunchTimer() as timer:
                out, grads = _op(graph, ins, mode, theta, with_e=with_e, needs=needs)
            tags = [tag[0] for tag, _, _ in timer.records]
            assert tags.count("soft_agg_forward") == 1
            assert tags.count("soft_agg_rows") == (1 if needs[1] or needs[2] else 0), (needs, tags)      # only for e or the scalar
            assert tags.count("soft_agg_cols") == (1 if needs[0] else 0), (needs, tags)
            assert torch.equal(out, ref[0])
            for k, (need, got, want) in enumerate(zip(needs, grads, ref[1])):
                assert (got is None) == (not need or (k == 1 and not with_e)), (needs, k)
                if got is not None:
                    assert torch.equal(got, want), (needs, k)


def test_the_op_replays_from_a_captured_graph_and_follows_t():
    """one capture; t is changed IN PLACE between the replays and the replayed output and gradients are those of the new t: the value
    reaches the kernels through its address, the host never reads it"""
    from dgll_amd import ops_softagg

    cpu = _graph(full=True)
    graph = cpu.to(DEV)
    graph.transpose()                                                               # the cached structure, built outside the capture
    ins = [t.to(DEV) for t in _inputs(cpu, 24, torch.float32, 3)]
    x, e = ins[0].requires_grad_(), ins[1].requires_grad_()
    t = torch.ones(1, device=DEV, requires_grad=True)

    def step():
        out = ops_softagg.softmax_aggregate(graph, x, e, t, eps=EPS)
        return (out.detach(),) + tuple(torch.autograd.grad(out, (x, e, t), ins[2]))

    eager = {}
    for value in (1.0, 3.0, -0.5):
        with torch.no_grad():
            t.fill_(value)
        eager[value] = [v.clone() for v in step()]
    assert not torch.equal(eager[1.0][0], eager[3.0][0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured, stream=side):
        static = step()
    for value in (3.0, -0.5, 1.0):
        with torch.no_grad():
            t.fill_(value)
        for v in static:
            v.zero_()
        captured.replay()
        torch.cuda.synchronize()
        for name, got, ref in zip(("out", "grad_x", "grad_e", "grad_t"), static, eager[value]):
            assert torch.equal(got, ref), (value, name)


def test_empty_graphs_give_zeros_with_zero_gradients():
    from dgll_amd import CSRGraph, ops_softagg

    for n_dst, op in ((3, ops_softagg.softmax_aggregate), (3, ops_softagg.powermean_aggregate), (0, ops_softagg.softmax_aggregate)):
        g = CSRGraph(torch.zeros(n_dst + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None, n_dst, 5).to(DEV)
        x = torch.randn(5, 8, device=DEV, requires_grad=True)
        e = torch.randn(0, 8, device=DEV, requires_grad=True)
        th = torch.ones(1, device=DEV, requires_grad=True)
        out = op(g, x, e, th)
        assert tuple(out.shape) == (n_dst, 8) and (n_dst == 0 or out.abs().max().item() == 0.0)
        out.sum().backward()
        assert all(t.grad.shape == t.shape and (t.numel() == 0 or t.grad.abs().max().item() == 0.0) for t in (x, e, th))


def test_nothing_of_the_size_of_the_edge_list_is_allocated():
    """n_dst = n_src = 1024, 64 entries a row (nnz = 2^16), F = 64 fp32, no e, a learned t: one [nnz, F] array would be 16 MiB.  The
    peak of a forward and backward above what is allocated before them stays below a quarter of that (4 MiB): by count, out, the output
    gradient as passed on and grad_x (256 KiB each), the statistics (512 KiB) and the partials come to about 2 MiB with the allocator's
    rounding.  A condition, not a measurement.  The same for the power mean."""
    from dgll_amd import CSRGraph, ops_softagg

    n, deg, F = 1024, 64, 64
    rng = np.random.RandomState(5)
    col = torch.from_numpy(np.concatenate([rng.choice(n, deg, replace=False) for _ in range(n)]).astype(np.int32))
    graph = CSRGraph(torch.arange(n + 1, dtype=torch.int64) * deg, col, None, n, n).to(DEV)
    nnz = graph.nnz
    assert nnz == 2 ** 16
    graph.transpose()                                                               # the transposed structure is built beforehand
    gen = torch.Generator().manual_seed(5)
    x0, go = (torch.randn(n, F, generator=gen).to(DEV) for _ in range(2))
    bound = nnz * F * 4 // 4

    def peak(op):
        x, t = x0.clone().requires_grad_(), torch.ones(1, device=DEV, requires_grad=True)
        op(graph, x, None, t).backward(go)                                          # once outside the measurement: lazy initialisation
        x.grad = t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        op(graph, x, None, t).backward(go)
        torch.cuda.synchronize()
        assert x.grad is not None and t.grad is not None
        return torch.cuda.max_memory_allocated() - before

    for name, op in (("softmax_aggregate", ops_softagg.softmax_aggregate), ("powermean_aggregate", ops_softagg.powermean_aggregate)):
        used = peak(op)
        print("%s peak above the inputs %d bytes (%.2f MiB), bound %d" % (name, used, used / 2 ** 20, bound))
        assert used < bound, (name, used, bound)


# ---- the layer and the model against their host path ----------------------------------------------------------------------------------

def _against_the_host_path(module, cpu, feats, edge, dtype, training, pair=False):
    """module(graph, feats, edge) on the GPU in `dtype` (fp32 parameters) against a float64 copy on the host with the inputs as stored:
    the output, the parameter gradients (weight and bias of a Linear, one affine map, as one vector: ahead of a norm a bias has no
    gradient but rounding residue) and the input gradients at the bars.  A learned t / p is judged as the op's own: |err| against the
    bar's fraction of sum |g * d agg / d theta| over the aggregation's outputs.  d agg / d theta is >= 0 element by element in both
    modes (the softmax-weighted variance of the messages; the power mean rises with p), so that sum is the gradient theta gets when
    |g| is fed into the aggregation's output, which the host path gives.  Every figure is printed before the first assertion fails."""
    from dgll_amd.nn.Convolution.genconv import SoftAggregation

    fwd, grad = _kinds(dtype)
    module.train(training)
    host = copy.deepcopy(module).double()
    aggs = {}                                                                       # parameter name -> [module, its output]
    for prefix, mod in host.named_modules():
        if isinstance(mod, SoftAggregation) and mod.learn:
            aggs[prefix + "." + mod.name] = [mod, None]
            mod.register_forward_hook(lambda m, args, out, key=prefix + "." + mod.name: aggs[key].__setitem__(1, out))
    ins = [t.to(dtype) for t in feats] + ([edge.to(dtype)] if edge is not None else [])
    ins64 = [t.double().requires_grad_() for t in ins]
    n = len(feats)
    call = lambda m, g, xs: m(g, tuple(xs[:n]) if pair else xs[0], xs[n] if edge is not None else None)      # noqa: E731
    want = call(host, cpu, ins64)
    go = torch.randn(want.shape, generator=torch.Generator().manual_seed(11)).to(dtype)
    trained = lambda m: [(k, p) for k, p in m.named_parameters() if p.requires_grad]        # noqa: E731
    names = [k for k, _ in trained(host)] + ["input%d" % i for i in range(len(ins))]
    scales = {}
    for key, (mod, agg) in aggs.items():
        g_agg = torch.autograd.grad(want, agg, go.double(), retain_graph=True)[0]
        scales[key] = torch.autograd.grad(agg, getattr(mod, mod.name), g_agg.abs(), retain_graph=True)[0].item()
    ref = dict(zip(names, torch.autograd.grad(want, [p for _, p in trained(host)] + ins64, go.double())))

    module = module.to(DEV)
    ins_g = [t.to(DEV).requires_grad_() for t in ins]
    out = call(module, cpu.to(DEV), ins_g)
    assert out.dtype == dtype and out.is_cuda and out.shape == want.shape
    got = dict(zip(names, torch.autograd.grad(out, [p for _, p in trained(module)] + ins_g, go.to(DEV))))
    label = "%s %s " % (type(module).__name__, _ids(dtype))
    missed = []

    def check(name, a, b, kind):
        try:
            _check(label + name, a, b, kind)
        except AssertionError as err:
            missed.append(str(err))

    check("out", out, want, fwd)
    for name in names:
        if name.endswith(".bias") and name[:-4] + "weight" in got:                  # a bias goes with its weight
            continue
        if name in scales:
            try:
                _check_scalar(label + "grad " + name, got[name].item(), {"grad_theta": ref[name].item(), "scale": scales[name]}, dtype)
            except AssertionError as err:
                missed.append(str(err))
            continue
        a, b = got[name].flatten().cpu(), ref[name].flatten()
        if name.endswith(".weight") and name[:-6] + "bias" in got:
            a, b = torch.cat([a, got[name[:-6] + "bias"].flatten().cpu()]), torch.cat([b, ref[name[:-6] + "bias"].flatten()])
        check("grad " + name, a, b, grad)
    assert not missed, missed


def _mlp_layers(dtype):
    """Linears of a GENConv's MLP in the layer comparisons: 2 for fp32.  For bf16 ONE, so that no norm + ReLU follows a bf16-rounded
    activation: the relu's gate would be the sign of a norm output formed from bf16-rounded values on the GPU and from exact ones in
    the float64 host path, and the elements within that error of 0 open on one side and stay shut on the other, whatever the kernels
    do (test_gated_gpu._smooth has the arithmetic).  The relu of the MESSAGE is not affected: its gate is the sign of a stored value,
    and rounding to bf16 keeps the sign."""
    return 2 if dtype == torch.float32 else 1


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("kw", [dict(aggr="softmax", learn_t=True, norm="batch", edge_dim=3, bias=True),
                                dict(aggr="power", p=2.0, learn_p=True, msg_norm=True, learn_msg_scale=True, norm="layer"),
                                dict(aggr="softmax_sg", t=0.5, msg_norm=True, norm=None, edge_dim=10)],
                         ids=["softmax-learn_t-edge3", "power-learn_p-msgnorm", "softmax_sg-edge10"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_genconv_against_its_host_path(dtype, kw, training):
    """a sampler block with a (src, dst) pair of different widths; out_channels = 10 is padded with zero columns and sliced.

    bf16 with edge attributes: the source width and edge_dim are 10, so that x_j and e_k are the STORED inputs and no lin_src / lin_edge
    stands before the message.  With both projections the gate is the sign of the sum of two separately bf16-rounded projections, in
    the float64 host path that of the exact sum: the elements with |x_j + e_k| below 2^-9 of its terms open on one side only and put
    their full size into every gradient that passes the gate -- measured with (6, 5) -> 10 and edge_dim = 3: relative L2 2.0e-2 in
    grad lin_src.weight, 1.8e-2 in grad lin_edge.weight, 2.8e-2 in the gradient of edge_attr, the others at 3e-3.
    A property of the number format, not of the kernels: one projection alone keeps its sign when rounded, and fp32 runs both."""
    from dgll_amd.nn.Convolution import GENConv

    cpu = _sampler_block()
    gen = torch.Generator().manual_seed(10)
    src = 6
    if dtype == torch.bfloat16 and "edge_dim" in kw:
        src, kw = 10, dict(kw, edge_dim=10)
    x_src, x_dst = torch.randn(cpu.n_cols, src, generator=gen), torch.randn(cpu.n_rows, 5, generator=gen)
    edge = torch.randn(cpu.nnz, kw["edge_dim"], generator=gen) if "edge_dim" in kw else None
    torch.manual_seed(10)
    layer = GENConv((src, 5), 10, num_layers=_mlp_layers(dtype), **kw)
    _against_the_host_path(layer, cpu, [x_src, x_dst], edge, dtype, training, pair=True)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("aggr", ["softmax", "power"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
def test_deepergcn_model_against_its_host_path(dtype, aggr, training):
    """2 layers, hidden 16.  relu and two-Linear MLPs for fp32; for bf16 one-Linear MLPs (_mlp_layers) and softplus between the layers:
    the next layer's message relu(h_j) would otherwise take its gate from the sign of a norm output rounded to bf16
    (test_gated_gpu._smooth).  For bf16 the encoder's bias is also raised by 4, which keeps its output positive: the dense path multiplies
    bf16 activations by weights rounded to bf16, the host path by the fp32 weights, so the first layer's gates -- the sign of the encoder's
    output -- differ for the elements within 2^-9 of their terms of 0, and each puts its full size into the gradients ahead of the gate:
    measured without the shift, relative L2 2.1e-2 in grad encoder.weight and 2.0e-2 in the input gradient, everything behind the gate
    at 2e-3 to 7e-3.  The gates themselves are held bit for bit by the op's tests above, where nothing is excluded."""
    from dgll_amd.nn.Convolution import DeeperGCN

    cpu = _sampler_block(n_dst=150, n_src=150)
    x = torch.randn(150, 8, generator=torch.Generator().manual_seed(8))
    torch.manual_seed(8)
    act = torch.nn.functional.relu if dtype == torch.float32 else torch.nn.functional.softplus
    model = DeeperGCN(8, 16, 8, 2, aggr=aggr, learn_t=True, learn_p=True, p=1.5, mlp_layers=_mlp_layers(dtype), activation=act)
    if dtype == torch.bfloat16:
        with torch.no_grad():
            model.encoder.bias += 4.0
    _against_the_host_path(model, cpu, [x], None, dtype, training)
