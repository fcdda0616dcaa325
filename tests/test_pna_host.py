"""PNA without a GPU: the binding of dgll_multi_agg_desc, the host-side argument checks of dgll_hip_multi_agg_pass, the refusals of
dgll_amd.ops_agg (shapes, names and dtypes first, then that the tensors are on the GPU, so both are checked here), and nn.PNAConv:
names and shapes, its refusals, and its host path -- the decomposition-free check of the layer's algebra -- against the float64
per-edge restatement of pna_ref.py, forward and parameter gradients at 1e-9 max |ref|."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pna_ref
from conftest import ROOT

INVALID = -1        # DGLL_ERR_INVALID


def _graph(rows, n_src):
    """CSRGraph from a list of per-row column lists (kept as given: duplicates stay separate entries)."""
    from dgll_amd import CSRGraph

    rowptr = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
    col = torch.tensor([int(c) for r in rows for c in r], dtype=torch.int32)
    return CSRGraph(rowptr, col, None, len(rows), n_src)


_SQUARE = [[0, 1, 4], [1], [], [0, 0, 2, 3, 5], [4, 5], [5, 1, 1]]      # row 2 is empty; rows 3 and 5 repeat a column


def _block():
    """9 destinations, 12 sources: an empty row, a row listing one source alone three times, the last two sources never referenced."""
    rng = np.random.RandomState(3)
    rows = [list(rng.randint(0, 10, rng.randint(1, 6))) for _ in range(9)]
    rows[4] = []
    rows[6] = [3, 3, 3]
    return _graph(rows, 12)


# ---- the C entry point -----------------------------------------------------------------------------------------------------------

def test_descriptor_binding_matches_the_c_struct(tmp_path):
    """_lib.MultiAggDesc field by field against offsetof / sizeof of dgll_multi_agg_desc as a C compiler lays it out."""
    import subprocess

    from dgll_amd import _lib

    fields = [name for name, _ in _lib.MultiAggDesc._fields_]
    c_names = ["pass" if f == "pass_" else f for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dgll_hip.h"\nint main(void) {\n'
                   + "".join('    printf("%%zu\\n", offsetof(dgll_multi_agg_desc, %s));\n' % n for n in c_names)
                   + '    printf("%zu\\n", sizeof(dgll_multi_agg_desc));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [getattr(_lib.MultiAggDesc, f).offset for f in fields] + [ctypes.sizeof(_lib.MultiAggDesc)]


def test_constants_match_the_header():
    from dgll_amd import _lib, ops_agg

    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    assert int(re.search(r"#define\s+DGLL_MAGG_LONG_ROW\s+(\d+)", text).group(1)) == ops_agg.LONG_ROW == _lib.MAGG_LONG_ROW == 256
    for name in ("FORWARD", "ROWS", "COLS", "MEAN", "SUM", "MAX", "MIN", "VAR", "STD", "IDENTITY", "AMPLIFICATION", "ATTENUATION"):
        assert int(re.search(r"DGLL_MAGG_%s\s*=\s*(\d+)" % name, text).group(1)) == getattr(_lib, "MAGG_" + name)
    assert list(ops_agg.AGGREGATORS) == list(pna_ref.AGGREGATORS) and list(ops_agg.SCALERS) == list(pna_ref.SCALERS)
    assert _lib.lib.dgll_hip_abi_version() == 2                                     # an addition: the ABI version stays


def _valid(kind):
    """A descriptor that passes every check of `kind` (the pointers are only inspected, never followed, before the checks pass)."""
    from dgll_amd import _lib

    buf = (ctypes.c_float * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    d = _lib.MultiAggDesc()
    d._keep = buf
    d.pass_, d.dtype, d.F, d.n_rows, d.n_cols, d.delta = kind, _lib.F32, 8, 0, 4, 1.5
    d.n_agg, d.n_scaler = 4, 3
    for i, c in enumerate((_lib.MAGG_MEAN, _lib.MAGG_MAX, _lib.MAGG_MIN, _lib.MAGG_STD)):
        d.agg[i] = c
    for i in range(3):
        d.scaler[i] = i
    d.rowptr = d.col = d.x = d.y = d.out = d.grad_out = d.stats = d.arg = d.coef = d.grad_y = d.grad_x = base
    d.ld_x = d.ld_y = d.ld_grad_y = d.ld_grad_x = 8
    d.ld_out = d.ld_grad_out = 96
    d.ld_stats = d.ld_arg = 16
    d.ld_coef = 40
    return d


def _refused(d, word):
    from dgll_amd import _lib

    code = _lib.lib.dgll_hip_multi_agg_pass(None, ctypes.byref(d))
    msg = _lib.last_error()
    assert code == INVALID and word in msg, (code, word, msg)


def test_pass_arguments_are_checked_on_the_host():
    from dgll_amd import _lib

    fn = _lib.lib.dgll_hip_multi_agg_pass
    assert fn(None, None) == INVALID and "NULL" in _lib.last_error()                # a NULL descriptor
    for kind in range(3):                                                           # n_rows == 0: nothing to do, and nothing launched
        assert fn(None, ctypes.byref(_valid(kind))) == _lib.OK, (kind, _lib.last_error())
    for bad in (-1, 3):
        d = _valid(0)
        d.pass_ = bad
        _refused(d, "pass")
    for kind in range(3):
        d = _valid(kind)
        d.n_rows, d.rowptr = 4, None                                                # (every refusal also holds with rows to sweep)
        _refused(d, "rowptr")
        d = _valid(kind)
        d.n_rows, d.dtype = 4, 7
        _refused(d, "dtype")
        d = _valid(kind)
        d.n_rows, d.F = 4, 6
        _refused(d, "F a positive multiple")                                        # no whole number of vectors (4 fp32 columns)
        d.dtype, d.F = _lib.BF16, 12
        _refused(d, "F a positive multiple")                                        # ... (8 bf16 columns)
        d = _valid(kind)
        d.n_rows, d.n_agg = 4, 7
        _refused(d, "n_agg")
        d = _valid(kind)
        d.n_rows, d.n_scaler = 4, 0
        _refused(d, "n_scaler")
        d = _valid(kind)
        d.n_rows = 4
        d.agg[2] = _lib.MAGG_MEAN
        _refused(d, "agg: an aggregator code is repeated")
        d.agg[2] = 6
        _refused(d, "agg: unknown")
        d = _valid(kind)
        d.n_rows = 4
        d.scaler[1] = 0
        _refused(d, "scaler: a scaler code is repeated")
        d.scaler[1] = 3
        _refused(d, "scaler: unknown")
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            d = _valid(kind)
            d.n_rows, d.delta = 4, bad
            _refused(d, "delta")
    for kind in (_lib.MAGG_FORWARD, _lib.MAGG_COLS):
        d = _valid(kind)
        d.n_rows, d.col = 4, None
        _refused(d, "col")
        d = _valid(kind)
        d.n_rows, d.x = 4, None
        _refused(d, "x non-NULL")
        d = _valid(kind)
        d.n_rows, d.ld_x = 4, 10
        _refused(d, "pitch")
        d.ld_x, d.x = 8, d.x + 4
        _refused(d, "aligned")
    d = _valid(_lib.MAGG_FORWARD)
    d.n_rows, d.ld_out = 4, 88                                                      # narrower than n_scaler * n_agg * F
    _refused(d, "out non-NULL")
    d = _valid(_lib.MAGG_FORWARD)
    d.n_rows, d.ld_stats = 4, 8
    _refused(d, "stats")
    d = _valid(_lib.MAGG_FORWARD)
    d.y = d.stats = d.arg = None                                                    # all three are optional
    assert fn(None, ctypes.byref(d)) == _lib.OK
    d = _valid(_lib.MAGG_ROWS)
    d.n_rows, d.stats = 4, None                                                     # STD is asked: the rows pass needs the variance
    _refused(d, "stats must be non-NULL")
    d = _valid(_lib.MAGG_ROWS)
    d.n_rows, d.grad_out = 4, None
    _refused(d, "grad_out non-NULL")
    d = _valid(_lib.MAGG_ROWS)
    d.n_rows, d.coef, d.grad_y = 4, None, None
    _refused(d, "coef and grad_y")
    d = _valid(_lib.MAGG_ROWS)
    d.n_rows, d.ld_coef = 4, 32
    _refused(d, "coef")
    d = _valid(_lib.MAGG_COLS)
    d.n_rows, d.arg = 4, None                                                       # MAX / MIN are asked
    _refused(d, "arg non-NULL")
    d = _valid(_lib.MAGG_COLS)
    d.n_rows, d.coef = 4, None
    _refused(d, "coef non-NULL")
    d = _valid(_lib.MAGG_COLS)
    d.n_rows, d.grad_x = 4, None
    _refused(d, "grad_x non-NULL")


# ---- the wrapper's refusals -----------------------------------------------------------------------------------------------------------

def test_multi_aggregate_argument_errors():
    from dgll_amd import ops_agg

    g = _graph(_SQUARE, 6)
    x = torch.ones(6, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops_agg.multi_aggregate(g, x)
    with pytest.raises(RuntimeError, match="GPU"):
        ops_agg.multi_aggregate(g, x, x, ("std", "min"), ("attenuation",), 2.0)
    with pytest.raises(TypeError, match="CSRGraph"):
        ops_agg.multi_aggregate(torch.eye(6).to_sparse(), x)
    with pytest.raises(ValueError, match="pad"):
        ops_agg.multi_aggregate(g, torch.ones(6, 6))
    with pytest.raises(ValueError, match="pad"):
        ops_agg.multi_aggregate(g, torch.ones(6, 12, dtype=torch.bfloat16))
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        ops_agg.multi_aggregate(g, x.double())
    with pytest.raises(ValueError, match="6 rows"):
        ops_agg.multi_aggregate(g, torch.ones(5, 8))
    with pytest.raises(ValueError, match="one dtype and width"):
        ops_agg.multi_aggregate(g, x, torch.ones(6, 4))
    with pytest.raises(ValueError, match="unknown aggregator"):
        ops_agg.multi_aggregate(g, x, aggregators=("mean", "median"))
    with pytest.raises(ValueError, match="unknown scaler"):
        ops_agg.multi_aggregate(g, x, scalers=("linear",))
    with pytest.raises(ValueError, match="without repeats"):
        ops_agg.multi_aggregate(g, x, aggregators=("mean", "max", "mean"))
    with pytest.raises(ValueError, match="without repeats"):
        ops_agg.multi_aggregate(g, x, scalers=())
    for name in ("moment3", "moment4", "moment5"):
        with pytest.raises(NotImplementedError, match="built: mean, sum, max, min, var, std"):
            ops_agg.multi_aggregate(g, x, aggregators=("mean", name))
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="delta"):
            ops_agg.multi_aggregate(g, x, delta=bad)


def test_pna_delta():
    from dgll_amd import ops_agg

    g = _graph(_SQUARE, 6)
    want = np.mean([np.log(len(r) + 1.0) for r in _SQUARE])
    assert abs(ops_agg.pna_delta(g) - want) <= 1e-12
    with pytest.raises(TypeError):
        ops_agg.pna_delta(torch.eye(3))


# ---- the restatement itself ----------------------------------------------------------------------------------------------------------

def test_reference_on_a_graph_worked_by_hand():
    g = _graph([[0, 1, 1], [], [2]], 3)
    x = torch.tensor([[1.0], [4.0], [7.0]], dtype=torch.float64, requires_grad=True)
    y = torch.tensor([[10.0], [20.0], [30.0]], dtype=torch.float64)
    parts = {}
    out = pna_ref.multi_aggregate_reference(g.rowptr, g.col, x, y, pna_ref.AGGREGATORS, ("identity", "amplification"), 2.0, parts)
    var0 = (1.0 + 16.0 + 16.0) / 3 - 9.0
    want = torch.tensor([[13.0, 39.0, 14.0, 11.0, var0, var0 ** 0.5], [0.0] * 6, [37.0, 37.0, 37.0, 37.0, 0.0, 1e-15]], dtype=torch.float64)
    amp = torch.tensor([[np.log(4.0) / 2.0], [0.0], [np.log(2.0) / 2.0]])
    assert (out.detach() - torch.cat([want, amp * want], 1)).abs().max().item() <= 1e-12
    assert parts["argmax"].flatten().tolist() == [1, -1, 2] and parts["argmin"].flatten().tolist() == [0, -1, 2]
    (g_max,) = torch.autograd.grad(out[:, 2].sum(), x, retain_graph=True)
    assert g_max.flatten().tolist() == [0.0, 1.0, 1.0]                              # the source listed twice receives the maximum's gradient once
    (g_std,) = torch.autograd.grad(out[2, 5], x)
    assert g_std.abs().max().item() == 0.0                                          # a one-entry row: exactly no gradient through std


# ---- nn.PNAConv ---------------------------------------------------------------------------------------------------------------------

def test_pnaconv_names_shapes_and_exports():
    import dgll
    from dgll.nn.Convolution.pnaconv import PNAConv as alias
    from dgll_amd.nn import Convolution as conv

    assert {"PNAConv", "PNA"} <= set(conv.__all__) and alias is conv.PNAConv and dgll.nn.Convolution.PNAConv is conv.PNAConv
    layer = conv.PNAConv(12, 8, ["mean", "max", "sum"], ["identity", "amplification"], 2.5, num_towers=2, residual=False)
    want = []
    for t in range(2):
        want += ["towers.%d.M.weight" % t, "towers.%d.M.bias" % t, "towers.%d.U.weight" % t, "towers.%d.U.bias" % t]
        want += ["towers.%d.batchnorm.%s" % (t, n) for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    want += ["mixing_layer.0.weight", "mixing_layer.0.bias"]
    assert list(layer.state_dict()) == want
    assert tuple(layer.towers[0].M.weight.shape) == (6, 12) and tuple(layer.towers[1].U.weight.shape) == (4, (3 * 2 + 1) * 6)
    assert tuple(layer.mixing_layer[0].weight.shape) == (8, 8) and isinstance(layer.mixing_layer[1], torch.nn.LeakyReLU)
    model = conv.PNA(5, 8, 3, n_layers=2, delta=1.3, num_towers=2)
    out = model(_graph(_SQUARE, 6), torch.randn(6, 5))
    assert tuple(out.shape) == (6, 3) and bool(torch.isfinite(out).all())


def test_pnaconv_refusals():
    from dgll_amd.nn.Convolution import PNAConv

    args = (["mean", "std"], ["identity"], 1.0)
    with pytest.raises(ValueError, match="divisible"):
        PNAConv(10, 8, *args, num_towers=4, residual=False)
    with pytest.raises(ValueError, match="divisible"):
        PNAConv(8, 10, *args, num_towers=4, residual=False)
    with pytest.raises(ValueError, match="residual"):
        PNAConv(8, 4, *args)
    with pytest.raises(NotImplementedError, match="edge"):
        PNAConv(8, 8, *args, edge_feat_size=3)
    with pytest.raises(NotImplementedError, match="moment"):
        PNAConv(8, 8, ["mean", "moment3"], ["identity"], 1.0)
    with pytest.raises(ValueError, match="unknown aggregator"):
        PNAConv(8, 8, ["mode"], ["identity"], 1.0)
    with pytest.raises(ValueError, match="delta"):
        PNAConv(8, 8, ["mean"], ["identity"], 0.0)
    layer = PNAConv(8, 8, *args)
    g = _graph(_SQUARE, 6)
    with pytest.raises(NotImplementedError, match="edge"):
        layer(g, torch.randn(6, 8), edge_feat=torch.randn(g.nnz, 2))
    with pytest.raises(ValueError):
        layer(g, torch.randn(5, 8))
    with pytest.raises(ValueError, match="in_size"):
        layer(g, torch.randn(6, 4))


def _reference_layer(layer, graph, h_src, h_dst, snorm_n, training):
    sd = {k: v.detach().clone().double().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in layer.state_dict().items()}
    out = pna_ref.pna_conv_reference(sd, graph.rowptr, graph.col, h_src, h_dst, layer.aggregators, layer.scalers, layer.delta,
                                     layer.num_towers, layer.residual, snorm_n, training)
    return out, sd


@pytest.mark.parametrize("towers,block,training", [(1, False, True), (2, False, True), (2, True, True), (3, True, False)])
def test_pnaconv_host_path_matches_the_reference(towers, block, training):
    """The whole layer on CPU float64 (its _host_aggregate: per-edge messages, torch segment ops) against pna_ref: outputs and every
    parameter gradient at 1e-9 max |ref|.  All six aggregators; a row without entries, repeated entries, a rectangular block with
    snorm_n; train and eval mode."""
    from dgll_amd.nn.Convolution import PNAConv

    torch.manual_seed(11 + towers)
    graph = _block() if block else _graph(_SQUARE, 6)
    size = 6 * towers
    layer = PNAConv(size, size, pna_ref.AGGREGATORS, pna_ref.SCALERS, 1.4, num_towers=towers, residual=not block or towers == 2).double()
    for tower in layer.towers:                                  # statistics that are not the initial ones
        tower.batchnorm.running_mean.normal_()
        tower.batchnorm.running_var.uniform_(0.5, 2.0)
    layer.train(training)
    h_src = torch.randn(graph.n_cols, size, dtype=torch.float64)
    feat = (h_src, torch.randn(graph.n_rows, size, dtype=torch.float64)) if block else h_src
    snorm = torch.rand(graph.n_rows, 1, dtype=torch.float64) + 0.5 if block else None
    h_dst = feat[1] if block else h_src
    want, sd = _reference_layer(layer, graph, h_src, h_dst, snorm, training)
    # the reference's messages: distinct values stay apart (the smallest non-zero variance of a row's messages)
    row = pna_ref.rows_of(graph.rowptr)
    for msg in pna_ref.edge_messages({k: v.detach() for k, v in sd.items()}, graph.rowptr, graph.col, h_src, h_dst, towers):
        parts = {}
        pna_ref.reduce_messages(msg, row, graph.col.long(), graph.n_rows, ("var",), ("identity",), 1.0, parts)
        assert parts["var"][parts["var"] > 0].min().item() >= 1e-8
    got = layer(graph, feat, snorm_n=snorm)
    assert tuple(got.shape) == (graph.n_rows, size)
    assert (got.detach() - want.detach()).abs().max().item() <= 1e-9 * want.detach().abs().max().item()
    g = torch.randn(want.shape, dtype=torch.float64)
    got.backward(g)
    want.backward(g)
    for name, p in layer.named_parameters():
        ref = sd[name].grad
        top = ref.abs().max().item()
        if top < 1e-12:         # U.bias ahead of a batch norm in training mode: the mean is removed, the gradient is rounding residue alone
            assert name.endswith("U.bias") and training and p.grad.abs().max().item() < 1e-12, name
        else:
            assert (p.grad - ref).abs().max().item() <= 1e-9 * top, name


def test_host_aggregate_matches_the_reference_on_ties():
    """_host_aggregate alone, with messages that tie (a source listed three times alone in a row, integer-valued features): the tie
    rule and the exact zero of the variance's gradient, forward and input gradients at 1e-9."""
    from dgll_amd.nn.Convolution import pnaconv

    torch.manual_seed(5)
    graph = _block()
    fc = torch.nn.Linear(8, 4).double()
    with torch.no_grad():
        fc.weight.copy_(torch.randint(-2, 3, (4, 8)).double())
        fc.bias.zero_()
    hs = torch.randint(-1, 2, (12, 4)).double().requires_grad_()
    hd = torch.randint(-1, 2, (9, 4)).double().requires_grad_()
    got = pnaconv._host_aggregate(graph, hs, hd, fc, pna_ref.AGGREGATORS, pna_ref.SCALERS, 0.9)
    sd = {"towers.0.M.weight": fc.weight.detach(), "towers.0.M.bias": fc.bias.detach()}
    hs2, hd2 = hs.detach().clone().requires_grad_(), hd.detach().clone().requires_grad_()
    (msg,) = pna_ref.edge_messages(sd, graph.rowptr, graph.col, hs2, hd2, 1)
    want = pna_ref.reduce_messages(msg, pna_ref.rows_of(graph.rowptr), graph.col.long(), graph.n_rows, pna_ref.AGGREGATORS, pna_ref.SCALERS, 0.9)
    assert (got - want).abs().max().item() <= 1e-9 * want.abs().max().item()
    g = torch.randn(want.shape, dtype=torch.float64)
    got.backward(g)
    want.backward(g)
    for a, b in ((hs.grad, hs2.grad), (hd.grad, hd2.grad)):
        assert bool(torch.isfinite(a).all()) and (a - b).abs().max().item() <= 1e-9 * b.abs().max().item()
