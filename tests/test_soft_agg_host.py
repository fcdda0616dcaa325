"""Soft aggregation without a GPU: softagg_ref.py against float64 autograd of the composition, the binding of dgll_soft_agg_desc and
the host-side argument checks of dgll_hip_soft_agg_pass, the refusals of dgll_amd.ops_softagg (names, dtypes and shapes first, then
that the tensors are on the GPU, so both are checked here), and nn.GENConv / DeeperGCN: names, PyG's state dict, blocks, padding, the
host path term by term, t = 0 and p = 1 as the mean, semi_grad."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import softagg_ref
from conftest import ROOT

INVALID = -1        # DGLL_ERR_INVALID


def _graph(rows, n_src):
    from dgll_amd import CSRGraph

    rowptr = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
    col = torch.tensor([int(c) for r in rows for c in r], dtype=torch.int32)
    return CSRGraph(rowptr, col, None, len(rows), n_src)


_SQUARE = [[0, 1, 4], [1], [], [0, 0, 2, 3, 5], [4, 5], [5, 1, 1]]      # row 2 is empty; rows 3 and 5 repeat a column


def _block():
    """9 destinations, 12 sources: an empty row, a row listing one source alone five times, the last two sources never referenced."""
    rng = np.random.RandomState(3)
    rows = [list(rng.randint(0, 10, rng.randint(1, 6))) for _ in range(9)]
    rows[4] = []
    rows[6] = [3] * 5
    return _graph(rows, 12)


def _close(name, got, want, bar):
    err = ((got.double() - want.double()).abs().max() / want.double().abs().max()).item()
    print("%-28s max/max %.3e  bar %.1e" % (name, err, bar))
    assert err <= bar, (name, err, bar)


# ---- the reference -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_e", [False, True], ids=["noe", "e"])
@pytest.mark.parametrize("mode,theta,semi", [("softmax", 1.0, False), ("softmax", -0.5, False), ("softmax", 8.0, False), ("softmax", 2.0, True),
                                             ("power", 0.5, False), ("power", 2.0, False), ("power", 1.0, False)])
def test_the_reference_agrees_with_autograd_of_the_composition(mode, theta, semi, with_e):
    """softagg_ref.reference (the formulas, row by row, no autograd) against float64 autograd of softagg_ref.composition (per-edge
    tensors and scatter ops) and of the layer's host path, on a block with an empty row, a column listed five times and unreferenced
    sources; some messages above the power mean's clamp of 100."""
    from dgll_amd.nn.Convolution.genconv import _host_soft_aggregate

    g = _block()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(12, 5, generator=gen, dtype=torch.float64)
    if mode == "power":
        x[3, 0], x[5, 1] = 150.0, 250.0                                             # above the clamp whatever e adds
    x.requires_grad_()
    e = torch.randn(g.nnz, 5, generator=gen, dtype=torch.float64, requires_grad=True) if with_e else None
    th = torch.tensor([theta], dtype=torch.float64, requires_grad=True)
    go = torch.randn(9, 5, generator=gen, dtype=torch.float64)
    leaves = [x] + ([e] if with_e else []) + [th]
    ref = softagg_ref.reference(g.rowptr, g.col, x.detach(), None if e is None else e.detach(), theta, go, mode, 1e-7, semi)
    for name, out in (("composition", softagg_ref.composition(g.rowptr, g.col, x, e, th, mode, 1e-7, semi)),
                      ("host path", _host_soft_aggregate(g, x, e, th, mode, semi, 1e-7))):
        grads = torch.autograd.grad((out * go).sum(), leaves, allow_unused=True)
        _close(name + " out", ref["out"], out.detach(), 1e-12)
        _close(name + " grad_x", ref["grad_x"], grads[0], 1e-10)
        if with_e:
            _close(name + " grad_e", ref["grad_e"], grads[1], 1e-10)
        if semi:
            assert ref["grad_theta"] is None and grads[-1] is None                  # semi_grad: t gets no gradient
        else:
            assert abs(ref["grad_theta"] - grads[-1].item()) <= 1e-10 * ref["scale"], (ref["grad_theta"], grads[-1].item())
    assert ref["out"][4].abs().max().item() == 0.0                                  # the empty row
    assert ref["grad_x"][10:].abs().max().item() == 0.0                             # the unreferenced sources
    if mode == "power":                                                             # above the clamp: no gradient
        assert ref["grad_x"][3, 0].item() == 0.0 and ref["grad_x"][5, 1].item() == 0.0


def test_t_zero_and_p_one_are_the_mean_of_the_messages():
    from dgll_amd.nn.Convolution.genconv import _host_soft_aggregate

    g = _block()
    gen = torch.Generator().manual_seed(2)
    x, e = torch.randn(12, 6, generator=gen, dtype=torch.float64), torch.randn(g.nnz, 6, generator=gen, dtype=torch.float64)
    go = torch.zeros(9, 6, dtype=torch.float64)
    m = torch.relu(x[g.col.long()] + e) + 1e-7
    row = g.row_index()
    mean = torch.zeros(9, 6, dtype=torch.float64).index_add_(0, row, m) / g.degrees().clamp(min=1).double().unsqueeze(1)
    for mode, theta in (("softmax", 0.0), ("power", 1.0)):
        _close(mode + " reference", softagg_ref.reference(g.rowptr, g.col, x, e, theta, go, mode)["out"], mean, 1e-13)
        _close(mode + " host path", _host_soft_aggregate(g, x, e, torch.tensor([theta], dtype=torch.float64), mode), mean, 1e-13)


# ---- the C entry point -----------------------------------------------------------------------------------------------------------

def test_descriptor_binding_matches_the_c_struct(tmp_path):
    """_lib.SoftAggDesc field by field against offsetof / sizeof of dgll_soft_agg_desc as a C compiler lays it out, and in the
    header's order."""
    import subprocess

    from dgll_amd import _lib

    fields = [name for name, _ in _lib.SoftAggDesc._fields_]
    c_names = ["pass" if f == "pass_" else f for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dgll_hip.h"\nint main(void) {\n'
                   + "".join('    printf("%%zu\\n", offsetof(dgll_soft_agg_desc, %s));\n' % n for n in c_names)
                   + '    printf("%zu\\n", sizeof(dgll_soft_agg_desc));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [getattr(_lib.SoftAggDesc, f).offset for f in fields] + [ctypes.sizeof(_lib.SoftAggDesc)]
    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    body = re.search(r"typedef struct dgll_soft_agg_desc \{(.*?)\} dgll_soft_agg_desc;", text, re.S).group(1)
    assert re.findall(r"(\w+);", body) == c_names                                   # every member, in the header's order


def test_constants_match_the_header():
    from dgll_amd import _lib, ops_agg, ops_softagg

    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    assert (int(re.search(r"#define\s+DGLL_SOFT_AGG_LONG_ROW\s+(\d+)", text).group(1)) == ops_softagg.LONG_ROW == _lib.SOFT_AGG_LONG_ROW
            == ops_agg.LONG_ROW == 256)
    assert int(re.search(r"#define\s+DGLL_SOFT_AGG_MAX_PARTIALS\s+(\d+)", text).group(1)) == _lib.SOFT_AGG_MAX_PARTIALS >= ops_softagg.PARTIALS >= 1
    for name in ("FORWARD", "ROWS", "COLS", "SOFTMAX", "POWER"):
        assert int(re.search(r"DGLL_SOFT_AGG_%s\s*=\s*(\d+)" % name, text).group(1)) == getattr(_lib, "SOFT_AGG_" + name)
    assert _lib.lib.dgll_hip_abi_version() == 2                                     # an addition: the ABI version stays
    assert ops_softagg._TAGS == ("soft_agg_forward", "soft_agg_rows", "soft_agg_cols")


_MATS = ("x", "e", "grad_out", "out", "grad_x", "grad_e")
# pass -> the matrices it requires in its full form (stats and theta: every pass)
_READS = {0: ("x", "e", "out"), 1: ("x", "e", "grad_out", "grad_e"), 2: ("x", "e", "grad_out", "grad_x")}


def _valid(kind, mode=0):
    """A descriptor that passes every check of the pass, with n_rows == 0 so that nothing is launched (the pointers are only
    inspected, never followed, before the checks pass)."""
    from dgll_amd import _lib

    buf = (ctypes.c_float * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    d = _lib.SoftAggDesc()
    d._keep = buf
    d.pass_, d.dtype, d.mode, d.F, d.n_rows, d.n_cols, d.nnz, d.eps = kind, _lib.F32, mode, 8, 0, 4, 5, 1e-7
    d.rowptr = d.col = d.perm = d.theta = d.stats = base
    d.ld_stats = 16
    for m in _MATS:
        setattr(d, m, base)
        setattr(d, "ld_" + m, 12 if m in ("x", "grad_x") else 8)                    # two of them on a pitch of their own
    if kind == 1:
        d.partials, d.n_partials, d.grad_theta = base, 7, base
    return d


def _refused(d, *words):
    from dgll_amd import _lib

    code = _lib.lib.dgll_hip_soft_agg_pass(None, ctypes.byref(d))
    msg = _lib.last_error()
    assert code == INVALID and all(w in msg for w in words), (code, words, msg)


def test_pass_arguments_are_checked_on_the_host():
    from dgll_amd import _lib

    fn = _lib.lib.dgll_hip_soft_agg_pass
    assert fn(None, None) == INVALID and "NULL" in _lib.last_error()                # a NULL descriptor
    for kind in range(3):                                                           # n_rows == 0: nothing to do, and nothing launched
        for mode in (0, 1):
            assert fn(None, ctypes.byref(_valid(kind, mode))) == _lib.OK, (kind, mode, _lib.last_error())
    for bad in (3, -1):
        d = _valid(0)
        d.pass_ = bad
        _refused(d, "pass must be")
    for bad in (2, -1):
        d = _valid(0)
        d.mode = bad
        _refused(d, "mode must be")
    for field in ("rowptr", "col"):
        for kind in range(3):
            d = _valid(kind)
            setattr(d, field, None)
            _refused(d, field, "non-NULL")
    d = _valid(0)
    d.dtype = 2
    _refused(d, "dtype")
    for dtype, F in ((_lib.F32, 6), (_lib.BF16, 12), (_lib.F32, 0)):                # not whole 16-byte vectors
        d = _valid(0)
        d.dtype, d.F = dtype, F
        _refused(d, "F a positive multiple")
    d = _valid(0)
    d.n_cols = 0
    _refused(d, "n_cols")
    d = _valid(0)
    d.nnz = -1
    _refused(d, "nnz")
    d = _valid(0)
    d.eps = -1.0
    _refused(d, "eps")
    for kind in range(3):
        d = _valid(kind)
        d.theta = None
        _refused(d, "theta", "non-NULL")
        d = _valid(kind)
        d.stats = None
        _refused(d, "stats", "non-NULL")
        d = _valid(kind)
        d.stats = d.stats + 4
        _refused(d, "stats must be 16-byte aligned")
        for ld in (12, 18):                                                         # shorter than 2 F; no whole vectors
            d = _valid(kind)
            d.ld_stats = ld
            _refused(d, "ld_stats")
    for kind, reads in _READS.items():
        for m in reads:
            if m != "e" and not (kind == 1 and m == "grad_e"):                      # e is optional in every pass, grad_e in rows
                d = _valid(kind)
                setattr(d, m, None)
                _refused(d, "dgll_hip_soft_agg_pass", m + " must be non-NULL")
            d = _valid(kind)
            setattr(d, m, getattr(d, m) + 4)                                        # a misaligned base
            _refused(d, m + " must be 16-byte aligned")
            d = _valid(kind)
            setattr(d, "ld_" + m, 4)                                                # a pitch shorter than F
            _refused(d, "ld_" + m)
            d = _valid(kind)
            setattr(d, "ld_" + m, 10)                                               # a pitch that is not whole vectors
            _refused(d, "ld_" + m)


def test_optional_operands_and_the_rows_pass():
    from dgll_amd import _lib

    fn = _lib.lib.dgll_hip_soft_agg_pass
    for kind, reads in _READS.items():                                              # what a pass does not read may be NULL
        d = _valid(kind)
        for m in _MATS:
            if m not in reads:
                setattr(d, m, None)
        assert fn(None, ctypes.byref(d)) == _lib.OK, (kind, _lib.last_error())
    for kind in (0, 2):                                                             # without e: no perm either
        d = _valid(kind)
        d.e = d.perm = None
        assert fn(None, ctypes.byref(d)) == _lib.OK, (kind, _lib.last_error())
    d = _valid(2)                                                                   # with e the transposed pass needs the permutation
    d.perm = None
    _refused(d, "perm must be non-NULL")
    d = _valid(1)                                                                   # rows: grad_e alone, the scalar gradient alone
    d.grad_theta = d.partials = None
    assert fn(None, ctypes.byref(d)) == _lib.OK, _lib.last_error()
    d = _valid(1)
    d.grad_e = d.e = None
    assert fn(None, ctypes.byref(d)) == _lib.OK, _lib.last_error()
    d = _valid(1)
    d.grad_e = d.grad_theta = None
    _refused(d, "nothing to write")
    d = _valid(1)
    d.e = None
    _refused(d, "grad_e without e")
    d = _valid(1)
    d.partials = None
    _refused(d, "partials", "non-NULL")
    for bad in (0, _lib.SOFT_AGG_MAX_PARTIALS + 1):
        d = _valid(1)
        d.n_partials = bad
        _refused(d, "n_partials")
    d = _valid(1)
    d.semi_grad = 1
    _refused(d, "semi_grad has no scalar gradient")
    d = _valid(1, mode=1)                                                           # the power mean has no semi_grad: the flag is ignored
    d.semi_grad = 1
    assert fn(None, ctypes.byref(d)) == _lib.OK, _lib.last_error()


# ---- dgll_amd.ops_softagg ----------------------------------------------------------------------------------------------------------

def test_op_refusals():
    from dgll_amd import ops_softagg

    g = _block()
    x, e = torch.randn(12, 8), torch.randn(g.nnz, 8)
    for op, name in ((ops_softagg.softmax_aggregate, "softmax_aggregate"), (ops_softagg.powermean_aggregate, "powermean_aggregate")):
        with pytest.raises(TypeError, match=name):
            op(torch.eye(6), x)                                                     # not a CSRGraph
        with pytest.raises(TypeError, match="one dtype"):
            op(g, x, e.bfloat16())
        with pytest.raises(TypeError):
            op(g, x.double(), e.double())                                           # not a kernel dtype
        with pytest.raises(ValueError, match="the sources"):
            op(g, x[:9])
        with pytest.raises(ValueError, match="x must be"):
            op(g, x.reshape(-1))                                                    # not a matrix
        with pytest.raises(ValueError, match="nnz"):
            op(g, x, e[:-1])
        with pytest.raises(ValueError, match="another width"):
            op(g, x, e[:, :4])
        with pytest.raises(ValueError, match="the layers pad"):
            op(g, x[:, :6], e[:, :6])                                               # F = 6
        with pytest.raises(ValueError, match="the layers pad"):
            op(g, x.bfloat16()[:, :4])
        with pytest.raises(ValueError, match="one-element"):
            op(g, x, e, torch.ones(8))                                              # one t / p per column is not built
        with pytest.raises(ValueError, match="one-element"):
            op(g, x, e, torch.ones(1, dtype=torch.int64))
        with pytest.raises(ValueError, match="eps"):
            op(g, x, e, eps=-1e-7)
        with pytest.raises(RuntimeError, match="GPU"):                              # everything else is right: CPU tensors
            op(g, x, e)
        with pytest.raises(RuntimeError, match="GPU"):
            op(g, x, None, torch.ones(1))
    with pytest.raises(ValueError, match="eps must be > 0"):
        ops_softagg.powermean_aggregate(g, x, e, eps=0.0)
    with pytest.raises(ValueError, match="p must not be 0"):
        ops_softagg.powermean_aggregate(g, x, e, p=0.0)


# ---- the layer ---------------------------------------------------------------------------------------------------------------------

def test_layer_names_state_dict_and_exports():
    import dgll
    import dgll_amd.nn
    from dgll.nn.Convolution.genconv import GENConv as alias
    from dgll_amd.nn import Convolution as conv

    names = {"GENConv", "DeeperGCN"}
    assert names <= set(conv.__all__) and names <= set(dgll_amd.nn.__all__)
    assert alias is conv.GENConv and dgll.nn.Convolution.GENConv is conv.GENConv
    assert dgll_amd.nn.GENConv is conv.GENConv and dgll.nn.DeeperGCN is conv.DeeperGCN

    layer = conv.GENConv(8, 8)                                                      # PyG's defaults: nothing to project, batch norm
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == {
        "aggr_module.t": (1,), "mlp.0.weight": (16, 8), "mlp.1.weight": (16,), "mlp.1.bias": (16,), "mlp.1.running_mean": (16,),
        "mlp.1.running_var": (16,), "mlp.1.num_batches_tracked": (), "mlp.4.weight": (8, 16)}
    assert {n for n, _ in layer.named_parameters()} == {"mlp.0.weight", "mlp.1.weight", "mlp.1.bias", "mlp.4.weight"}      # t: a buffer
    assert float(layer.aggr_module.t) == 1.0
    layer = conv.GENConv((5, 6), 7, aggr="power", p=2.0, learn_p=True, msg_norm=True, learn_msg_scale=True, norm="layer", bias=True, edge_dim=3)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == {
        "aggr_module.p": (1,), "lin_src.weight": (7, 5), "lin_src.bias": (7,), "lin_edge.weight": (7, 3), "lin_edge.bias": (7,),
        "lin_dst.weight": (7, 6), "lin_dst.bias": (7,), "mlp.0.weight": (14, 7), "mlp.0.bias": (14,), "mlp.1.weight": (14,),
        "mlp.1.bias": (14,), "mlp.4.weight": (7, 14), "mlp.4.bias": (7,), "msg_norm.scale": (1,)}
    params = dict(layer.named_parameters())
    assert params["aggr_module.p"].requires_grad and params["aggr_module.p"].item() == 2.0 and params["msg_norm.scale"].requires_grad
    layer = conv.GENConv(4, 6, aggr="softmax_sg", t=0.5, learn_t=False, msg_norm=True, norm=None, num_layers=3, expansion=3, edge_dim=6)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == {
        "aggr_module.t": (1,), "lin_src.weight": (6, 4), "lin_dst.weight": (6, 4), "mlp.0.weight": (18, 6), "mlp.3.weight": (18, 18),
        "mlp.6.weight": (6, 18), "msg_norm.scale": (1,)}                            # edge_dim == out_channels: no lin_edge
    assert not dict(layer.named_parameters())["msg_norm.scale"].requires_grad and layer.aggr_module.semi_grad
    layer = conv.GENConv(4, 4, learn_t=True, num_layers=1)
    assert set(layer.state_dict()) == {"aggr_module.t", "mlp.0.weight"} and layer.aggr_module.t.requires_grad
    assert conv.GENConv(4, 4, aggr="powermean").aggr_module.mode == "power"

    model = conv.DeeperGCN(5, 8, 4, 3)
    assert len(model.convs) == 3 and len(model.norms) == 3 and model.encoder.weight.shape == (8, 5) and model.cls.weight.shape == (4, 8)
    assert all(isinstance(c, conv.GENConv) and c.aggr_module.t.requires_grad for c in model.convs)


def test_what_is_not_built_raises():
    from dgll_amd.nn.Convolution import GENConv

    for aggr in ("mean", "max", "add", ["softmax", "power"], None):
        with pytest.raises(NotImplementedError, match="'softmax', 'softmax_sg', 'power' or 'powermean'"):
            GENConv(4, 4, aggr=aggr)
    with pytest.raises(ValueError, match="norm"):
        GENConv(4, 4, norm="instance")
    with pytest.raises(ValueError, match="p must not be 0"):
        GENConv(4, 4, aggr="power", p=0.0)
    with pytest.raises(ValueError, match="eps > 0"):
        GENConv(4, 4, aggr="power", eps=0.0)
    with pytest.raises(ValueError, match="softmax_sg"):
        GENConv(4, 4, aggr="softmax_sg", learn_t=True)
    g = _block()
    layer = GENConv((6, 6), 8, edge_dim=3)
    x_src, x_dst = torch.randn(12, 6), torch.randn(9, 6)
    with pytest.raises(ValueError):
        layer(g, (x_src, x_dst[:-1]))
    with pytest.raises(TypeError, match="one dtype"):
        layer(g, (x_src, x_dst.double()))
    with pytest.raises(ValueError, match="nnz"):
        layer(g, (x_src, x_dst), torch.randn(g.nnz - 1, 3))
    with pytest.raises(TypeError, match="edge_attr"):
        layer(g, (x_src, x_dst), torch.randn(g.nnz, 3).double())
    with pytest.raises(ValueError, match="edge_dim"):
        GENConv((6, 6), 8)(g, (x_src, x_dst), torch.randn(g.nnz, 3))                # no lin_edge for a width that differs


def _by_hand(layer, g, x_src, x_dst, edge_attr=None):
    """the layer's forward, term by term, from its state dict (float64, eval mode)"""
    sd = {k: v.detach().double() for k, v in layer.state_dict().items()}
    lin = lambda x, m: x.double() @ sd[m + ".weight"].t() + sd.get(m + ".bias", 0.0)        # noqa: E731
    h = lin(x_src, "lin_src") if "lin_src.weight" in sd else x_src.double()
    e = None
    if edge_attr is not None:
        e = lin(edge_attr, "lin_edge") if "lin_edge.weight" in sd else edge_attr.double()
    mode = layer.aggr_module.mode
    theta = sd["aggr_module.t" if mode == "softmax" else "aggr_module.p"].item()
    out = softagg_ref.reference(g.rowptr, g.col, h, e, theta, torch.zeros(g.n_rows, h.shape[1]), mode, layer.eps)["out"]
    if "msg_norm.scale" in sd:
        out = out / out.norm(dim=1, keepdim=True).clamp(min=1e-12) * x_dst.double().norm(dim=1, keepdim=True) * sd["msg_norm.scale"]
    out = out + (lin(x_dst, "lin_dst") if "lin_dst.weight" in sd else x_dst.double())
    mods = list(layer.mlp)
    for i, mod in enumerate(mods):
        if isinstance(mod, torch.nn.Linear):
            out = lin(out, "mlp.%d" % i)
        elif isinstance(mod, torch.nn.BatchNorm1d):
            out = (out - sd["mlp.%d.running_mean" % i]) / (sd["mlp.%d.running_var" % i] + mod.eps).sqrt() * sd["mlp.%d.weight" % i] + sd["mlp.%d.bias" % i]
        elif isinstance(mod, torch.nn.LayerNorm):
            out = (out - out.mean(1, keepdim=True)) / (out.var(1, unbiased=False, keepdim=True) + mod.eps).sqrt() * sd["mlp.%d.weight" % i] + sd["mlp.%d.bias" % i]
        elif isinstance(mod, torch.nn.ReLU):
            out = torch.relu(out)
    return out


@pytest.mark.parametrize("kw", [dict(), dict(aggr="power", p=2.0, norm="layer", bias=True, edge_dim=3),
                                dict(aggr="softmax", t=0.3, msg_norm=True, norm=None, edge_dim=10, num_layers=3),
                                dict(aggr="powermean", p=0.5, msg_norm=True, learn_msg_scale=True, norm="batch", num_layers=1)],
                         ids=["defaults", "power-layer-edge", "softmax-msgnorm-e10", "powermean-one-linear"])
def test_host_path_term_by_term(kw):
    from dgll_amd.nn.Convolution import GENConv

    g = _block()
    gen = torch.Generator().manual_seed(3)
    torch.manual_seed(7)
    layer = GENConv((6, 5), 10, **kw).eval()
    for mod in layer.mlp:                                                           # running statistics off their defaults
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=gen) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=gen) + 0.5)
    x_src, x_dst = torch.randn(12, 6, generator=gen), torch.randn(9, 5, generator=gen)
    edge = torch.randn(g.nnz, kw["edge_dim"], generator=gen) if "edge_dim" in kw else None
    got = layer(g, (x_src, x_dst), edge)
    assert got.shape == (9, 10) and got.dtype == torch.float32
    _close("out", got, _by_hand(layer, g, x_src, x_dst, edge), 1e-5)


def test_blocks_semi_grad_and_every_parameter_trains():
    from dgll_amd.nn.Convolution import DeeperGCN, GENConv

    g = _block()
    gen = torch.Generator().manual_seed(4)
    torch.manual_seed(4)
    layer = GENConv(6, 6, learn_t=True, norm="layer")
    x_src, x_dst = torch.randn(12, 6, generator=gen), torch.randn(9, 6, generator=gen)
    both = torch.cat([x_dst, x_src[9:]], 0)                                         # a tensor on a block: the destinations come first
    assert torch.equal(layer(g, both), layer(g, (both, both[:9])))
    layer(g, both).square().sum().backward()
    assert layer.aggr_module.t.grad is not None and float(layer.aggr_module.t.grad.abs()) > 0
    # semi_grad: the same forward, and t out of the backward
    full, semi = GENConv(6, 6, t=0.7, norm=None), GENConv(6, 6, aggr="softmax_sg", t=0.7, norm=None)
    semi.load_state_dict(full.state_dict())
    xa, xb = both.clone().requires_grad_(), both.clone().requires_grad_()
    a, b = full(g, xa), semi(g, xb)
    assert torch.equal(a, b)
    a.sum().backward()
    b.sum().backward()
    assert not torch.equal(xa.grad, xb.grad)
    t = torch.ones(1, requires_grad=True)
    from dgll_amd.nn.Convolution.genconv import _host_soft_aggregate
    gx, gt = torch.autograd.grad(_host_soft_aggregate(g, xa, None, t, "softmax", True).sum(), (xa, t), allow_unused=True)
    assert gt is None and gx is not None

    sq = _graph(_SQUARE, 6)
    torch.manual_seed(2)
    model = DeeperGCN(6, 8, 4, 3, msg_norm=True, learn_msg_scale=True)
    x = torch.randn(6, 6, generator=gen)
    out = model(sq, x)
    assert out.shape == (6, 4)
    out.square().sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in model.parameters())
    drop = DeeperGCN(6, 8, 4, 3, msg_norm=True, learn_msg_scale=True, dropout=0.5)
    drop.load_state_dict(model.state_dict())
    assert torch.equal(drop.eval()(sq, x), out.detach()) and not torch.equal(drop.train()(sq, x), out.detach())


def test_out_channels_10_and_the_padding_the_gpu_path_uses():
    """out_channels = 10 is no whole number of 16-byte vectors.  The GPU path pads the messages with zero columns; such a column
    aggregates to eps (softmax) or eps (the power mean of equal values), not to 0, so it is sliced off before anything else is added."""
    from dgll_amd import ops
    from dgll_amd.nn.Convolution.genconv import _host_soft_aggregate, _pad_cols

    for dtype, padded in ((torch.float32, 12), (torch.bfloat16, 16)):
        assert ops.head_width_padded(10, dtype, pow2=False) == padded
    g = _block()
    gen = torch.Generator().manual_seed(10)
    x, e = torch.randn(12, 10, generator=gen, dtype=torch.float64), torch.randn(g.nnz, 10, generator=gen, dtype=torch.float64)
    live = (g.degrees() > 0)
    for mode, theta in (("softmax", 1.5), ("power", 2.0)):
        th = torch.tensor([theta], dtype=torch.float64)
        wide = _host_soft_aggregate(g, _pad_cols(x, 2), _pad_cols(e, 2), th, mode)
        assert wide.shape == (9, 12) and torch.allclose(wide[live][:, 10:], torch.full((int(live.sum()), 2), 1e-7, dtype=torch.float64), rtol=1e-9)
        assert torch.equal(wide[:, :10], _host_soft_aggregate(g, x, e, th, mode))
