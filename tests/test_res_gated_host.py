"""ResGated aggregation without a GPU: res_gated_ref.py against float64 autograd of a loop over the edges, the binding of
dgll_res_gated_desc and the host-side argument checks of dgll_hip_res_gated_pass, the refusals of
dgll_amd.ops_res_gated.res_gated_sum (names, dtypes and shapes first, then that the tensors are on the GPU, so both are checked
here), and nn.ResGatedGraphConv / ResGatedGCN: names, PyG's state dict, blocks, padding, the mean, and the host path term by term."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import res_gated_ref
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

@pytest.mark.parametrize("mean", [False, True], ids=["sum", "mean"])
def test_the_reference_agrees_with_autograd_of_a_loop_over_edges(mean):
    """res_gated_ref.forward / gradients (vectorised over the edge list) against float64 autograd of the formula written as a Python
    loop over rows and entries, on a block with an empty row, a column listed five times and unreferenced sources; the layer's host
    path (the same formula with index_add_) is held against the same loop."""
    from dgll_amd.nn.Convolution.resgatedconv import _host_res_gated_sum

    g = _block()
    gen = torch.Generator().manual_seed(1)
    mk = lambda n: torch.randn(n, 5, generator=gen, dtype=torch.float64, requires_grad=True)      # noqa: E731
    k, q, v = mk(9), mk(12), mk(12)
    go = torch.randn(9, 5, generator=gen, dtype=torch.float64)
    rp = g.rowptr.tolist()
    rows = []
    for i in range(9):
        acc = torch.zeros(5, dtype=torch.float64)
        for e in range(rp[i], rp[i + 1]):
            j = int(g.col[e])
            acc = acc + torch.sigmoid(k[i] + q[j]) * v[j]
        rows.append(acc / max(rp[i + 1] - rp[i], 1) if mean else acc)
    out = torch.stack(rows)
    want = torch.autograd.grad((out * go).sum(), (k, q, v))
    ins = [t.detach() for t in (k, q, v)]
    ref_out = res_gated_ref.forward(g.rowptr, g.col, *ins, mean=mean)
    _close("out", ref_out, out.detach(), 1e-12)
    _close("host path", _host_res_gated_sum(g, *ins, "mean" if mean else "sum"), out.detach(), 1e-12)      # the layer's own composition
    assert ref_out[4].abs().max().item() == 0.0                                     # the empty row
    for name, x, y in zip("kqv", res_gated_ref.gradients(g.rowptr, g.col, *ins, go, mean=mean), want):
        _close("grad_" + name, x, y, 1e-12)


# ---- the C entry point -----------------------------------------------------------------------------------------------------------

def test_descriptor_binding_matches_the_c_struct(tmp_path):
    """_lib.ResGatedDesc field by field against offsetof / sizeof of dgll_res_gated_desc as a C compiler lays it out, and in the
    header's order."""
    import subprocess

    from dgll_amd import _lib

    fields = [name for name, _ in _lib.ResGatedDesc._fields_]
    c_names = ["pass" if f == "pass_" else f for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dgll_hip.h"\nint main(void) {\n'
                   + "".join('    printf("%%zu\\n", offsetof(dgll_res_gated_desc, %s));\n' % n for n in c_names)
                   + '    printf("%zu\\n", sizeof(dgll_res_gated_desc));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [getattr(_lib.ResGatedDesc, f).offset for f in fields] + [ctypes.sizeof(_lib.ResGatedDesc)]
    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    body = re.search(r"typedef struct dgll_res_gated_desc \{(.*?)\} dgll_res_gated_desc;", text, re.S).group(1)
    assert re.findall(r"(\w+);", body) == c_names                                   # every member, in the header's order
    assert not any("perm" in n or n == "nnz" for n in c_names)                      # nothing per edge, and no permutation


def test_constants_match_the_header():
    from dgll_amd import _lib, ops_res_gated

    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    assert (int(re.search(r"#define\s+DGLL_RES_GATED_LONG_ROW\s+(\d+)", text).group(1)) == ops_res_gated.LONG_ROW
            == _lib.RES_GATED_LONG_ROW == _lib.GATED_LONG_ROW == 256)
    for name in ("FORWARD", "ROWS", "COLS"):
        assert int(re.search(r"DGLL_RES_GATED_%s\s*=\s*(\d+)" % name, text).group(1)) == getattr(_lib, "RES_GATED_" + name)
    assert _lib.lib.dgll_hip_abi_version() == 2                                     # an addition: the ABI version stays
    assert ops_res_gated._TAGS == ("res_gated_forward", "res_gated_rows", "res_gated_cols")


_MATS = ("k", "q", "v", "grad_out", "out", "grad_k", "grad_q", "grad_v")
# pass -> the operands it requires in its full form
_READS = {0: ("k", "q", "v", "out"),
          1: ("k", "q", "v", "grad_out", "grad_k"),
          2: ("k", "q", "v", "grad_out", "grad_q", "grad_v")}


def _valid(kind):
    """A descriptor that passes every check of the pass, with n_rows == 0 so that nothing is launched (the pointers are only
    inspected, never followed, before the checks pass)."""
    from dgll_amd import _lib

    buf = (ctypes.c_float * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    d = _lib.ResGatedDesc()
    d._keep = buf
    d.pass_, d.dtype, d.F, d.n_rows, d.n_cols = kind, _lib.F32, 8, 0, 4
    d.rowptr = d.col = base
    for m in _MATS:
        setattr(d, m, base)
        setattr(d, "ld_" + m, 12 if m in ("q", "v", "grad_q") else 8)              # three of them on a pitch of their own
    return d


def _refused(d, *words):
    from dgll_amd import _lib

    code = _lib.lib.dgll_hip_res_gated_pass(None, ctypes.byref(d))
    msg = _lib.last_error()
    assert code == INVALID and all(w in msg for w in words), (code, words, msg)


def test_pass_arguments_are_checked_on_the_host():
    from dgll_amd import _lib

    fn = _lib.lib.dgll_hip_res_gated_pass
    assert fn(None, None) == INVALID and "NULL" in _lib.last_error()                # a NULL descriptor
    for kind in range(3):                                                           # n_rows == 0: nothing to do, and nothing launched
        for mean in (0, 1):
            d = _valid(kind)
            d.mean = mean
            assert fn(None, ctypes.byref(d)) == _lib.OK, (kind, _lib.last_error())
    for bad in (3, -1):
        d = _valid(0)
        d.pass_ = bad
        _refused(d, "pass must be")
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
    for kind, reads in _READS.items():
        for m in reads:
            d = _valid(kind)
            setattr(d, m, None)
            if kind == 2 and m in ("grad_q", "grad_v"):                             # either output alone is a valid pass
                assert fn(None, ctypes.byref(d)) == _lib.OK, (m, _lib.last_error())
                continue
            _refused(d, "dgll_hip_res_gated_pass", m + " must be non-NULL")
            d = _valid(kind)
            setattr(d, m, getattr(d, m) + 4)                                        # a misaligned base
            _refused(d, m + " must be 16-byte aligned")
            d = _valid(kind)
            setattr(d, "ld_" + m, 4)                                                # a pitch shorter than F
            _refused(d, "ld_" + m)
            d = _valid(kind)
            setattr(d, "ld_" + m, 10)                                               # a pitch that is not whole vectors
            _refused(d, "ld_" + m)


def test_operands_a_pass_does_not_read_may_be_null():
    from dgll_amd import _lib

    fn = _lib.lib.dgll_hip_res_gated_pass
    for kind, reads in _READS.items():
        d = _valid(kind)
        for m in _MATS:
            if m not in reads:
                setattr(d, m, None)
        assert fn(None, ctypes.byref(d)) == _lib.OK, (kind, _lib.last_error())
    d = _valid(2)
    d.grad_q = d.grad_v = None
    _refused(d, "nothing to write")
    d = _valid(2)                                                                   # cols with grad_v alone does not read v ...
    d.grad_q = d.v = None
    assert fn(None, ctypes.byref(d)) == _lib.OK, _lib.last_error()
    d = _valid(2)                                                                   # ... with grad_q it does
    d.grad_v = d.v = None
    _refused(d, "v must be non-NULL")


# ---- dgll_amd.ops_res_gated --------------------------------------------------------------------------------------------------------

def test_op_refusals():
    from dgll_amd import ops_res_gated

    op = ops_res_gated.res_gated_sum
    g = _block()
    k, q, v = torch.randn(9, 8), torch.randn(12, 8), torch.randn(12, 8)
    with pytest.raises(TypeError):
        op(torch.eye(6), k, q, v)                                                   # not a CSRGraph
    with pytest.raises(TypeError):
        op(g, k, q.bfloat16(), v)                                                   # two dtypes
    with pytest.raises(TypeError):
        op(g, k.double(), q.double(), v.double())                                   # not a kernel dtype
    with pytest.raises(ValueError, match="destinations"):
        op(g, q, q, v)                                                              # rows of k
    with pytest.raises(ValueError, match="q must be"):
        op(g, k, k, v)                                                              # rows of q
    with pytest.raises(ValueError, match="v must be"):
        op(g, k, q, v[:-1])
    with pytest.raises(ValueError):
        op(g, k.reshape(-1), q, v)                                                  # not a matrix
    with pytest.raises(ValueError, match="one width"):
        op(g, k, q[:, :4], v)
    with pytest.raises(ValueError, match="one width"):
        op(g, k, q, v[:, :4])
    with pytest.raises(ValueError, match="the layers pad"):
        op(g, k[:, :6], q[:, :6], v[:, :6])                                         # F = 6
    with pytest.raises(ValueError, match="the layers pad"):
        op(g, *(t.bfloat16()[:, :4] for t in (k, q, v)))
    for reduce in ("max", "add", None):
        with pytest.raises(ValueError, match="reduce"):
            op(g, k, q, v, reduce=reduce)
    for reduce in ("sum", "mean"):
        with pytest.raises(RuntimeError, match="GPU"):                              # everything else is right: CPU tensors
            op(g, k, q, v, reduce=reduce)


# ---- the layer ---------------------------------------------------------------------------------------------------------------------

def test_layer_names_state_dict_and_exports():
    import dgll
    import dgll_amd.nn
    from dgll.nn.Convolution.resgatedconv import ResGatedGraphConv as alias
    from dgll_amd.nn import Convolution as conv

    names = {"ResGatedGraphConv", "ResGatedGCN"}
    assert names <= set(conv.__all__) and names <= set(dgll_amd.nn.__all__)
    assert alias is conv.ResGatedGraphConv and dgll.nn.Convolution.ResGatedGraphConv is conv.ResGatedGraphConv
    assert dgll_amd.nn.ResGatedGraphConv is conv.ResGatedGraphConv and dgll.nn.ResGatedGCN is conv.ResGatedGCN

    lins = {"%s.%s" % (m, s) for m in ("lin_key", "lin_query", "lin_value") for s in ("weight", "bias")}
    for root_weight in (True, False):                                               # PyG's keys, parameter for parameter
        for bias in (True, False):
            layer = conv.ResGatedGraphConv(5, 7, root_weight=root_weight, bias=bias)
            want = lins | ({"lin_skip.weight"} if root_weight else set()) | ({"bias"} if bias else set())
            assert set(layer.state_dict()) == want == {n for n, _ in layer.named_parameters()}
            assert (layer.lin_skip is None) == (not root_weight) and (layer.bias is None) == (not bias)
    layer = conv.ResGatedGraphConv((5, 3), 7)                                       # (src, dst): key and skip on the destinations
    assert [tuple(getattr(layer, m).weight.shape) for m in ("lin_key", "lin_query", "lin_value", "lin_skip")] == [(7, 3), (7, 5), (7, 5), (7, 3)]
    assert tuple(layer.bias.shape) == (7,) and float(layer.bias.detach().abs().max()) == 0.0
    for act in (None, torch.nn.Sigmoid(), torch.nn.Sigmoid):
        conv.ResGatedGraphConv(4, 4, act=act)

    model = conv.ResGatedGCN(5, 8, 4, layers=3)
    assert len(model.convs) == 3 and all(c.aggr == "mean" for c in model.convs)
    assert model.convs[0].lin_key.weight.shape == (8, 5) and model.convs[2].lin_key.weight.shape == (8, 8) and model.cls.weight.shape == (4, 8)


def test_what_is_not_built_raises():
    from dgll_amd.nn.Convolution import ResGatedGraphConv

    for act in (torch.nn.ReLU(), torch.nn.Tanh, torch.sigmoid):
        with pytest.raises(NotImplementedError, match="sigmoid"):
            ResGatedGraphConv(4, 4, act=act)
    with pytest.raises(NotImplementedError, match="GatedGCNConv"):
        ResGatedGraphConv(4, 4, edge_dim=3)
    with pytest.raises(ValueError, match="aggr"):
        ResGatedGraphConv(4, 4, aggr="max")


def _by_hand(layer, g, x_src, x_dst, mean=False):
    """the layer's forward, term by term, from its state dict (float64)"""
    sd = {k: v.detach().double() for k, v in layer.state_dict().items()}
    lin = lambda x, m: x.double() @ sd[m + ".weight"].t() + sd.get(m + ".bias", 0.0)        # noqa: E731
    out = res_gated_ref.forward(g.rowptr, g.col, lin(x_dst, "lin_key"), lin(x_src, "lin_query"), lin(x_src, "lin_value"), mean=mean)
    if "lin_skip.weight" in sd:
        out = out + lin(x_dst, "lin_skip")
    return out + sd.get("bias", 0.0)


@pytest.mark.parametrize("aggr", ["add", "sum", "mean"])
@pytest.mark.parametrize("root_weight,bias", [(True, True), (True, False), (False, True), (False, False)])
def test_host_path_term_by_term(root_weight, bias, aggr):
    from dgll_amd.nn.Convolution import ResGatedGraphConv

    g = _graph(_SQUARE, 6)
    gen = torch.Generator().manual_seed(3)
    torch.manual_seed(7)
    layer = ResGatedGraphConv(5, 10, root_weight=root_weight, bias=bias, aggr=aggr)
    if bias:
        with torch.no_grad():
            layer.bias.copy_(torch.randn(10, generator=gen))                        # off its default of zeros
    x = torch.randn(6, 5, generator=gen)
    got = layer(g, x)
    assert got.shape == (6, 10) and got.dtype == torch.float32
    _close("out", got, _by_hand(layer, g, x, x, mean=aggr == "mean"), 1e-5)
    # the row without entries: the skip term and the bias alone
    alone = (x[2] @ layer.lin_skip.weight.t() if root_weight else torch.zeros(10)) + (layer.bias if bias else 0.0)
    assert torch.allclose(got[2], alone, atol=1e-6)


def test_mean_is_the_sum_divided_by_the_degree_and_empty_rows_give_zero():
    from dgll_amd.nn.Convolution import ResGatedGraphConv
    from dgll_amd.nn.Convolution.resgatedconv import _host_res_gated_sum

    g = _block()
    gen = torch.Generator().manual_seed(6)
    k, q, v = (torch.randn(n, 6, generator=gen, dtype=torch.float64) for n in (9, 12, 12))
    total, mean = _host_res_gated_sum(g, k, q, v), _host_res_gated_sum(g, k, q, v, "mean")
    deg = g.degrees().double()
    assert deg[4].item() == 0 and total[4].abs().max().item() == 0.0 and mean[4].abs().max().item() == 0.0
    assert torch.allclose(mean[deg > 0], total[deg > 0] / deg[deg > 0].unsqueeze(1), rtol=1e-14, atol=0)
    _close("sum", total, res_gated_ref.forward(g.rowptr, g.col, k, q, v), 1e-14)
    _close("mean", mean, res_gated_ref.forward(g.rowptr, g.col, k, q, v, mean=True), 1e-14)
    # and through the layer: the same parameters, the two aggregations
    torch.manual_seed(1)
    add = ResGatedGraphConv((6, 6), 8, root_weight=False, bias=False)
    avg = ResGatedGraphConv((6, 6), 8, root_weight=False, bias=False, aggr="mean")
    avg.load_state_dict(add.state_dict())
    x_src, x_dst = torch.randn(12, 6, generator=gen), torch.randn(9, 6, generator=gen)
    a, m = add(g, (x_src, x_dst)), avg(g, (x_src, x_dst))
    assert m[4].abs().max().item() == 0.0
    assert torch.allclose(m, a / g.degrees().clamp(min=1).float().unsqueeze(1), rtol=1e-6, atol=1e-7)


def test_out_channels_10_on_the_host_and_the_padding_the_gpu_path_uses():
    """out_channels = 10 is no whole number of 16-byte vectors.  The host path needs no padding; the GPU path appends zero weight
    rows: the padded projections are the real ones plus zero columns (a gate of 1/2 on a value of 0), so the first 10 columns of the
    padded aggregation are the unpadded aggregation."""
    from dgll_amd import ops
    from dgll_amd.nn.Convolution import ResGatedGraphConv
    from dgll_amd.nn.Convolution.pnaconv import _linear, _pad_rows
    from dgll_amd.nn.Convolution.resgatedconv import _host_res_gated_sum

    g = _block()
    gen = torch.Generator().manual_seed(10)
    torch.manual_seed(10)
    layer = ResGatedGraphConv(6, 10)
    x_src, x_dst = torch.randn(12, 6, generator=gen), torch.randn(9, 6, generator=gen)
    got = layer(g, (x_src, x_dst))
    assert got.shape == (9, 10)
    _close("out", got, _by_hand(layer, g, x_src, x_dst), 1e-5)
    for dtype, padded in ((torch.float32, 12), (torch.bfloat16, 16)):
        assert ops.head_width_padded(10, dtype, pow2=False) == padded
    pad = 2
    k, q, v = (_linear(h, _pad_rows(fc.weight, pad), _pad_rows(fc.bias, pad)) for fc, h in
               ((layer.lin_key, x_dst), (layer.lin_query, x_src), (layer.lin_value, x_src)))
    assert k.shape == (9, 12) and all(float(t.detach()[:, 10:].abs().max()) == 0.0 for t in (k, q, v))
    k, q, v = k.detach(), q.detach(), v.detach()
    wide = _host_res_gated_sum(g, k, q, v)
    assert float(wide[:, 10:].abs().max()) == 0.0
    assert torch.equal(wide[:, :10], _host_res_gated_sum(g, k[:, :10], q[:, :10], v[:, :10]))


def test_blocks_pairs_and_refusals():
    from dgll_amd.nn.Convolution import ResGatedGraphConv

    g = _block()
    gen = torch.Generator().manual_seed(4)
    torch.manual_seed(4)
    layer = ResGatedGraphConv(6, 6)
    x_src, x_dst = torch.randn(12, 6, generator=gen), torch.randn(9, 6, generator=gen)
    # a tensor on a block: the destinations are the first n_dst sources
    both = torch.cat([x_dst, x_src[9:]], 0)
    assert torch.equal(layer(g, both), layer(g, (both, both[:9])))
    with pytest.raises(ValueError):
        layer(g, x_src[:5])
    with pytest.raises(ValueError):
        layer(g, (x_src, x_dst[:-1]))
    with pytest.raises(TypeError):
        layer(g, (x_src, x_dst.double()))
    pair = ResGatedGraphConv((6, 4), 8)                                             # different widths on the two sides
    out = pair(g, (x_src, x_dst[:, :4]))
    _close("pair", out, _by_hand(pair, g, x_src, x_dst[:, :4]), 1e-5)


def test_model_host_path_against_the_restatement_and_trains_every_parameter():
    from dgll_amd.nn.Convolution import ResGatedGCN

    g = _graph(_SQUARE, 6)
    gen = torch.Generator().manual_seed(2)
    torch.manual_seed(2)
    model = ResGatedGCN(6, 8, 4, layers=2)
    x = torch.randn(6, 6, generator=gen)
    out = model(g, x)
    assert out.shape == (6, 4)
    h = x.double()
    for conv in model.convs:
        h = torch.relu(_by_hand(conv, g, h, h, mean=True))
    _close("logits", out, h @ model.cls.weight.detach().double().t() + model.cls.bias.detach().double(), 1e-5)
    out.square().sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in model.parameters())
    drop = ResGatedGCN(6, 8, 4, layers=2, dropout=0.5)
    drop.load_state_dict(model.state_dict())
    assert torch.equal(drop.eval()(g, x), out.detach()) and not torch.equal(drop.train()(g, x), out.detach())
