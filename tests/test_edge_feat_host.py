"""Edge-feature aggregation without a GPU: the binding of dgll_edge_feat_desc, the host-side argument checks of
dgll_hip_edge_feat_pass (each names the offending field), the refusals of dgll_amd.ops_ef (names, dtypes and shapes first, then
that the tensors are on the GPU, so both are checked here), edge_graph_from_coo, and nn.GINEConv / GINE / CFConv: names, state
dicts, blocks, and their host path in fp32 against the float64 per-edge restatement of ef_ref.py at 1e-6 max |ref|, forward and
parameter gradients."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ef_ref
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


def _close(name, got, want, bar=1e-6):
    err = ((got.double() - want.double()).abs().max() / want.double().abs().max()).item()
    print("%-28s max/max %.3e  bar %.1e" % (name, err, bar))
    assert err <= bar, (name, err, bar)


# ---- the C entry point -----------------------------------------------------------------------------------------------------------

def test_descriptor_binding_matches_the_c_struct(tmp_path):
    """_lib.EdgeFeatDesc field by field against offsetof / sizeof of dgll_edge_feat_desc as a C compiler lays it out."""
    import subprocess

    from dgll_amd import _lib

    fields = [name for name, _ in _lib.EdgeFeatDesc._fields_]
    c_names = ["pass" if f == "pass_" else f for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dgll_hip.h"\nint main(void) {\n'
                   + "".join('    printf("%%zu\\n", offsetof(dgll_edge_feat_desc, %s));\n' % n for n in c_names)
                   + '    printf("%zu\\n", sizeof(dgll_edge_feat_desc));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [getattr(_lib.EdgeFeatDesc, f).offset for f in fields] + [ctypes.sizeof(_lib.EdgeFeatDesc)]


def test_constants_match_the_header():
    from dgll_amd import _lib, ops_ef

    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    assert int(re.search(r"#define\s+DGLL_EF_LONG_ROW\s+(\d+)", text).group(1)) == ops_ef.LONG_ROW == _lib.EF_LONG_ROW == 256
    for name in ("FORWARD", "COLS", "EDGE", "ADD", "ADD_RELU", "MUL"):
        assert int(re.search(r"DGLL_EF_%s\s*=\s*(\d+)" % name, text).group(1)) == getattr(_lib, "EF_" + name)
    assert _lib.lib.dgll_hip_abi_version() == 2                                     # an addition: the ABI version stays


def _valid(kind, op):
    """A descriptor that passes every check of (kind, op), with n_rows == 0 so that nothing is launched (the pointers are only
    inspected, never followed, before the checks pass)."""
    from dgll_amd import _lib

    buf = (ctypes.c_float * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    d = _lib.EdgeFeatDesc()
    d._keep = buf
    d.pass_, d.dtype, d.op, d.F, d.n_rows, d.n_cols, d.nnz = kind, _lib.F32, op, 8, 0, 4, 5
    d.rowptr = d.col = d.perm = d.scale = d.x = d.e = d.grad_out = d.out = d.grad_x = d.grad_e = base
    d.ld_x = d.ld_grad_out = d.ld_out = d.ld_grad_x = 8
    d.ld_e = d.ld_grad_e = 12                                                       # e and grad_e on a pitch of their own
    return d


def _refused(d, *words):
    from dgll_amd import _lib

    code = _lib.lib.dgll_hip_edge_feat_pass(None, ctypes.byref(d))
    msg = _lib.last_error()
    assert code == INVALID and all(w in msg for w in words), (code, words, msg)


def test_pass_arguments_are_checked_on_the_host():
    from dgll_amd import _lib

    fn = _lib.lib.dgll_hip_edge_feat_pass
    assert fn(None, None) == INVALID and "NULL" in _lib.last_error()                # a NULL descriptor
    for kind in range(3):                                                           # n_rows == 0: nothing to do, and nothing launched
        for op in range(3):
            assert fn(None, ctypes.byref(_valid(kind, op))) == _lib.OK, (kind, op, _lib.last_error())
    for field, bad in (("pass_", 3), ("pass_", -1), ("op", 3), ("op", -1)):
        d = _valid(0, 0)
        setattr(d, field, bad)
        _refused(d, field.rstrip("_"))
    for field in ("rowptr", "col"):                                                 # NULL CSR arrays
        for kind in range(3):
            d = _valid(kind, _lib.EF_ADD)
            setattr(d, field, None)
            _refused(d, field, "non-NULL")
    d = _valid(0, 0)
    d.dtype = 2                                                                     # neither F32 nor BF16
    _refused(d, "dtype")
    for dtype, F in ((_lib.F32, 6), (_lib.BF16, 12), (_lib.F32, 0)):                # not whole 16-byte vectors
        d = _valid(0, 0)
        d.dtype, d.F = dtype, F
        _refused(d, "F a positive multiple")
    d = _valid(0, 0)
    d.x += 4                                                                        # a misaligned base
    _refused(d, "x must be 16-byte aligned")
    d = _valid(_lib.EF_EDGE, _lib.EF_ADD)
    d.grad_e += 8
    _refused(d, "grad_e must be 16-byte aligned")
    d = _valid(0, 0)
    d.ld_e = 4                                                                      # a pitch shorter than F
    _refused(d, "ld_e")
    d = _valid(0, 0)
    d.ld_out = 10                                                                   # a pitch that is not whole vectors
    _refused(d, "ld_out")
    d = _valid(0, 0)
    d.nnz = 1 << 31
    _refused(d, "nnz")


# (pass, op) -> the operands it reads, of x / e / perm (include/dgll_hip.h)
_READS = {(0, 0): "xe", (0, 1): "xe", (0, 2): "xe",
          (1, 0): "", (1, 1): "xep", (1, 2): "ep",
          (2, 0): "", (2, 1): "xe", (2, 2): "x"}


@pytest.mark.parametrize("kind,op", sorted(_READS))
def test_operands_a_pass_reads_are_required_and_the_others_may_be_null(kind, op):
    from dgll_amd import _lib

    reads = _READS[(kind, op)]
    d = _valid(kind, op)                                                            # all that the pass does not read: NULL
    for letter, field in (("x", "x"), ("e", "e"), ("p", "perm")):
        if letter not in reads:
            setattr(d, field, None)
    d.scale = None
    for field in {0: ("grad_out", "grad_x", "grad_e"), 1: ("out", "grad_e"), 2: ("out", "grad_x")}[kind]:
        setattr(d, field, None)
    assert _lib.lib.dgll_hip_edge_feat_pass(None, ctypes.byref(d)) == _lib.OK, _lib.last_error()
    for letter, field in (("x", "x"), ("e", "e"), ("p", "perm")):
        if letter in reads:
            d = _valid(kind, op)
            setattr(d, field, None)
            _refused(d, field + " must be non-NULL")
    for field in {0: ("out",), 1: ("grad_out", "grad_x"), 2: ("grad_out", "grad_e")}[kind]:
        d = _valid(kind, op)
        setattr(d, field, None)
        _refused(d, field + " must be non-NULL")


# ---- dgll_amd.ops_ef ---------------------------------------------------------------------------------------------------------------

def test_op_refusals():
    from dgll_amd import ops_ef

    g = _graph(_SQUARE, 6)
    x, e = torch.randn(6, 8), torch.randn(g.nnz, 8)
    with pytest.raises(TypeError):
        ops_ef.u_op_e_sum(torch.eye(6), x, e)                                       # not a CSRGraph
    with pytest.raises(TypeError):
        ops_ef.u_op_e_sum(g, x, e.bfloat16())                                       # two dtypes
    with pytest.raises(TypeError):
        ops_ef.u_op_e_sum(g, x.double(), e.double())                                # not a kernel dtype
    with pytest.raises(ValueError):
        ops_ef.u_op_e_sum(g, x[:5], e)                                              # rows of x
    with pytest.raises(ValueError):
        ops_ef.u_op_e_sum(g, x, e[:-1])                                             # rows of e
    with pytest.raises(ValueError, match="width"):
        ops_ef.u_op_e_sum(g, x, e[:, :4])                                           # another width
    with pytest.raises(ValueError, match="the layers pad"):
        ops_ef.u_op_e_sum(g, x[:, :6], e[:, :6])                                    # F = 6
    with pytest.raises(ValueError, match="the layers pad"):
        ops_ef.u_op_e_sum(g, x.bfloat16()[:, :4], e.bfloat16()[:, :4])
    with pytest.raises(ValueError, match="relu"):
        ops_ef.u_op_e_sum(g, x, e, op="mul", act="relu")
    with pytest.raises(ValueError):
        ops_ef.u_op_e_sum(g, x, e, op="sub")
    with pytest.raises(ValueError):
        ops_ef.u_op_e_sum(g, x, e, act="elu")
    with pytest.raises(ValueError, match="max / min"):
        ops_ef.u_op_e_sum(g, x, e, reduce="max")
    for call in (lambda: ops_ef.u_op_e_sum(g, x, e), lambda: ops_ef.u_add_e_sum(g, x, e, act="relu", reduce="mean"),
                 lambda: ops_ef.u_mul_e_sum_full(g, x, e)):
        with pytest.raises(RuntimeError, match="GPU"):                              # everything else is right: CPU tensors
            call()


def test_edge_graph_from_coo_keeps_parallel_edges_apart_and_in_order():
    from dgll_amd import ops_ef

    src = torch.tensor([2, 0, 2, 1, 2, 0, 3, 2])
    dst = torch.tensor([1, 1, 1, 0, 1, 2, 0, 0])
    feat = torch.arange(8, dtype=torch.float32).unsqueeze(1) * torch.ones(1, 4)     # row k holds k
    g, e, order = ops_ef.edge_graph_from_coo(src, dst, feat, n_dst=4, n_src=5)
    assert (g.n_rows, g.n_cols, g.nnz) == (4, 5, 8)
    assert g.rowptr.tolist() == [0, 3, 7, 8, 8] and g.col.tolist() == [1, 2, 3, 0, 2, 2, 2, 0]
    assert order.tolist() == [3, 7, 6, 1, 0, 2, 4, 5]                               # 2 -> 1 three times, in order of appearance
    assert torch.equal(e, feat[order]) and e[:, 0].tolist() == [3.0, 7.0, 6.0, 1.0, 0.0, 2.0, 4.0, 5.0]
    assert torch.equal(src[order].to(torch.int32), g.col)
    g2, e2, order2 = ops_ef.edge_graph_from_coo(src, dst, feat)                     # sizes from the ids
    assert (g2.n_rows, g2.n_cols) == (3, 4) and torch.equal(order2, order)
    with pytest.raises(ValueError):
        ops_ef.edge_graph_from_coo(src, dst, feat[:-1])
    with pytest.raises(ValueError):
        ops_ef.edge_graph_from_coo(src, dst, feat, n_src=3)
    g0, e0, order0 = ops_ef.edge_graph_from_coo(src[:0], dst[:0], feat[:0], n_dst=2, n_src=2)
    assert g0.nnz == 0 and e0.shape == (0, 4) and order0.numel() == 0


def test_the_reference_agrees_with_itself():
    """ef_ref.gradients (written out entry by entry) is the autograd gradient of ef_ref.forward."""
    g = _block()
    gen = torch.Generator().manual_seed(0)
    for op in ef_ref.OPS:
        for reduce in ("sum", "mean"):
            x = torch.randn(12, 5, generator=gen, dtype=torch.float64, requires_grad=True)
            e = torch.randn(g.nnz, 5, generator=gen, dtype=torch.float64, requires_grad=True)
            go = torch.randn(9, 5, generator=gen, dtype=torch.float64)
            gx, ge = torch.autograd.grad(ef_ref.forward(g.rowptr, g.col, x, e, op, reduce), (x, e), go)
            want_gx, want_ge = ef_ref.gradients(g.rowptr, g.col, x.detach(), e.detach(), go, op, reduce)
            _close("gx %s %s" % (op, reduce), gx, want_gx, 1e-12)
            _close("ge %s %s" % (op, reduce), ge, want_ge, 1e-12)


# ---- the layers --------------------------------------------------------------------------------------------------------------------

def test_layer_names_state_dicts_and_exports():
    import dgll
    import dgll_amd.nn
    from dgll.nn.Convolution.cfconv import CFConv as cf_alias
    from dgll.nn.Convolution.gineconv import GINEConv as gine_alias
    from dgll_amd.nn import Convolution as conv

    assert {"GINEConv", "GINE", "CFConv"} <= set(conv.__all__) and {"GINEConv", "GINE", "CFConv"} <= set(dgll_amd.nn.__all__)
    assert gine_alias is conv.GINEConv and cf_alias is conv.CFConv and dgll.nn.Convolution.GINEConv is conv.GINEConv
    assert dgll_amd.nn.CFConv is conv.CFConv and dgll_amd.nn.GINE is conv.GINE

    fixed, learned = conv.GINEConv(), conv.GINEConv(torch.nn.Linear(4, 3), init_eps=0.25, learn_eps=True)
    assert list(fixed.state_dict()) == ["eps"] and not list(fixed.parameters()) and fixed.eps.shape == (1,) and fixed.eps.item() == 0.0
    assert set(learned.state_dict()) == {"eps", "apply_func.weight", "apply_func.bias"}
    assert isinstance(learned.eps, torch.nn.Parameter) and learned.eps.item() == 0.25
    fixed.load_state_dict({"eps": torch.tensor([0.5])})                              # buffer and Parameter share the key
    assert fixed.eps.item() == 0.5

    cf = conv.CFConv(5, 7, 6, 3)
    assert set(cf.state_dict()) == {p + s for p in ("project_edge.0.", "project_edge.2.", "project_node.", "project_out.0.")
                                    for s in ("weight", "bias")}
    assert cf.project_edge[0].weight.shape == (6, 7) and cf.project_edge[2].weight.shape == (6, 6)
    assert cf.project_node.weight.shape == (6, 5) and cf.project_out[0].weight.shape == (3, 6)
    ssp = conv.ShiftedSoftplus()
    assert ssp(torch.zeros(3)).abs().max().item() < 1e-7                             # softplus(0) - log 2
    assert torch.allclose(ssp(torch.tensor([30.0])), torch.tensor([30.0 - float(np.log(2.0))]))     # past the threshold: linear

    model = conv.GINE(5, 3, 8, 4, n_layers=3)
    assert [m.weight.shape for m in model.edge_encoders] == [(5, 3), (8, 3), (8, 3)]     # one encoder per layer, of that layer's width
    assert [m.weight.shape for m in model.lins] == [(8, 5), (8, 8), (8, 8)] and model.cls.weight.shape == (4, 8)
    assert all(isinstance(c.eps, torch.nn.Parameter) for c in model.convs)


def test_layer_refusals():
    from dgll_amd.nn.Convolution import CFConv, GINEConv

    g = _graph(_SQUARE, 6)
    h = torch.randn(6, 4)
    with pytest.raises(ValueError):
        GINEConv()(g, h, torch.randn(g.nnz, 3))                                     # another width: project it first
    with pytest.raises(ValueError):
        GINEConv()(g, h, torch.randn(g.nnz - 1, 4))
    with pytest.raises(TypeError):
        GINEConv()(g, h, torch.randn(g.nnz, 4).double())
    with pytest.raises(ValueError):
        GINEConv()(g, h[:5], torch.randn(g.nnz, 4))
    with pytest.raises(ValueError):
        CFConv(4, 3, 8, 2)(g, h, torch.randn(g.nnz + 1, 3))


@pytest.mark.parametrize("width", [8, 6], ids=["F8", "F6"])
@pytest.mark.parametrize("block", [False, True], ids=["square", "block"])
def test_gineconv_host_path_matches_the_reference(block, width):
    """fp32 on the host against float64: forward, the gradients of eps and apply_func's parameters, of h and of e.  The block is
    rectangular with a (src, dst) pair; both graphs have rows without entries."""
    from dgll_amd.nn.Convolution import GINEConv

    g = _block() if block else _graph(_SQUARE, 6)
    gen = torch.Generator().manual_seed(5 + width)
    layer = GINEConv(torch.nn.Linear(width, 5), init_eps=0.3, learn_eps=True)
    h_src = torch.randn(g.n_cols, width, generator=gen, requires_grad=True)
    h_dst = torch.randn(g.n_rows, width, generator=gen, requires_grad=True) if block else h_src
    e = torch.randn(g.nnz, width, generator=gen, requires_grad=True)
    go = torch.randn(g.n_rows, 5, generator=gen)
    out = layer(g, (h_src, h_dst) if block else h_src, e)
    assert out.shape == (g.n_rows, 5) and out.dtype == torch.float32
    params = list(layer.parameters())
    inputs = [h_src, e] + ([h_dst] if block else [])
    got = torch.autograd.grad(out, params + inputs, go)

    sd = {k: v.detach().double().requires_grad_() for k, v in layer.state_dict().items()}
    ins64 = [t.detach().double().requires_grad_() for t in inputs]
    h64, e64, hd64 = ins64[0], ins64[1], ins64[2] if block else ins64[0]
    probe = torch.zeros(g.n_rows, width, dtype=torch.float64, requires_grad=True)      # its gradient: that of apply_func's input
    want = ef_ref.gineconv(sd, g.rowptr, g.col, h64, hd64, e64, lambda v: (v + probe) @ sd["apply_func.weight"].t() + sd["apply_func.bias"])
    names = [n for n, _ in layer.named_parameters()]
    want_grads = torch.autograd.grad(want, [sd[n] for n in names] + ins64 + [probe], go.double())
    _close("out", out, want)
    for name, a, b in zip(names + ["h_src", "e", "h_dst"], got, want_grads):
        if name == "eps":
            # ONE number, the dot product <d loss / d apply_func's input, h_dst> of n_dst * F terms of either sign.  An fp32 dot product
            # is within n 2^-24 sum |terms| of the exact one whatever the order of summation, but relative to its own cancelled value
            # the error has no bound and moves with the machine's summation order (3.5e-7 on one CPU, 2.8e-6 on another, same
            # inputs): it is measured against sum |terms|, the scale its rounding error has.
            terms = (want_grads[-1] * hd64.detach()).abs().sum().item()
            err = abs(a.item() - b.item()) / terms
            print("%-28s err / sum|terms| %.3e  bar %.1e" % ("grad eps", err, 1e-6))
            assert err <= 1e-6, ("grad eps", err)
        else:
            _close("grad " + name, a, b)
    # a row without entries: (1 + eps) h_dst alone
    empty = 4 if block else 2
    assert torch.allclose(out[empty], layer.apply_func(1.3 * h_dst[empty]), atol=1e-6)
    # only the (src, dst) split of a tensor on a square graph / the first n_dst rows of a block
    if block:
        both = torch.cat([h_dst, h_src[g.n_rows:]], 0)
        assert torch.equal(layer(g, both, e), layer(g, (both, both[:g.n_rows]), e))


@pytest.mark.parametrize("hidden", [8, 6], ids=["H8", "H6"])
@pytest.mark.parametrize("block", [False, True], ids=["square", "block"])
def test_cfconv_host_path_matches_the_reference(block, hidden):
    from dgll_amd.nn.Convolution import CFConv

    g = _block() if block else _graph(_SQUARE, 6)
    gen = torch.Generator().manual_seed(11 + hidden)
    layer = CFConv(5, 7, hidden, 4)
    h_src = torch.randn(g.n_cols, 5, generator=gen, requires_grad=True)
    a = torch.randn(g.nnz, 7, generator=gen, requires_grad=True)
    go = torch.randn(g.n_rows, 4, generator=gen)
    out = layer(g, (h_src, h_src[:g.n_rows]) if block else h_src, a)
    assert out.shape == (g.n_rows, 4) and out.dtype == torch.float32
    names = [n for n, _ in layer.named_parameters()]
    got = torch.autograd.grad(out, list(layer.parameters()) + [h_src, a], go)

    sd = {k: v.detach().double().requires_grad_() for k, v in layer.state_dict().items()}
    h64, a64 = h_src.detach().double().requires_grad_(), a.detach().double().requires_grad_()
    want = ef_ref.cfconv(sd, g.rowptr, g.col, h64, a64)
    want_grads = torch.autograd.grad(want, [sd[n] for n in names] + [h64, a64], go.double())
    _close("out", out, want)
    for name, x, y in zip(names + ["h_src", "a"], got, want_grads):
        _close("grad " + name, x, y)
    # a row without entries aggregates 0: project_out of zeros
    empty = 4 if block else 2
    assert torch.allclose(out[empty], layer.project_out(torch.zeros(hidden)), atol=1e-7)


def test_gine_model_host_path_runs_and_trains_every_parameter():
    from dgll_amd.nn.Convolution import GINE

    g = _graph(_SQUARE, 6)
    gen = torch.Generator().manual_seed(2)
    model = GINE(6, 3, 8, 4, n_layers=2)
    x, attr = torch.randn(6, 6, generator=gen), torch.randn(g.nnz, 3, generator=gen)
    out = model(g, x, attr)
    assert out.shape == (6, 4)
    out.square().sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert all(float(m.weight.grad.abs().max()) > 0 for m in model.edge_encoders)   # the edge attributes reach the loss in every layer
