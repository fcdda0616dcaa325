"""The message-passing family without a GPU: the float64 restatements of mp_ref.py (the oracle of test_mp_gpu.py and
test_mp_emulated.py) against dense formulas, the host-side argument checks of dgll_hip_mp_pass, the binding of its descriptor, the
refusals of the dgll_amd.ops_mp wrappers (they check shapes and dtypes first, then that the tensors are on the GPU, so both are
checked here), and nn.AGNNConv: names, the host path against mp_ref, the refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mp_ref
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
    """9 destinations, 12 sources: an empty row, a repeated column, the last two sources never referenced."""
    rng = np.random.RandomState(3)
    rows = [list(rng.randint(0, 10, rng.randint(1, 6))) for _ in range(9)]
    rows[4] = []
    rows[6] = [3, 3, 8]
    return _graph(rows, 12)


# ---- the restatements ----------------------------------------------------------------------------------------------------------

def test_reference_equals_dense_formulas():
    """30 x 30, no duplicate entries: every operator against a dense masked matrix."""
    n, heads, D = 30, 3, 5
    gen = torch.Generator().manual_seed(0)
    mask = torch.rand(n, n, generator=gen) < 0.2
    mask[7] = False                                         # an empty row
    graph = _graph([mask[i].nonzero().flatten().tolist() for i in range(n)], n)
    rp, col = graph.rowptr, graph.col
    row = mp_ref.rows_of(rp)
    e = torch.randn(graph.nnz, heads, generator=gen, dtype=torch.float64)
    x, y = (torch.randn(n, heads, D, generator=gen, dtype=torch.float64) for _ in range(2))
    dense = torch.full((heads, n, n), -float("inf"), dtype=torch.float64)
    dense[:, row, col.long()] = e.t()
    for by, dim in (("dst", 2), ("src", 1)):
        sm = torch.nan_to_num(torch.softmax(dense, dim=dim), nan=0.0)
        got = mp_ref.edge_softmax_reference(rp, col, n, e, by)
        assert (got - sm[:, row, col.long()].t()).abs().max().item() <= 1e-12
    w = torch.zeros(heads, n, n, dtype=torch.float64)
    w[:, row, col.long()] = e.t()
    assert (mp_ref.u_mul_e_sum_reference(rp, col, x, e) - torch.einsum("hij,jhd->ihd", w, x)).abs().max().item() <= 1e-12
    dots = torch.einsum("ihd,jhd->hij", y, x)
    assert (mp_ref.u_dot_v_reference(rp, col, x, y) - dots[:, row, col.long()].t()).abs().max().item() <= 1e-12
    assert (mp_ref.copy_e_sum_reference(rp, col, n, e, "dst") - w.sum(2).t()).abs().max().item() <= 1e-12
    assert (mp_ref.copy_e_sum_reference(rp, col, n, e, "src") - w.sum(1).t()).abs().max().item() <= 1e-12
    a, b = (torch.randn(n, heads, generator=gen, dtype=torch.float64) for _ in range(2))
    assert torch.equal(mp_ref.u_add_v_reference(rp, col, a, b), a[col.long()] + b[row])


def test_reference_softmax_maps_minus_infinity_to_zero():
    graph = _graph([[0, 1, 2], [1, 2], []], 3)
    e = torch.tensor([[0.5], [-float("inf")], [1.5], [-float("inf")], [-float("inf")]], dtype=torch.float64, requires_grad=True)
    got = mp_ref.edge_softmax_reference(graph.rowptr, graph.col, 3, e)
    want = torch.softmax(torch.tensor([0.5, 1.5], dtype=torch.float64), 0)
    assert (got.detach().flatten() - torch.tensor([want[0], 0.0, want[1], 0.0, 0.0])).abs().max().item() <= 1e-15
    (grad,) = torch.autograd.grad(got, e, torch.ones_like(got))
    assert bool(torch.isfinite(grad).all())


# ---- the C entry point: every refusal happens on the host, before anything is launched -----------------------------------------------

def _valid(kind):
    """A descriptor that passes every check of `kind` (the pointers are only inspected, never followed, before the checks pass)."""
    from dgll_amd import _lib

    buf = (ctypes.c_float * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    d = _lib.MpDesc()
    d._keep = buf
    d.pass_, d.dtype, d.heads, d.D, d.n_rows, d.n_cols, d.nnz = kind, _lib.F32, 2, 8, 0, 4, 10
    d.rowptr = d.col = base
    d.e = d.e2 = d.e_out = d.x = d.y = d.out = base
    d.ld_e = d.ld_e2 = d.ld_e_out = 2
    node = kind in (_lib.MP_U_MUL_E_SUM, _lib.MP_U_DOT_V)
    d.ld_x = d.ld_y = d.ld_out = 16 if node else 2
    return d


def _refused(d, word):
    from dgll_amd import _lib

    code = _lib.lib.dgll_hip_mp_pass(None, ctypes.byref(d))
    msg = _lib.last_error()
    assert code == INVALID and word in msg, (code, msg)


def test_pass_arguments_are_checked_on_the_host():
    from dgll_amd import _lib

    fn = _lib.lib.dgll_hip_mp_pass
    assert fn(None, None) == INVALID and "NULL" in _lib.last_error()                # a NULL descriptor
    for kind in range(6):                                                           # n_rows == 0: nothing to do, and nothing launched
        assert fn(None, ctypes.byref(_valid(kind))) == _lib.OK, (kind, _lib.last_error())
    for bad in (-1, 6):
        d = _valid(0)
        d.pass_ = bad
        _refused(d, "pass")
    for kind in range(6):
        d = _valid(kind)
        d.heads = 0
        _refused(d, "heads")
        d = _valid(kind)
        d.rowptr = None
        _refused(d, "NULL")
        d = _valid(kind)
        d.n_rows = 4                                                                # (every refusal below also holds with rows to sweep)
        d.dtype = 7
        _refused(d, "dtype")
    for kind in (_lib.MP_U_MUL_E_SUM, _lib.MP_U_DOT_V):
        d = _valid(kind)
        d.n_rows, d.D = 4, 6
        _refused(d, "multiple")                                                     # D no whole number of vectors (4 fp32 columns)
        d.dtype, d.D = _lib.BF16, 12
        _refused(d, "multiple")                                                     # ... (8 bf16 columns)
        d.dtype, d.D, d.ld_x, d.ld_y, d.ld_out = _lib.F32, 260, 520, 520, 520
        _refused(d, "64 vectors")                                                   # a head of 65 vectors
        d = _valid(kind)
        d.n_rows, d.ld_x = 4, 18
        _refused(d, "pitch")                                                        # a pitch that is no multiple of 16 bytes
        d.ld_x = 8
        _refused(d, "pitch")                                                        # a pitch shorter than heads * D
        d.ld_x, d.x = 16, d.x + 4
        _refused(d, "aligned")                                                      # a misaligned base
        d = _valid(kind)
        d.n_rows, d.x = 4, None
        _refused(d, "x non-NULL")
        d = _valid(kind)
        d.n_rows, d.col = 4, None
        _refused(d, "NULL")
    d = _valid(_lib.MP_U_MUL_E_SUM)
    d.n_rows, d.e = 4, None
    _refused(d, "e non-NULL")
    d = _valid(_lib.MP_U_MUL_E_SUM)
    d.n_rows, d.ld_e = 4, 1
    _refused(d, "pitch >= heads")
    d = _valid(_lib.MP_U_MUL_E_SUM)
    d.n_rows, d.out = 4, None
    _refused(d, "out non-NULL")
    d = _valid(_lib.MP_U_DOT_V)
    d.n_rows, d.y = 4, None
    _refused(d, "y non-NULL")
    d = _valid(_lib.MP_U_DOT_V)
    d.n_rows, d.e_out = 4, None
    _refused(d, "e_out non-NULL")
    for kind in (_lib.MP_EDGE_SOFTMAX, _lib.MP_EDGE_SOFTMAX_BWD, _lib.MP_E_SUM):
        d = _valid(kind)
        d.n_rows, d.e = 4, None
        _refused(d, "e non-NULL")
        d = _valid(kind)
        d.n_rows, d.ld_e = 4, 1
        _refused(d, "pitch >= heads")
    for kind in (_lib.MP_EDGE_SOFTMAX, _lib.MP_EDGE_SOFTMAX_BWD, _lib.MP_U_ADD_V):
        d = _valid(kind)
        d.n_rows, d.e_out = 4, None
        _refused(d, "e_out non-NULL")
        d = _valid(kind)
        d.n_rows, d.ld_e_out = 4, 1
        _refused(d, "pitch >= heads")
    d = _valid(_lib.MP_EDGE_SOFTMAX_BWD)
    d.n_rows, d.e2 = 4, None
    _refused(d, "e2")
    d = _valid(_lib.MP_E_SUM)
    d.n_rows, d.out = 4, None
    _refused(d, "out non-NULL")
    d = _valid(_lib.MP_E_SUM)
    d.n_rows, d.ld_out = 4, 1
    _refused(d, "pitch >= heads")
    for kind in (_lib.MP_E_SUM, _lib.MP_U_ADD_V):                                   # fp32 per-row arrays only
        d = _valid(kind)
        d.n_rows, d.dtype = 4, _lib.BF16
        _refused(d, "DGLL_F32")
    d = _valid(_lib.MP_U_ADD_V)
    d.n_rows, d.ld_y = 4, 1
    _refused(d, "pitch >= heads")
    d = _valid(_lib.MP_U_ADD_V)
    d.n_rows, d.col = 4, None                                                       # x gathers through col
    _refused(d, "col")
    d = _valid(_lib.MP_U_ADD_V)
    d.x = d.col = None                                                              # either side may be NULL
    assert fn(None, ctypes.byref(d)) == _lib.OK
    d = _valid(_lib.MP_EDGE_SOFTMAX)
    d.n_rows, d.nnz = 4, 1 << 31
    _refused(d, "nnz")


def test_descriptor_binding_matches_the_c_struct(tmp_path):
    """_lib.MpDesc field by field against offsetof / sizeof of dgll_mp_desc as a C compiler lays it out."""
    import subprocess

    from dgll_amd import _lib

    fields = [name for name, _ in _lib.MpDesc._fields_]
    c_names = ["pass" if f == "pass_" else f for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dgll_hip.h"\nint main(void) {\n'
                   + "".join('    printf("%%zu\\n", offsetof(dgll_mp_desc, %s));\n' % n for n in c_names)
                   + '    printf("%zu\\n", sizeof(dgll_mp_desc));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [getattr(_lib.MpDesc, f).offset for f in fields] + [ctypes.sizeof(_lib.MpDesc)]


def test_constants_match_the_header():
    from dgll_amd import _lib, ops_mp

    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    assert int(re.search(r"#define\s+DGLL_MP_LONG_ROW\s+(\d+)", text).group(1)) == ops_mp.LONG_ROW == _lib.MP_LONG_ROW == 256
    names = ("EDGE_SOFTMAX", "EDGE_SOFTMAX_BWD", "E_SUM", "U_ADD_V", "U_MUL_E_SUM", "U_DOT_V")
    for name in names:
        assert int(re.search(r"DGLL_MP_%s\s*=\s*(\d+)" % name, text).group(1)) == getattr(_lib, "MP_" + name)


# ---- the wrappers' refusals ---------------------------------------------------------------------------------------------------------

def test_wrappers_refuse_cpu_tensors():
    from dgll_amd import ops_mp

    g = _graph(_SQUARE, 6)
    e, x, a = torch.ones(g.nnz, 2), torch.ones(6, 8), torch.ones(6, 2)
    for call in (lambda: ops_mp.edge_softmax(g, e), lambda: ops_mp.edge_softmax(g, e[:, 0], norm_by="src"), lambda: ops_mp.u_mul_e_sum(g, x, e),
                 lambda: ops_mp.u_dot_v(g, x, x, 2), lambda: ops_mp.u_add_v(g, a, a), lambda: ops_mp.copy_e_sum(g, e),
                 lambda: ops_mp.copy_e_sum(g, e, norm_by="src")):
        with pytest.raises(RuntimeError, match="GPU"):
            call()


def test_wrappers_refuse_wrong_shapes_and_dtypes():
    from dgll_amd import ops_mp

    g = _graph(_SQUARE, 6)
    e, x, a = torch.ones(g.nnz, 2), torch.ones(6, 8), torch.ones(6, 2)
    with pytest.raises(TypeError, match="CSRGraph"):
        ops_mp.edge_softmax(torch.eye(6).to_sparse(), e)
    # per-edge data is fp32
    for call in (lambda: ops_mp.edge_softmax(g, e.bfloat16()), lambda: ops_mp.u_mul_e_sum(g, x, e.double()), lambda: ops_mp.copy_e_sum(g, e.half())):
        with pytest.raises(TypeError, match="float32"):
            call()
    for call in (lambda: ops_mp.edge_softmax(g, e[:-1]), lambda: ops_mp.edge_softmax(g, e.unsqueeze(2)), lambda: ops_mp.copy_e_sum(g, e[1:]),
                 lambda: ops_mp.u_mul_e_sum(g, x, e[:5])):
        with pytest.raises(ValueError, match="nnz"):
            call()
    with pytest.raises(ValueError, match="norm_by"):
        ops_mp.edge_softmax(g, e, norm_by="both")
    with pytest.raises(ValueError, match="norm_by"):
        ops_mp.copy_e_sum(g, e, norm_by="row")
    with pytest.raises(ValueError, match="rows"):
        ops_mp.u_mul_e_sum(g, x[:5], e)
    with pytest.raises(ValueError, match="heads"):
        ops_mp.u_mul_e_sum(g, x, e, heads=4)                    # w has 2 columns
    with pytest.raises(ValueError, match="divide"):
        ops_mp.u_dot_v(g, x, x, 3)
    with pytest.raises(ValueError, match="the layers pad"):
        ops_mp.u_mul_e_sum(g, torch.ones(6, 12), e)             # D = 6: no whole number of 4-column vectors
    with pytest.raises(ValueError, match="the layers pad"):
        ops_mp.u_dot_v(g, x.bfloat16(), x.bfloat16(), 2)        # D = 4 bf16 columns
    with pytest.raises(ValueError, match="at most"):
        ops_mp.u_dot_v(g, torch.ones(6, 260), torch.ones(6, 260), 1)
    with pytest.raises(TypeError):
        ops_mp.u_dot_v(g, x.double(), x.double(), 2)
    with pytest.raises(ValueError, match="one dtype and width"):
        ops_mp.u_dot_v(g, x, x.bfloat16(), 1)
    with pytest.raises(ValueError, match="one dtype and width"):
        ops_mp.u_dot_v(g, x, torch.ones(6, 16), 1)
    with pytest.raises(TypeError, match="float32"):
        ops_mp.u_add_v(g, a.bfloat16(), a)
    with pytest.raises(ValueError, match="columns"):
        ops_mp.u_add_v(g, a, torch.ones(6, 3))
    with pytest.raises(ValueError):
        ops_mp.u_add_v(g, a[:5], a)


# ---- AGNNConv ------------------------------------------------------------------------------------------------------------------------

def _agnn_reference(graph, h_src, h_dst, beta):
    """DGL's AGNNConv through mp_ref: beta * cos, softmax over the row, weighted sum."""
    norm = lambda h: torch.nn.functional.normalize(h, p=2, dim=-1)      # noqa: E731
    e = beta * mp_ref.u_dot_v_reference(graph.rowptr, graph.col, norm(h_src).unsqueeze(1), norm(h_dst).unsqueeze(1))
    p = mp_ref.edge_softmax_reference(graph.rowptr, graph.col, graph.n_cols, e)
    return mp_ref.u_mul_e_sum_reference(graph.rowptr, graph.col, h_src.unsqueeze(1), p).squeeze(1)


def test_agnnconv_state_dict_and_beta():
    from dgll_amd.nn.Convolution import AGNNConv

    learn, fixed = AGNNConv(init_beta=2.0), AGNNConv(init_beta=0.5, learn_beta=False)
    assert list(learn.state_dict().keys()) == ["beta"] and list(fixed.state_dict().keys()) == ["beta"]
    assert isinstance(learn.beta, torch.nn.Parameter) and tuple(learn.beta.shape) == (1,) and learn.beta.item() == 2.0
    assert not isinstance(fixed.beta, torch.nn.Parameter) and tuple(fixed.beta.shape) == (1,) and fixed.beta.item() == 0.5
    assert [n for n, _ in learn.named_parameters()] == ["beta"] and list(fixed.parameters()) == []
    fixed.load_state_dict(learn.state_dict())
    assert fixed.beta.item() == 2.0


@pytest.mark.parametrize("learn", [True, False])
def test_agnnconv_host_path_matches_the_reference(learn):
    from dgll_amd.nn.Convolution import AGNNConv

    gen = torch.Generator().manual_seed(4)
    layer = AGNNConv(init_beta=1.7, learn_beta=learn).double()
    # a 9 x 12 block: a feature pair, and one tensor whose first rows are the destinations
    block = _block()
    h_src = torch.randn(12, 5, generator=gen, dtype=torch.float64, requires_grad=True)
    h_dst = torch.randn(9, 5, generator=gen, dtype=torch.float64, requires_grad=True)
    got, want = layer(block, (h_src, h_dst)), _agnn_reference(block, h_src, h_dst, layer.beta)
    assert got.shape == (9, 5) and (got - want).abs().max().item() <= 1e-12
    assert got[4].abs().max().item() == 0.0                 # the empty row
    leaves = [h_src, h_dst] + list(layer.parameters())
    g = torch.randn(9, 5, generator=gen, dtype=torch.float64)
    for a, b in zip(torch.autograd.grad(got, leaves, g), torch.autograd.grad(want, leaves, g)):
        assert (a - b).abs().max().item() <= 1e-12
    assert (layer(block, h_src) - _agnn_reference(block, h_src, h_src[:9], layer.beta)).abs().max().item() <= 1e-12
    # a square graph with an empty row
    square = _graph(_SQUARE, 6)
    x = torch.randn(6, 7, generator=gen, dtype=torch.float64)
    got = layer(square, x)
    assert (got - _agnn_reference(square, x, x, layer.beta)).abs().max().item() <= 1e-12 and got[2].abs().max().item() == 0.0


def test_agnnconv_refusals_and_exports():
    import dgll
    import dgll_amd.nn.Convolution as conv
    from dgll.nn.Convolution.agnnconv import AGNNConv as alias

    assert "AGNNConv" in conv.__all__ and alias is conv.AGNNConv and dgll.nn.Convolution.AGNNConv is conv.AGNNConv
    square = _graph(_SQUARE, 6)
    with pytest.raises(ValueError, match="rows without entries"):
        conv.AGNNConv(allow_zero_in_degree=False)(square, torch.randn(6, 4))
    layer = conv.AGNNConv()
    layer(square, torch.randn(6, 4))
    layer.set_allow_zero_in_degree(False)
    with pytest.raises(ValueError):
        layer(square, torch.randn(6, 4))
    with pytest.raises(ValueError, match="sources"):
        conv.AGNNConv()(square, torch.randn(5, 4))
