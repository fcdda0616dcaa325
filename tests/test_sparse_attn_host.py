"""Sparse dot-product attention without a GPU: the float64 restatement (attn_ref.py, the oracle of test_sparse_attn_gpu.py) against dense
masked softmax attention, the host paths of DotGatConv and TransformerConv against hand-written formulas, the parameter names of DGL
and PyG, the refused arguments, the exports, and the host-side argument checks of dgll_hip_sparse_attn_pass.

sparse_attention checks that its tensors are on the GPU before it looks at their shapes (as gatv2_aggregate does), so the shape and
width errors of the op are checked in test_sparse_attn_gpu.py; here: the graph type and the CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from attn_ref import sparse_attention_reference
from conftest import ROOT


def _graph(rows, n_src):
    """CSRGraph from a list of per-row column lists (kept as given: duplicates stay separate entries)."""
    from dgll_amd import CSRGraph

    rowptr = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
    col = torch.tensor([int(c) for r in rows for c in r], dtype=torch.int32)
    return CSRGraph(rowptr, col, None, len(rows), n_src)


def _ref(graph, q, k, v, heads, scale):
    """[n_dst, heads, D] from 2-D q, k, v through the restatement."""
    D = q.shape[1] // heads
    return sparse_attention_reference(graph.rowptr, graph.col, q.view(-1, heads, D), k.view(-1, heads, D), v.view(-1, heads, D), scale)[0]


_SQUARE = [[0, 1, 4], [1], [], [0, 0, 2, 3, 5], [4, 5], [5, 1, 1]]      # row 2 is empty; rows 3 and 5 repeat a column
_BLOCK = [[0, 5, 6], [], [1, 2, 2, 4], [3]]                             # 4 destinations, 7 sources


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def test_reference_equals_dense_masked_softmax_attention():
    """40 nodes, no duplicate entries, every row non-empty: softmax over a -inf-masked dense score matrix."""
    n, heads, D = 40, 3, 5
    gen = torch.Generator().manual_seed(0)
    mask = torch.rand(n, n, generator=gen) < 0.15
    mask |= torch.eye(n, dtype=torch.bool)
    rows = [mask[i].nonzero().flatten().tolist() for i in range(n)]
    graph = _graph(rows, n)
    q, k, v = (torch.randn(n, heads, D, generator=gen, dtype=torch.float64) for _ in range(3))
    scale = D ** -0.5
    out, s = sparse_attention_reference(graph.rowptr, graph.col, q, k, v, scale)
    dense = torch.einsum("ihd,jhd->hij", q, k) * scale
    dense = dense.masked_fill(~mask.unsqueeze(0), -float("inf"))
    want = torch.einsum("hij,jhd->ihd", torch.softmax(dense, dim=-1), v)
    assert out.shape == (n, heads, D) and s.shape == (graph.nnz, heads)
    assert (out - want).abs().max().item() <= 1e-12


def test_reference_counts_a_duplicated_entry_twice_and_leaves_an_empty_row_zero():
    heads, D = 2, 3
    gen = torch.Generator().manual_seed(1)
    q = torch.randn(3, heads, D, generator=gen, dtype=torch.float64)
    k, v = (torch.randn(4, heads, D, generator=gen, dtype=torch.float64) for _ in range(2))
    graph = _graph([[1, 1, 2], [], [0]], 4)
    out, _ = sparse_attention_reference(graph.rowptr, graph.col, q, k, v, 0.7)
    s1, s2 = (q[0] * k[1]).sum(-1) * 0.7, (q[0] * k[2]).sum(-1) * 0.7
    w1, w2 = 2 * torch.exp(s1), torch.exp(s2)                   # column 1 twice: twice its weight
    want0 = (w1.unsqueeze(-1) * v[1] + w2.unsqueeze(-1) * v[2]) / (w1 + w2).unsqueeze(-1)
    assert (out[0] - want0).abs().max().item() <= 1e-12
    assert out[1].abs().max().item() == 0.0                     # the empty row
    assert (out[2] - v[0]).abs().max().item() <= 1e-12          # one entry: its value


def test_padded_scale_misses_the_forward_bar():
    """The power of the padded-head GPU test: a 6-wide head padded to 8 computed with scale = 8 ** -0.5 instead of 6 ** -0.5 is
    further from the truth than the fp32 forward bar allows (max |err| <= 1e-4 max |ref|)."""
    heads, D = 3, 6
    gen = torch.Generator().manual_seed(2)
    graph = _graph(_SQUARE, 6)
    q, k, v = (torch.randn(6, heads, D, generator=gen, dtype=torch.float64) for _ in range(3))
    right, _ = sparse_attention_reference(graph.rowptr, graph.col, q, k, v, 6 ** -0.5)
    wrong, _ = sparse_attention_reference(graph.rowptr, graph.col, q, k, v, 8 ** -0.5)
    assert (right - wrong).abs().max().item() > 1e-4 * right.abs().max().item()


# ---- DotGatConv ----------------------------------------------------------------------------------------------------------------

def test_dotgatconv_host_path_matches_the_formula():
    from dgll_amd.nn.Convolution import DotGatConv

    torch.manual_seed(3)
    graph = _graph(_SQUARE, 6)
    layer = DotGatConv(7, 3, 2).double()
    x = torch.randn(6, 7, dtype=torch.float64, requires_grad=True)
    got = layer(graph, x)
    h = x @ layer.fc.weight.t()
    want = _ref(graph, h, h, h, 2, 3 ** -0.5)
    assert got.shape == (6, 2, 3)
    assert (got - want).abs().max().item() <= 1e-12
    assert got[2].abs().max().item() == 0.0         # the empty row
    g = torch.randn_like(got)
    params = [x] + list(layer.parameters())
    for a, b in zip(torch.autograd.grad(got, params, g, retain_graph=True), torch.autograd.grad(want, params, g)):
        assert (a - b).abs().max().item() <= 1e-10


def test_dotgatconv_host_path_on_a_block_and_a_feature_pair():
    from dgll_amd.nn.Convolution import DotGatConv

    torch.manual_seed(4)
    graph = _graph(_BLOCK, 7)
    h_src, h_dst = torch.randn(7, 5, dtype=torch.float64), torch.randn(4, 4, dtype=torch.float64)
    pair = DotGatConv((5, 4), 3, 2).double()
    got = pair(graph, (h_src, h_dst))
    ks = h_src @ pair.fc_src.weight.t()
    want = _ref(graph, h_dst @ pair.fc_dst.weight.t(), ks, ks, 2, 3 ** -0.5)
    assert got.shape == (4, 2, 3) and (got - want).abs().max().item() <= 1e-12
    # one tensor on a block: the destinations are its first rows; one fc on a pair of equal widths
    single = DotGatConv(5, 3, 2).double()
    ks = h_src @ single.fc.weight.t()
    want = _ref(graph, ks[:4], ks, ks, 2, 3 ** -0.5)
    assert (single(graph, h_src) - want).abs().max().item() <= 1e-12
    assert (single(graph, (h_src, h_src[:4].clone())) - want).abs().max().item() <= 1e-12
    assert single(graph, h_src)[1].abs().max().item() == 0.0


def test_dotgatconv_state_dict_and_refusals():
    from dgll_amd.nn.Convolution import DotGatConv

    assert {k: tuple(v.shape) for k, v in DotGatConv(10, 4, 3).state_dict().items()} == {"fc.weight": (12, 10)}
    assert {k: tuple(v.shape) for k, v in DotGatConv((10, 6), 4, 3).state_dict().items()} == \
        {"fc_src.weight": (12, 10), "fc_dst.weight": (12, 6)}
    graph = _graph(_BLOCK, 7)
    layer = DotGatConv(5, 3, 2)
    with pytest.raises(NotImplementedError, match="get_attention"):
        layer(graph, torch.randn(7, 5), get_attention=True)
    with pytest.raises(ValueError, match="rows without entries"):
        DotGatConv(5, 3, 2, allow_zero_in_degree=False)(graph, torch.randn(7, 5))
    with pytest.raises(ValueError, match="sources"):
        layer(graph, torch.randn(6, 5))
    layer.set_allow_zero_in_degree(False)
    with pytest.raises(ValueError):
        layer(graph, torch.randn(7, 5))


# ---- TransformerConv ---------------------------------------------------------------------------------------------------------

def _transformer_formula(layer, graph, x_src, x_dst):
    """PyG's TransformerConv from the layer's parameters, written out."""
    heads, fo = layer.heads, layer.out_channels
    lin = lambda fc, h: h @ fc.weight.t() + (fc.bias if fc.bias is not None else 0)     # noqa: E731
    out = _ref(graph, lin(layer.lin_query, x_dst), lin(layer.lin_key, x_src), lin(layer.lin_value, x_src), heads, fo ** -0.5)
    out = out.reshape(-1, heads * fo) if layer.concat else out.mean(1)
    if layer.lin_skip is not None:
        x_r = lin(layer.lin_skip, x_dst)
        if layer.lin_beta is not None:
            b = torch.sigmoid(torch.cat([x_r, out, out - x_r], dim=-1) @ layer.lin_beta.weight.t())
            out = b * x_r + (1 - b) * out
        else:
            out = out + x_r
    return out


@pytest.mark.parametrize("concat,beta,root_weight,bias", [(True, False, True, True), (False, False, True, True), (True, True, True, True),
                                                          (False, True, True, False), (True, False, False, True), (False, True, False, True)])
def test_transformerconv_host_path_matches_the_formula(concat, beta, root_weight, bias):
    from dgll_amd.nn.Convolution import TransformerConv

    torch.manual_seed(5)
    graph = _graph(_SQUARE, 6)
    layer = TransformerConv(7, 3, heads=2, concat=concat, beta=beta, root_weight=root_weight, bias=bias).double()
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn_like(p))
    x = torch.randn(6, 7, dtype=torch.float64, requires_grad=True)
    got = layer(graph, x)
    want = _transformer_formula(layer, graph, x, x)
    assert got.shape == ((6, 6) if concat else (6, 3))
    assert (got - want).abs().max().item() <= 1e-12
    if not root_weight:
        assert got[2].abs().max().item() == 0.0     # the empty row
    g = torch.randn_like(got)
    params = [x] + list(layer.parameters())
    for a, b in zip(torch.autograd.grad(got, params, g, retain_graph=True), torch.autograd.grad(want, params, g)):
        assert (a - b).abs().max().item() <= 1e-10


def test_transformerconv_host_path_on_a_block_and_a_feature_pair():
    from dgll_amd.nn.Convolution import TransformerConv

    torch.manual_seed(6)
    graph = _graph(_BLOCK, 7)
    x_src, x_dst = torch.randn(7, 5, dtype=torch.float64), torch.randn(4, 4, dtype=torch.float64)
    pair = TransformerConv((5, 4), 3, heads=2, beta=True).double()
    got = pair(graph, (x_src, x_dst))
    assert got.shape == (4, 6) and (got - _transformer_formula(pair, graph, x_src, x_dst)).abs().max().item() <= 1e-12
    single = TransformerConv(5, 3, heads=2, concat=False).double()
    got = single(graph, x_src)                      # a block: the destinations are the first rows
    assert got.shape == (4, 3) and (got - _transformer_formula(single, graph, x_src, x_src[:4])).abs().max().item() <= 1e-12
    assert bool(torch.isfinite(got).all())
    with pytest.raises(ValueError, match="sources"):
        single(graph, x_src[:6])


def test_transformerconv_state_dict_has_pygs_names_and_shapes():
    from dgll_amd.nn.Convolution import TransformerConv

    qkv = {"lin_key.weight": (12, 10), "lin_key.bias": (12,), "lin_query.weight": (12, 10), "lin_query.bias": (12,),
           "lin_value.weight": (12, 10), "lin_value.bias": (12,)}
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}       # noqa: E731
    assert shapes(TransformerConv(10, 4, heads=3)) == dict(qkv, **{"lin_skip.weight": (12, 10), "lin_skip.bias": (12,)})
    assert shapes(TransformerConv(10, 4, heads=3, beta=True)) == \
        dict(qkv, **{"lin_skip.weight": (12, 10), "lin_skip.bias": (12,), "lin_beta.weight": (1, 36)})
    assert shapes(TransformerConv(10, 4, heads=3, concat=False, beta=True, bias=False)) == \
        dict(qkv, **{"lin_skip.weight": (4, 10), "lin_beta.weight": (1, 12)})
    assert shapes(TransformerConv(10, 4, heads=3, beta=True, root_weight=False)) == qkv
    pair = shapes(TransformerConv((10, 6), 4, heads=3))
    assert pair["lin_key.weight"] == (12, 10) and pair["lin_value.weight"] == (12, 10)
    assert pair["lin_query.weight"] == (12, 6) and pair["lin_skip.weight"] == (12, 6)
    layer = TransformerConv(10, 4, heads=3, beta=True)
    layer.load_state_dict({k: torch.zeros_like(v) for k, v in layer.state_dict().items()})
    layer.reset_parameters()
    assert layer.lin_key.weight.abs().max().item() > 0.0


def test_transformerconv_refuses_dropout_and_edge_features():
    from dgll_amd.nn.Convolution import TransformerConv

    with pytest.raises(ValueError, match="dropout"):
        TransformerConv(4, 4, heads=2, dropout=0.1)
    with pytest.raises(ValueError, match="edge_dim"):
        TransformerConv(4, 4, heads=2, edge_dim=3)
    TransformerConv(4, 4, heads=2, dropout=0.0, edge_dim=None)


# ---- exports, the op's refusals, the ABI ---------------------------------------------------------------------------------------

def test_exports_and_aliases():
    import dgll
    import dgll_amd.nn.Convolution as conv
    from dgll.nn.Convolution.dotgatconv import DotGatConv as dot_alias
    from dgll.nn.Convolution.transformerconv import TransformerConv as tr_alias

    assert "DotGatConv" in conv.__all__ and "TransformerConv" in conv.__all__
    assert all(hasattr(conv, name) for name in conv.__all__)
    assert dot_alias is conv.DotGatConv and tr_alias is conv.TransformerConv
    assert dgll.nn.Convolution.DotGatConv is conv.DotGatConv and dgll.nn.Convolution.TransformerConv is conv.TransformerConv


def test_op_refuses_a_foreign_graph_and_cpu_tensors():
    from dgll_amd import ops_attn

    x = torch.ones(6, 8)
    with pytest.raises(TypeError, match="CSRGraph"):
        ops_attn.sparse_attention(torch.eye(6).to_sparse(), x, x, x, 2)
    with pytest.raises(RuntimeError):
        ops_attn.sparse_attention(_graph(_SQUARE, 6), x, x, x, 2)


def test_long_row_constant_matches_the_header():
    from dgll_amd import _lib, ops_attn

    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    assert int(re.search(r"#define\s+DGLL_ATTN_LONG_ROW\s+(\d+)", text).group(1)) == ops_attn.LONG_ROW == _lib.ATTN_LONG_ROW == 256


def test_pass_arguments_are_checked_on_the_host():
    from dgll_amd import _lib

    fn = _lib.lib.dgll_hip_sparse_attn_pass
    assert fn(None, None) == -1 and "NULL" in _lib.last_error()                     # a NULL descriptor
    d = _lib.AttnDesc()
    d.pass_, d.dtype, d.heads, d.D, d.n_rows, d.n_cols, d.scale = _lib.ATTN_FORWARD, 7, 2, 8, 4, 4, 0.5
    assert fn(None, ctypes.byref(d)) == -1 and "dtype" in _lib.last_error()         # an unknown dtype
    d.dtype, d.pass_ = _lib.F32, 5
    assert fn(None, ctypes.byref(d)) == -1 and "pass" in _lib.last_error()          # an unknown pass
    d.pass_, d.heads = _lib.ATTN_FORWARD, 0
    assert fn(None, ctypes.byref(d)) == -1 and "heads" in _lib.last_error()         # heads < 1
    d.heads, d.D = 1, 6
    assert fn(None, ctypes.byref(d)) == -1 and "multiple" in _lib.last_error()      # D no whole number of vectors (4 fp32 columns)
    d.dtype, d.D = _lib.BF16, 12
    assert fn(None, ctypes.byref(d)) == -1 and "multiple" in _lib.last_error()      # ... (8 bf16 columns)
    d.dtype, d.D = _lib.F32, 8
    assert fn(None, ctypes.byref(d)) == -1 and "NULL" in _lib.last_error()          # no CSR arrays, no matrices
    # pointers are only inspected, never followed, before the checks pass
    buf = (ctypes.c_float * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    d.rowptr = d.col = base
    assert fn(None, ctypes.byref(d)) == -1 and "NULL" in _lib.last_error()          # q, k, v, out
    d.q = d.k = d.v = d.out = base
    d.ld_q, d.ld_k, d.ld_v, d.ld_out = 8, 10, 8, 8
    assert fn(None, ctypes.byref(d)) == -1 and "pitch" in _lib.last_error()         # a pitch that is no multiple of 16 bytes
    d.ld_k = 8
    assert fn(None, ctypes.byref(d)) == -1 and "lse" in _lib.last_error()           # forward without lse
    d.kv_shared, d.ld_v = 1, 12
    assert fn(None, ctypes.byref(d)) == -1 and "kv_shared" in _lib.last_error()     # shared buffers on two pitches
    d.kv_shared, d.ld_v, d.pass_ = 0, 8, _lib.ATTN_ROWS
    assert fn(None, ctypes.byref(d)) == -1 and "grad_out" in _lib.last_error()      # backward without grad_out
    d.grad_out, d.ld_grad_out, d.lse_delta, d.pass_ = base, 8, base, _lib.ATTN_COLS
    assert fn(None, ctypes.byref(d)) == -1 and "out2" in _lib.last_error()          # cols pass without its second output


def test_descriptor_binding_matches_the_c_struct(tmp_path):
    """_lib.AttnDesc field by field against offsetof / sizeof of dgll_attn_desc as a C compiler lays it out."""
    import subprocess

    from dgll_amd import _lib

    fields = [name for name, _ in _lib.AttnDesc._fields_]
    c_names = ["pass" if f == "pass_" else f for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dgll_hip.h"\nint main(void) {\n'
                   + "".join('    printf("%%zu\\n", offsetof(dgll_attn_desc, %s));\n' % n for n in c_names)
                   + '    printf("%zu\\n", sizeof(dgll_attn_desc));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [getattr(_lib.AttnDesc, f).offset for f in fields] + [ctypes.sizeof(_lib.AttnDesc)]
