"""Typed-edge aggregation and RelGraphConv without a GPU: the float64 restatement against a brute-force loop, the COO builder and the
TypedEdges checks, the layer's logic on host tensors against the restatement, DGL's state-dict names and shapes, and the C entry
point's argument checks (no launch)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from conftest import ROOT
from typed_ref import relgraphconv_reference, typed_spmm_reference


def _coo():
    """6 nodes; parallel edges 1 -> 0 of types 0, 2 and 0 again, an isolated destination (4), a source nobody references as a
    destination's neighbour (5), in scrambled order."""
    src = torch.tensor([1, 3, 1, 2, 1, 0, 3, 2, 4, 0])
    dst = torch.tensor([0, 2, 0, 1, 0, 3, 5, 0, 2, 1])
    ety = torch.tensor([0, 1, 2, 1, 0, 2, 0, 1, 2, 0])
    norm = torch.tensor([.5, 1., .25, 2., 1.5, 1., .75, .5, 1.25, 3.])
    return src, dst, ety, norm


def test_reference_against_a_triple_loop():
    from dgll_amd.ops_typed import typed_graph_from_coo

    src, dst, ety, norm = _coo()
    graph, edges = typed_graph_from_coo(src, dst, ety, norm, 6, 6)
    gen = torch.Generator().manual_seed(0)
    x, coeff = torch.randn(6, 3, generator=gen, dtype=torch.float64), torch.randn(3, 2, generator=gen, dtype=torch.float64)
    want = torch.zeros(6, 2, 3, dtype=torch.float64)
    for e in range(src.numel()):
        for b in range(2):
            for f in range(3):
                want[dst[e], b, f] += norm[e].double() * coeff[ety[e], b] * x[src[e], f]
    got = typed_spmm_reference(graph.rowptr, graph.col, edges.etypes, edges.norm, x, coeff)
    assert torch.allclose(got, want.reshape(6, 6), rtol=0, atol=1e-12)
    assert got[4].abs().max().item() == 0.0


def test_typed_graph_from_coo_keeps_parallel_edges_in_order():
    from dgll_amd.ops_typed import typed_graph_from_coo

    src, dst, ety, norm = _coo()
    graph, edges = typed_graph_from_coo(src, dst, ety, norm, 6, 6)
    assert graph.nnz == 10 and graph.shape == (6, 6) and edges.num_rels == 3
    assert graph.rowptr.tolist() == [0, 4, 6, 8, 9, 9, 10]
    # row 0: the three parallel 1 -> 0 edges in their order of appearance (types 0, 2, 0; norms .5, .25, 1.5), then 2 -> 0
    assert graph.col[:4].tolist() == [1, 1, 1, 2]
    assert edges.etypes[:4].tolist() == [0, 2, 0, 1] and edges.norm[:4].tolist() == [.5, .25, 1.5, .5]
    assert edges.etypes.dtype == torch.int32 and edges.norm.dtype == torch.float32
    # every (dst, src, type, norm) survives the sort
    row = graph.row_index()
    assert sorted(zip(row.tolist(), graph.col.tolist(), edges.etypes.tolist(), edges.norm.tolist())) == \
        sorted(zip(dst.tolist(), src.tolist(), ety.tolist(), norm.tolist()))
    # the cached derived orders
    gt, perm = graph.transpose()
    t_ety, t_norm = edges.transposed()
    assert torch.equal(t_ety, edges.etypes[perm]) and torch.equal(t_norm, edges.norm[perm])
    by = edges.by_type()
    assert by.shape == (3, 10) and by.rowptr.tolist() == [0, 4, 7, 10]
    assert torch.equal(edges.etypes[by.col.long()], torch.tensor([0] * 4 + [1] * 3 + [2] * 3, dtype=torch.int32))
    assert by.col[:4].tolist() == sorted(by.col[:4].tolist())                      # stable
    assert torch.equal(by.val, edges.norm[by.col.long()])


def test_typed_edges_checks():
    from dgll_amd.ops_typed import TypedEdges, typed_graph_from_coo

    src, dst, ety, norm = _coo()
    graph, _ = typed_graph_from_coo(src, dst, ety, norm, 6, 6)
    with pytest.raises(ValueError, match="edge types"):
        TypedEdges(graph, ety, 2)
    with pytest.raises(ValueError, match="edge types"):
        TypedEdges(graph, ety - 1, 3)
    with pytest.raises(ValueError):
        TypedEdges(graph, ety[:-1], 3)
    with pytest.raises(ValueError):
        TypedEdges(graph, ety, 3, norm[:-1])
    with pytest.raises(TypeError):
        TypedEdges(graph, ety.float(), 3)
    assert TypedEdges(graph, ety.to(torch.int16), 3, norm.reshape(-1, 1)).norm.shape == (10,)


def test_typed_spmm_refuses_cpu_tensors():
    from dgll_amd import ops_typed

    src, dst, ety, norm = _coo()
    graph, edges = ops_typed.typed_graph_from_coo(src, dst, ety, norm, 6, 6)
    with pytest.raises(RuntimeError):
        ops_typed.typed_spmm(graph, edges, torch.ones(6, 4), torch.ones(3, 2))


def _random_typed(n_dst, n_src, nnz, R, seed):
    from dgll_amd.ops_typed import typed_graph_from_coo

    gen = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, n_src, (nnz,), generator=gen), torch.randint(0, n_dst - 1, (nnz,), generator=gen)     # last row empty
    ety = torch.randint(0, R, (nnz,), generator=gen)
    norm = torch.rand(nnz, generator=gen) + 0.25
    return typed_graph_from_coo(src, dst, ety, norm, n_src, n_dst, R)


def _layer_reference(layer, graph, edges, feat, activation=None):
    sd = layer.state_dict()
    return relgraphconv_reference(graph.rowptr, graph.col, edges.etypes, edges.norm, feat, sd["linear_r.W"], sd.get("linear_r.coeff"),
                                  sd.get("h_bias"), sd.get("loop_weight"), sd.get("layer_norm_weight.weight"),
                                  sd.get("layer_norm_weight.bias"), activation)


@pytest.mark.parametrize("in_feat", [5, 16])
@pytest.mark.parametrize("regularizer", ["basis", None])
@pytest.mark.parametrize("bias,self_loop,layer_norm", [(True, True, False), (False, False, False), (True, False, True), (False, True, True)])
def test_layer_on_host_tensors(in_feat, regularizer, bias, self_loop, layer_norm):
    from dgll_amd.nn.Convolution import RelGraphConv

    torch.manual_seed(in_feat * 10 + bias)
    R = 4
    graph, edges = _random_typed(12, 12, 60, R, 3)
    layer = RelGraphConv(in_feat, 7, R, regularizer=regularizer, num_bases=3 if regularizer else None, bias=bias, self_loop=self_loop,
                         layer_norm=layer_norm, activation=torch.tanh).double()
    if bias:
        torch.nn.init.normal_(layer.h_bias)
    feat = torch.randn(12, in_feat, dtype=torch.float64)
    got = layer(graph, feat, edges)
    want = _layer_reference(layer, graph, edges, feat, torch.tanh)
    assert got.shape == (12, 7) and torch.allclose(got, want, rtol=1e-10, atol=1e-10)
    # the same through raw etypes / norm tensors
    assert torch.equal(layer(graph, feat, edges.etypes, edges.norm), got)


def test_layer_on_a_rectangular_host_graph():
    from dgll_amd.nn.Convolution import RelGraphConv

    torch.manual_seed(1)
    graph, edges = _random_typed(5, 12, 40, 3, 4)
    layer = RelGraphConv(6, 4, 3, regularizer="basis", num_bases=2).double()
    feat = torch.randn(12, 6, dtype=torch.float64)
    got = layer(graph, feat, edges, presorted=True)
    assert got.shape == (5, 4) and torch.allclose(got, _layer_reference(layer, graph, edges, feat), rtol=1e-10, atol=1e-10)


def test_state_dict_names_and_shapes():
    from dgll_amd.nn.Convolution import RGCN, RelGraphConv

    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}      # noqa: E731
    assert shapes(RelGraphConv(10, 6, 5, regularizer="basis", num_bases=3, layer_norm=True)) == {
        "linear_r.W": (3, 10, 6), "linear_r.coeff": (5, 3), "h_bias": (6,), "loop_weight": (10, 6),
        "layer_norm_weight.weight": (6,), "layer_norm_weight.bias": (6,)}
    assert shapes(RelGraphConv(10, 6, 5)) == {"linear_r.W": (5, 10, 6), "h_bias": (6,), "loop_weight": (10, 6)}
    assert shapes(RelGraphConv(10, 6, 5, regularizer="basis", num_bases=2, bias=False, self_loop=False)) == {
        "linear_r.W": (2, 10, 6), "linear_r.coeff": (5, 2)}
    layer = RelGraphConv(10, 6, 5, regularizer="basis", num_bases=3)
    assert layer.linear_r.W.abs().max().item() <= 10 ** -0.5 and layer.h_bias.abs().max().item() == 0.0
    model = RGCN(10, 8, 3, 5, 2)
    assert len(model.layers) == 2 and "layers.1.linear_r.coeff" in model.state_dict()


def test_unsupported_regularisers_raise():
    from dgll_amd.nn.Convolution import RelGraphConv, relgraphconv

    with pytest.raises(NotImplementedError, match="bdd"):
        RelGraphConv(8, 8, 4, regularizer="bdd", num_bases=2)
    RelGraphConv(8, 8, relgraphconv._MAX_DIRECT_RELS)
    with pytest.raises(NotImplementedError, match="basis"):
        RelGraphConv(8, 8, relgraphconv._MAX_DIRECT_RELS + 1)


def test_names_are_exported():
    import dgll
    from dgll_amd.nn import Convolution as conv

    assert "RelGraphConv" in conv.__all__ and "RGCN" in conv.__all__
    assert dgll.nn.Convolution.RelGraphConv is conv.RelGraphConv
    import dgll.nn.Convolution.relgraphconv as mod
    assert mod.RGCN is conv.RGCN


def test_synthetic_typed_graph():
    from dgll_amd import synth
    from dgll_amd.ops_typed import typed_graph_from_coo

    d = synth.typed_graph(7, num_rels=5, reverse=True, seed=2)
    d2 = synth.typed_graph(7, num_rels=5, reverse=True, seed=2)
    assert all(torch.equal(d[k], d2[k]) for k in ("src", "dst", "etypes", "norm", "labels")) and d["num_rels"] == 10
    graph, edges = typed_graph_from_coo(d["src"], d["dst"], d["etypes"], d["norm"], d["num_nodes"], d["num_nodes"], d["num_rels"])
    # norm = 1 / c_{i, r}: the norms of a node's edges of one type sum to 1
    key = graph.row_index() * 10 + edges.etypes.long()
    sums = torch.zeros(128 * 10, dtype=torch.float64).index_add_(0, key, edges.norm.double())
    assert torch.allclose(sums[sums > 0], torch.ones(int((sums > 0).sum()), dtype=torch.float64), atol=1e-6)
    counts = torch.bincount(d["etypes"][:d["etypes"].numel() // 2], minlength=5)
    assert counts[0] > counts[4]                                                    # skewed
    assert d["labels"].unique().numel() > 1


# ---- the C entry point without a device ------------------------------------------------------------------------------------------
def _desc(**kw):
    from dgll_amd import _lib

    d = _lib.TypedDesc()
    d.pass_, d.dtype = _lib.TYPED_EXPAND, _lib.F32
    d.rowptr = d.col = d.etype = d.coeff = d.x = d.out = d.dz = d.p = 64            # never dereferenced: the checks come first
    d.n_rows, d.n_cols, d.R, d.B, d.F = 4, 4, 3, 2, 8
    d.ld_x, d.ld_out, d.ld_dz, d.ld_p = 8, 16, 16, 4
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_entry_point_symbol_and_struct_size(tmp_path):
    from dgll_amd import _lib

    assert hasattr(_lib.lib, "dgll_hip_typed_spmm_pass") and "dgll_hip_typed_spmm_pass" in _lib.SIGNATURES
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "dgll_hip.h"\nint main(void) { printf("%zu %d %d %d %d %d %d\\n", sizeof(dgll_typed_desc), '
                   'DGLL_TYPED_EXPAND, DGLL_TYPED_CONTRACT, DGLL_TYPED_EDGE_DOTS, DGLL_TYPED_LONG_ROW, DGLL_TYPED_COEFF_LDS, '
                   'DGLL_TYPED_BASIS_BLOCK); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.run(["gcc", "-std=c99", str(src), "-I", os.path.join(ROOT, "include"), "-o", exe], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.TypedDesc), _lib.TYPED_EXPAND, _lib.TYPED_CONTRACT, _lib.TYPED_EDGE_DOTS, _lib.TYPED_LONG_ROW,
                   _lib.TYPED_COEFF_LDS, _lib.TYPED_BASIS_BLOCK]


@pytest.mark.parametrize("bad", [dict(x=None), dict(rowptr=None), dict(etype=None), dict(out=None), dict(ld_x=6), dict(ld_out=12), dict(x=68),
                                 dict(B=0), dict(R=0), dict(F=6), dict(pass_=7), dict(dtype=5), dict(n_rows=1 << 31),
                                 dict(pass_=1, ld_dz=12), dict(pass_=2, ld_p=2), dict(pass_=2, p=None)],
                         ids=lambda b: ",".join("%s=%s" % kv for kv in b.items()))
def test_entry_point_rejects_bad_descriptors(bad):
    from dgll_amd import _lib

    code = _lib.lib.dgll_hip_typed_spmm_pass(None, C.byref(_desc(**bad)))
    assert code == -1 and "dgll_hip_typed_spmm_pass" in _lib.last_error()


def test_entry_point_rejects_a_null_descriptor():
    from dgll_amd import _lib

    assert _lib.lib.dgll_hip_typed_spmm_pass(None, None) == -1 and "dgll_hip_typed_spmm_pass" in _lib.last_error()
