"""Edge-gated aggregation without a GPU: gated_ref.py against float64 autograd of the index_add_ composition, the binding of
dgll_gated_desc and the host-side argument checks of dgll_hip_gated_pass, the refusals of dgll_amd.ops_gated.gated_sum (names,
dtypes and shapes first, then that the tensors are on the GPU, so both are checked here), and nn.GatedGCNConv / GatedGCN: names,
state dict, blocks, and the host path term by term."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gated_ref
from conftest import ROOT

INVALID = -1        # DGLL_ERR_INVALID
EPS = 1e-6


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

@pytest.mark.parametrize("with_ge", [False, True], ids=["noge", "ge"])
def test_the_reference_agrees_with_autograd_of_the_composition(with_ge):
    """gated_ref.forward / gradients (written out entry by entry) against float64 autograd of the index_add_ composition, on a block
    with an empty row, a column listed five times and unreferenced sources."""
    g = _block()
    gen = torch.Generator().manual_seed(1)
    mk = lambda n: torch.randn(n, 5, generator=gen, dtype=torch.float64, requires_grad=True)      # noqa: E731
    a, b, c, v = mk(9), mk(12), mk(g.nnz), mk(12)
    go, ge = torch.randn(9, 5, generator=gen, dtype=torch.float64), torch.randn(g.nnz, 5, generator=gen, dtype=torch.float64)
    out, ehat = gated_ref.composition(g.rowptr, g.col, a, b, c, v, EPS)
    loss = (out * go).sum() + ((ehat * ge).sum() if with_ge else 0.0)
    want = torch.autograd.grad(loss, (a, b, c, v))
    ins = [t.detach() for t in (a, b, c, v)]
    ref_out, ref_ehat = gated_ref.forward(g.rowptr, g.col, *ins, EPS)
    _close("out", ref_out, out.detach(), 1e-12)
    _close("ehat", ref_ehat, ehat.detach(), 1e-12)
    assert ref_out[4].abs().max().item() == 0.0                                     # the empty row
    for name, x, y in zip("abcv", gated_ref.gradients(g.rowptr, g.col, *ins, EPS, go, ge if with_ge else None), want):
        _close("grad_" + name, x, y, 1e-12)


# ---- the C entry point -----------------------------------------------------------------------------------------------------------

def test_descriptor_binding_matches_the_c_struct(tmp_path):
    """_lib.GatedDesc field by field against offsetof / sizeof of dgll_gated_desc as a C compiler lays it out, and in the header's order."""
    import subprocess

    from dgll_amd import _lib

    fields = [name for name, _ in _lib.GatedDesc._fields_]
    c_names = ["pass" if f == "pass_" else f for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dgll_hip.h"\nint main(void) {\n'
                   + "".join('    printf("%%zu\\n", offsetof(dgll_gated_desc, %s));\n' % n for n in c_names)
                   + '    printf("%zu\\n", sizeof(dgll_gated_desc));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [getattr(_lib.GatedDesc, f).offset for f in fields] + [ctypes.sizeof(_lib.GatedDesc)]
    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    body = re.search(r"typedef struct dgll_gated_desc \{(.*?)\} dgll_gated_desc;", text, re.S).group(1)
    assert re.findall(r"(\w+);", body) == c_names                                   # every member, in the header's order


def test_constants_match_the_header():
    from dgll_amd import _lib, ops_gated

    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    assert int(re.search(r"#define\s+DGLL_GATED_LONG_ROW\s+(\d+)", text).group(1)) == ops_gated.LONG_ROW == _lib.GATED_LONG_ROW == 256
    for name in ("FORWARD", "ROWS", "COLS"):
        assert int(re.search(r"DGLL_GATED_%s\s*=\s*(\d+)" % name, text).group(1)) == getattr(_lib, "GATED_" + name)
    assert _lib.lib.dgll_hip_abi_version() == 2                                     # an addition: the ABI version stays


_MATS = ("a", "b", "c", "v", "out", "ehat", "inv_s", "out32", "grad_out", "grad_ehat", "grad_c", "grad_a", "w", "grad_b", "grad_v")
# pass -> the operands it requires in its full form (grad_ehat is optional)
_READS = {0: ("a", "b", "c", "v", "out", "ehat", "inv_s", "out32"),
          1: ("grad_out", "inv_s", "out32", "v", "ehat", "grad_c", "grad_a"),
          2: ("grad_c", "grad_b", "ehat", "w", "grad_v")}


def _valid(kind):
    """A descriptor that passes every check of the pass, with n_rows == 0 so that nothing is launched (the pointers are only
    inspected, never followed, before the checks pass)."""
    from dgll_amd import _lib

    buf = (ctypes.c_float * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    d = _lib.GatedDesc()
    d._keep = buf
    d.pass_, d.dtype, d.F, d.n_rows, d.n_cols, d.nnz, d.eps = kind, _lib.F32, 8, 0, 4, 5, 1e-6
    d.rowptr = d.col = d.perm = base
    for m in _MATS:
        setattr(d, m, base)
        setattr(d, "ld_" + m, 12 if m in ("c", "ehat", "grad_c") else 8)           # the per-edge matrices on a pitch of their own
    return d


def _refused(d, *words):
    from dgll_amd import _lib

    code = _lib.lib.dgll_hip_gated_pass(None, ctypes.byref(d))
    msg = _lib.last_error()
    assert code == INVALID and all(w in msg for w in words), (code, words, msg)


def test_pass_arguments_are_checked_on_the_host():
    from dgll_amd import _lib

    fn = _lib.lib.dgll_hip_gated_pass
    assert fn(None, None) == INVALID and "NULL" in _lib.last_error()                # a NULL descriptor
    for kind in range(3):                                                           # n_rows == 0: nothing to do, and nothing launched
        assert fn(None, ctypes.byref(_valid(kind))) == _lib.OK, (kind, _lib.last_error())
    for bad in (3, -1):
        d = _valid(0)
        d.pass_ = bad
        _refused(d, "pass")
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
    d.eps = 0.0
    _refused(d, "eps")
    d = _valid(0)
    d.nnz = 1 << 31
    _refused(d, "nnz")
    d = _valid(2)
    d.perm = None
    _refused(d, "perm must be non-NULL")
    for kind, reads in _READS.items():
        for m in reads:
            if (kind, m) in ((1, "grad_c"), (1, "grad_a")):
                continue                                                            # these two go together: below
            d = _valid(kind)
            setattr(d, m, None)
            if kind == 2 and m in ("grad_b", "grad_v"):                             # either output alone is a valid pass
                assert fn(None, ctypes.byref(d)) == _lib.OK, (m, _lib.last_error())
                continue
            _refused(d, m + " must be non-NULL")
            d = _valid(kind)
            setattr(d, m, getattr(d, m) + 4)                                        # a misaligned base
            _refused(d, m + " must be 16-byte aligned")
            d = _valid(kind)
            setattr(d, "ld_" + m, 4)                                                # a pitch shorter than F
            _refused(d, "ld_" + m)
            d = _valid(kind)
            setattr(d, "ld_" + m, 10)                                               # a pitch that is not whole vectors
            _refused(d, "ld_" + m)
    d = _valid(1)
    d.grad_ehat += 4                                                                # optional, but checked when given
    _refused(d, "grad_ehat must be 16-byte aligned")


def test_operands_a_pass_does_not_read_may_be_null():
    from dgll_amd import _lib

    fn = _lib.lib.dgll_hip_gated_pass
    for kind, reads in _READS.items():
        d = _valid(kind)
        for m in _MATS:
            if m not in reads:
                setattr(d, m, None)
        assert fn(None, ctypes.byref(d)) == _lib.OK, (kind, _lib.last_error())
    # rows: grad_c and grad_a go together; without both the pass only leaves w and reads no per-edge operand
    for m in ("grad_c", "grad_a"):
        d = _valid(1)
        setattr(d, m, None)
        _refused(d, "go together")
    d = _valid(1)
    for m in _MATS:
        if m not in ("grad_out", "inv_s", "out32", "w"):
            setattr(d, m, None)
    assert fn(None, ctypes.byref(d)) == _lib.OK, _lib.last_error()
    d.w = None
    _refused(d, "nothing to write")
    d = _valid(2)
    d.grad_b = d.grad_v = None
    _refused(d, "nothing to write")
    d = _valid(2)                                                                   # cols with grad_v alone reads neither grad_c ...
    d.grad_b = d.grad_c = None
    assert fn(None, ctypes.byref(d)) == _lib.OK, _lib.last_error()
    d = _valid(2)                                                                   # ... and with grad_b alone neither ehat nor w
    d.grad_v = d.ehat = d.w = None
    assert fn(None, ctypes.byref(d)) == _lib.OK, _lib.last_error()


# ---- dgll_amd.ops_gated ------------------------------------------------------------------------------------------------------------

def test_op_refusals():
    from dgll_amd import ops_gated

    g = _block()
    a, b, c, v = torch.randn(9, 8), torch.randn(12, 8), torch.randn(g.nnz, 8), torch.randn(12, 8)
    with pytest.raises(TypeError):
        ops_gated.gated_sum(torch.eye(6), a, b, c, v)                               # not a CSRGraph
    with pytest.raises(TypeError):
        ops_gated.gated_sum(g, a, b, c.bfloat16(), v)                               # two dtypes
    with pytest.raises(TypeError):
        ops_gated.gated_sum(g, a.double(), b.double(), c.double(), v.double())      # not a kernel dtype
    with pytest.raises(ValueError, match="destinations"):
        ops_gated.gated_sum(g, b, b, c, v)                                          # rows of a
    with pytest.raises(ValueError, match="b must be"):
        ops_gated.gated_sum(g, a, a, c, v)                                          # rows of b
    with pytest.raises(ValueError, match="v must be"):
        ops_gated.gated_sum(g, a, b, c, v[:-1])
    with pytest.raises(ValueError, match="nnz"):
        ops_gated.gated_sum(g, a, b, c[:-1], v)
    with pytest.raises(ValueError):
        ops_gated.gated_sum(g, a, b, c.reshape(-1), v)                              # not a matrix
    with pytest.raises(ValueError, match="one width"):
        ops_gated.gated_sum(g, a, b, c[:, :4], v)
    with pytest.raises(ValueError, match="one width"):
        ops_gated.gated_sum(g, a, b[:, :4], c, v)
    with pytest.raises(ValueError, match="the layers pad"):
        ops_gated.gated_sum(g, a[:, :6], b[:, :6], c[:, :6], v[:, :6])              # F = 6
    with pytest.raises(ValueError, match="the layers pad"):
        ops_gated.gated_sum(g, *(t.bfloat16()[:, :4] for t in (a, b, c, v)))
    with pytest.raises(ValueError, match="eps"):
        ops_gated.gated_sum(g, a, b, c, v, eps=0.0)
    with pytest.raises(RuntimeError, match="GPU"):                                  # everything else is right: CPU tensors
        ops_gated.gated_sum(g, a, b, c, v)


# ---- the layer ---------------------------------------------------------------------------------------------------------------------

def test_layer_names_state_dict_and_exports():
    import dgll
    import dgll_amd.nn
    from dgll.nn.Convolution.gatedgcnconv import GatedGCNConv as alias
    from dgll_amd.nn import Convolution as conv

    assert {"GatedGCNConv", "GatedGCN"} <= set(conv.__all__) and {"GatedGCNConv", "GatedGCN"} <= set(dgll_amd.nn.__all__)
    assert alias is conv.GatedGCNConv and dgll.nn.Convolution.GatedGCNConv is conv.GatedGCNConv
    assert dgll_amd.nn.GatedGCNConv is conv.GatedGCNConv and dgll_amd.nn.GatedGCN is conv.GatedGCN and dgll.nn.GatedGCN is conv.GatedGCN

    layer = conv.GatedGCNConv(5, 3, 7)
    bn = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
    assert set(layer.state_dict()) == ({"%s.%s" % (m, s) for m in "ABCDE" for s in ("weight", "bias")}
                                       | {"%s.%s" % (m, s) for m in ("bn_node", "bn_edge") for s in bn})
    assert [getattr(layer, m).weight.shape for m in "ABCDE"] == [(7, 5), (7, 5), (7, 3), (7, 5), (7, 5)]
    assert layer.bn_node.num_features == 7 and layer.bn_edge.num_features == 7 and layer.dropout.p == 0
    # residual silently turns off on a width mismatch
    assert not layer.residual and not conv.GatedGCNConv(7, 3, 7).residual and not conv.GatedGCNConv(3, 7, 7).residual
    assert conv.GatedGCNConv(7, 7, 7).residual and not conv.GatedGCNConv(7, 7, 7, residual=False).residual

    model = conv.GatedGCN(5, 3, 8, 4, layers=3)
    assert len(model.convs) == 3 and all(c.residual for c in model.convs)
    assert model.embed_h.weight.shape == (8, 5) and model.embed_e.weight.shape == (8, 3) and model.cls.weight.shape == (4, 8)


def _by_hand(layer, g, h_src, h_dst, e_in, training):
    """the layer's forward, term by term, from its state dict (float64)"""
    sd = {k: v.detach().double() for k, v in layer.state_dict().items()}
    lin = lambda x, m: x.double() @ sd[m + ".weight"].t() + sd[m + ".bias"]        # noqa: E731
    out, ehat = gated_ref.forward(g.rowptr, g.col, lin(h_dst, "E"), lin(h_src, "D"), lin(e_in, "C"), lin(h_src, "B"), EPS)
    h, e = lin(h_dst, "A") + out, ehat
    if layer.batch_norm:
        def bn(x, m):
            mean, var = (x.mean(0), x.var(0, unbiased=False)) if training else (sd[m + ".running_mean"], sd[m + ".running_var"])
            return (x - mean) / torch.sqrt(var + 1e-5) * sd[m + ".weight"] + sd[m + ".bias"]
        h, e = bn(h, "bn_node"), bn(e, "bn_edge")
    h, e = torch.relu(h), torch.relu(e)
    if layer.residual:
        h, e = h_dst.double() + h, e_in.double() + e
    return h, e


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("widths", [(6, 6, 6), (6, 4, 6), (5, 3, 7)], ids=["residual", "edge-mismatch", "all-differ"])
def test_host_path_term_by_term(widths, training):
    from dgll_amd.nn.Convolution import GatedGCNConv

    g = _graph(_SQUARE, 6)
    fin, fe, fout = widths
    gen = torch.Generator().manual_seed(sum(widths))
    torch.manual_seed(7)
    layer = GatedGCNConv(fin, fe, fout)
    assert layer.residual == (fin == fout == fe)
    with torch.no_grad():                                                           # running statistics and affine terms off their defaults
        for bn in (layer.bn_node, layer.bn_edge):
            bn.running_mean.copy_(0.3 * torch.randn(fout, generator=gen))
            bn.running_var.copy_(0.5 + torch.rand(fout, generator=gen))
            bn.weight.copy_(1.0 + 0.2 * torch.randn(fout, generator=gen))
            bn.bias.copy_(0.1 * torch.randn(fout, generator=gen))
    layer.train(training)
    h, e_in = torch.randn(6, fin, generator=gen), torch.randn(g.nnz, fe, generator=gen)
    want_h, want_e = _by_hand(layer, g, h, h, e_in, training)                       # before the forward updates the running statistics
    got_h, got_e = layer(g, h, e_in)
    assert got_h.shape == (6, fout) and got_e.shape == (g.nnz, fout) and got_h.dtype == torch.float32
    _close("h", got_h, want_h, 1e-5)
    _close("e", got_e, want_e, 1e-5)
    # without batch norm and activation the outputs are the bare formula: A h + out, ehat
    bare = GatedGCNConv(fin, fe, fout, batch_norm=False, residual=False, activation=None)
    bare.load_state_dict(layer.state_dict())
    sd = {k: v.detach().double() for k, v in layer.state_dict().items()}
    lin = lambda x, m: x.double() @ sd[m + ".weight"].t() + sd[m + ".bias"]        # noqa: E731
    out, ehat = gated_ref.forward(g.rowptr, g.col, lin(h, "E"), lin(h, "D"), lin(e_in, "C"), lin(h, "B"), EPS)
    bh, be = bare(g, h, e_in)
    _close("bare h", bh, lin(h, "A") + out, 1e-5)
    _close("bare e", be, ehat, 1e-5)
    assert torch.allclose(bh[2].double(), lin(h, "A")[2], atol=1e-6)                # the row without entries: A h alone


def test_pair_on_a_rectangular_block_and_dropout():
    from dgll_amd.nn.Convolution import GatedGCNConv

    g = _block()
    gen = torch.Generator().manual_seed(4)
    torch.manual_seed(4)
    layer = GatedGCNConv(6, 6, 6).eval()
    h_src, h_dst, e_in = torch.randn(12, 6, generator=gen), torch.randn(9, 6, generator=gen), torch.randn(g.nnz, 6, generator=gen)
    got_h, got_e = layer(g, (h_src, h_dst), e_in)
    want_h, want_e = _by_hand(layer, g, h_src, h_dst, e_in, False)
    assert got_h.shape == (9, 6) and got_e.shape == (g.nnz, 6)
    _close("h", got_h, want_h, 1e-5)
    _close("e", got_e, want_e, 1e-5)
    # a tensor on a block: the destinations are the first n_dst sources
    both = torch.cat([h_dst, h_src[9:]], 0)
    for x, y in zip(layer(g, both, e_in), layer(g, (both, both[:9]), e_in)):
        assert torch.equal(x, y)
    with pytest.raises(ValueError):
        layer(g, (h_src, h_dst), e_in[:-1])
    with pytest.raises(TypeError):
        layer(g, (h_src, h_dst), e_in.double())
    with pytest.raises(ValueError):
        layer(g, h_src[:5], e_in)
    # dropout applies to both outputs in training, to neither in eval
    drop = GatedGCNConv(6, 6, 6, dropout=0.5)
    drop.load_state_dict(layer.state_dict())
    eh, ee = drop.eval()(g, (h_src, h_dst), e_in)
    assert torch.equal(eh, got_h) and torch.equal(ee, got_e)
    dh, de = drop.train()(g, (h_src, h_dst), e_in)
    assert (dh == 0).any() and (de == 0).any()


def test_model_host_path_runs_and_trains_every_parameter():
    from dgll_amd.nn.Convolution import GatedGCN

    g = _graph(_SQUARE, 6)
    gen = torch.Generator().manual_seed(2)
    torch.manual_seed(2)
    model = GatedGCN(6, 3, 8, 4, layers=2)
    x, attr = torch.randn(6, 6, generator=gen), torch.randn(g.nnz, 3, generator=gen)
    out = model(g, x, attr)
    assert out.shape == (6, 4)
    out.square().sum().backward()
    used = [(n, p) for n, p in model.named_parameters() if not n.startswith("convs.1.bn_edge")]    # the last edge output is dropped
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for _, p in used)
    assert float(model.convs[1].C.weight.grad.abs().max()) > 0                      # the last layer's edge projection still gates h
    assert float(model.embed_e.weight.grad.abs().max()) > 0                         # the edge attributes reach the loss
    assert float(model.convs[0].bn_edge.weight.grad.abs().max()) > 0                # ... through the first layer's edge output
