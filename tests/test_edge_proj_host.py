"""The fused edge projection without a GPU: the binding of dgll_edge_proj_desc, the host-side argument checks of
dgll_hip_edge_proj_pass, the refusals of dgll_amd.ops_efp.u_op_proj_e_sum (names, dtypes and shapes first, then that the tensors are
on the GPU, so both are checked here), efp_ref.py against float64 autograd, and nn.GINEConv(edge_dim=) / GINE(fused_edge=): state
dicts, and the host path in fp32 against efp_ref.py at 1e-6 max |ref|, forward and parameter gradients."""
import ctypes
import os
import re

import pytest
import torch

import efp_ref
from conftest import ROOT
from test_edge_feat_host import _SQUARE, _block, _close, _graph

INVALID = -1        # DGLL_ERR_INVALID


# ---- the C entry point -----------------------------------------------------------------------------------------------------------

def test_descriptor_binding_matches_the_c_struct(tmp_path):
    """_lib.EdgeProjDesc field by field against offsetof / sizeof of dgll_edge_proj_desc as a C compiler lays it out."""
    import subprocess

    from dgll_amd import _lib

    fields = [name for name, _ in _lib.EdgeProjDesc._fields_]
    c_names = ["pass" if f == "pass_" else f for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dgll_hip.h"\nint main(void) {\n'
                   + "".join('    printf("%%zu\\n", offsetof(dgll_edge_proj_desc, %s));\n' % n for n in c_names)
                   + '    printf("%zu\\n", sizeof(dgll_edge_proj_desc));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [getattr(_lib.EdgeProjDesc, f).offset for f in fields] + [ctypes.sizeof(_lib.EdgeProjDesc)]
    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    body = re.search(r"typedef struct dgll_edge_proj_desc \{(.*?)\} dgll_edge_proj_desc;", text, re.S).group(1)
    assert re.findall(r"(\w+);", body) == c_names                                   # every field, in the header's order


def test_constants_match_the_header():
    from dgll_amd import _lib, ops_efp

    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    define = lambda name: int(re.search(r"#define\s+DGLL_EFP_%s\s+(\d+)" % name, text).group(1))      # noqa: E731
    assert define("LONG_ROW") == ops_efp.LONG_ROW == _lib.EFP_LONG_ROW == 256
    assert define("MAX_DE") == ops_efp.MAX_DE == _lib.EFP_MAX_DE == 16
    assert define("MAX_PARTIALS") == _lib.EFP_MAX_PARTIALS == 512
    for name in ("FORWARD", "COLS", "PARAM", "DOTS"):
        assert int(re.search(r"DGLL_EFP_%s\s*=\s*(\d+)" % name, text).group(1)) == getattr(_lib, "EFP_" + name)
    assert ops_efp._TAGS == ("efp_forward", "efp_cols", "efp_param", "efp_dots")
    assert _lib.lib.dgll_hip_abi_version() == 2                                     # an addition: the ABI version stays


def _valid(kind, op):
    """A descriptor that passes every check of (kind, op), with n_rows == 0 so that nothing is launched (the pointers are only
    inspected, never followed, before the checks pass)."""
    from dgll_amd import _lib

    buf = (ctypes.c_float * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    d = _lib.EdgeProjDesc()
    d._keep = buf
    d.pass_, d.dtype, d.op, d.De, d.F, d.n_rows, d.n_cols, d.nnz = kind, _lib.F32, op, 3, 8, 0, 4, 5
    d.rowptr = d.col = d.perm = d.scale = d.x = d.a = d.weight = d.bias = d.grad_out = d.out = d.grad_x = d.grad_a = base
    d.dots_part = d.slabs = base
    d.partials = 2
    d.ld_x = d.ld_grad_out = d.ld_out = d.ld_grad_x = 8
    d.ld_a = d.ld_grad_a = 4
    return d


def _refused(d, *words):
    from dgll_amd import _lib

    code = _lib.lib.dgll_hip_edge_proj_pass(None, ctypes.byref(d))
    msg = _lib.last_error()
    assert code == INVALID and all(w in msg for w in words), (code, words, msg)


_PAIRS = [(k, o) for k in range(4) for o in range(3) if (k, o) != (1, 0)]           # COLS of ADD is the edge-feature pass's


def test_pass_arguments_are_checked_on_the_host():
    from dgll_amd import _lib

    fn = _lib.lib.dgll_hip_edge_proj_pass
    assert fn(None, None) == INVALID and "NULL" in _lib.last_error()                # a NULL descriptor
    for kind, op in _PAIRS:                                                         # n_rows == 0: nothing to do, and nothing launched
        assert fn(None, ctypes.byref(_valid(kind, op))) == _lib.OK, (kind, op, _lib.last_error())
    _refused(_valid(_lib.EFP_COLS, _lib.EF_ADD), "cols", "DGLL_EF_ADD")
    for field, bad in (("pass_", 4), ("pass_", -1), ("op", 3), ("op", -1)):
        d = _valid(0, 0)
        setattr(d, field, bad)
        _refused(d, field.rstrip("_"))
    for bad in (0, -1, 17):
        d = _valid(0, 0)
        d.De = bad
        _refused(d, "De", "16")
    for bad in (0, -1, _lib.EFP_MAX_PARTIALS + 1):
        d = _valid(_lib.EFP_PARAM, 0)
        d.partials = bad
        _refused(d, "partials", "512")
    d = _valid(_lib.EFP_PARAM, 0)
    d.slabs = None
    _refused(d, "slabs")
    for field in ("rowptr", "col"):                                                 # NULL CSR arrays
        d = _valid(0, 0)
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
    d.a += 4                                                                        # a misaligned base
    _refused(d, "a must be 16-byte aligned")
    d = _valid(0, 0)
    d.weight += 4
    _refused(d, "weight", "16-byte aligned")
    d = _valid(0, 0)
    d.bias += 4
    _refused(d, "bias", "16-byte aligned")
    d = _valid(0, 0)
    d.De, d.ld_a = 5, 4                                                             # a pitch shorter than De
    _refused(d, "ld_a")
    d = _valid(0, 0)
    d.ld_a = 6                                                                      # a pitch that is not whole vectors
    _refused(d, "ld_a")
    d = _valid(_lib.EFP_DOTS, 0)
    d.ld_grad_a = 2
    _refused(d, "ld_grad_a")
    d = _valid(_lib.EFP_DOTS, 0)
    d.F, d.dots_part = 260, None                                                    # two column blocks: the partial dots are required
    d.ld_x = d.ld_grad_out = 260
    _refused(d, "dots_part")
    d.dots_part, d.grad_a = d.slabs, None                                           # ... and grad_a is then not written
    assert fn(None, ctypes.byref(d)) == _lib.OK, _lib.last_error()


# (pass, op) -> the operands it reads, of x / a / weight / perm (include/dgll_hip.h); bias may always be NULL
_READS = {(0, 0): "xaw", (0, 1): "xaw", (0, 2): "xaw",
          (1, 1): "xawp", (1, 2): "awp",
          (2, 0): "a", (2, 1): "xaw", (2, 2): "xa",
          (3, 0): "w", (3, 1): "xaw", (3, 2): "xw"}
_FIELD = (("x", "x"), ("a", "a"), ("w", "weight"), ("p", "perm"))


@pytest.mark.parametrize("kind,op", sorted(_READS))
def test_operands_a_pass_reads_are_required_and_the_others_may_be_null(kind, op):
    from dgll_amd import _lib

    reads = _READS[(kind, op)]
    d = _valid(kind, op)                                                            # all that the pass does not read: NULL
    for letter, field in _FIELD:
        if letter not in reads:
            setattr(d, field, None)
    d.scale = d.bias = None
    for field in {0: ("grad_out", "grad_x", "grad_a", "dots_part", "slabs"), 1: ("out", "grad_a", "dots_part", "slabs"),
                  2: ("out", "grad_x", "grad_a", "dots_part"), 3: ("out", "grad_x", "dots_part", "slabs")}[kind]:
        setattr(d, field, None)
    assert _lib.lib.dgll_hip_edge_proj_pass(None, ctypes.byref(d)) == _lib.OK, _lib.last_error()
    for letter, field in _FIELD:
        if letter in reads:
            d = _valid(kind, op)
            setattr(d, field, None)
            _refused(d, field, "non-NULL")
    for field in {0: ("out",), 1: ("grad_out", "grad_x"), 2: ("grad_out", "slabs"), 3: ("grad_out", "grad_a")}[kind]:
        d = _valid(kind, op)
        setattr(d, field, None)
        _refused(d, field, "non-NULL")


# ---- dgll_amd.ops_efp ----------------------------------------------------------------------------------------------------------------

def test_op_refusals():
    from dgll_amd import ops_efp

    g = _graph(_SQUARE, 6)
    x, a, w, b = torch.randn(6, 8), torch.randn(g.nnz, 3), torch.randn(8, 3), torch.randn(8)
    f = ops_efp.u_op_proj_e_sum
    with pytest.raises(TypeError, match="CSRGraph"):
        f(torch.eye(6), x, a, w, b)
    with pytest.raises(TypeError, match="one dtype"):
        f(g, x, a.bfloat16(), w, b)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        f(g, x.double(), a.double(), w, b)
    with pytest.raises(ValueError, match="x must be a matrix of 6 rows"):
        f(g, x[:5], a, w, b)
    with pytest.raises(ValueError, match=r"a must be \[nnz, De\]"):
        f(g, x, a[:-1], w, b)
    with pytest.raises(ValueError, match="the layers pad"):
        f(g, x[:, :6], a, w[:6], b[:6])                                             # F = 6
    with pytest.raises(ValueError, match="the layers pad"):
        f(g, x.bfloat16()[:, :4], a.bfloat16(), w[:4], b[:4])
    with pytest.raises(ValueError, match=r"1\.\.16"):
        f(g, x, torch.randn(g.nnz, 17), torch.randn(8, 17), b)                      # De past the limit, named
    with pytest.raises(ValueError, match=r"1\.\.16"):
        f(g, x, torch.randn(g.nnz, 0), torch.randn(8, 0), b)
    with pytest.raises(ValueError, match=r"weight must be a floating-point \[F, De\] = \[8, 3\]"):
        f(g, x, a, w.t(), b)                                                        # [De, F]: not Linear's layout
    with pytest.raises(ValueError, match="weight"):
        f(g, x, a, w[:, :2], b)
    with pytest.raises(ValueError, match=r"bias must be None or a floating-point \[F\] = \[8\]"):
        f(g, x, a, w, b[:4])
    with pytest.raises(ValueError, match="relu"):
        f(g, x, a, w, b, op="mul", act="relu")
    with pytest.raises(ValueError, match="op must be"):
        f(g, x, a, w, b, op="sub")
    with pytest.raises(ValueError, match="act must be"):
        f(g, x, a, w, b, act="elu")
    with pytest.raises(ValueError, match="max / min"):
        f(g, x, a, w, b, reduce="max")
    for call in (lambda: f(g, x, a, w, b), lambda: f(g, x, a, w, None, "add", "relu", "mean"), lambda: f(g, x, a, w, b, "mul")):
        with pytest.raises(RuntimeError, match="GPU"):                              # everything else is right: CPU tensors
            call()


def test_geometry_matches_the_row_tile_layout():
    from dgll_amd import ops_efp

    assert ops_efp.geometry(24, 4, torch.float32) == (1, 1)                         # 8 lanes a row, 32 rows a tile
    assert ops_efp.geometry(1024, 64, torch.float32) == (64, 1)                     # 16 lanes a row, 16 rows a tile
    assert ops_efp.geometry(9, 260, torch.float32) == (3, 2) and ops_efp.geometry(9, 520, torch.bfloat16) == (3, 2)
    assert ops_efp.geometry(0, 8, torch.bfloat16) == (0, 1)


def test_the_reference_agrees_with_itself():
    """efp_ref.gradients (entry by entry through ef_ref.gradients) is the autograd gradient of efp_ref.forward, for all five inputs."""
    g = _block()
    gen = torch.Generator().manual_seed(0)
    for op in efp_ref.OPS:
        for reduce in ("sum", "mean"):
            mk = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64, requires_grad=True)      # noqa: E731
            x, a, W, b = mk(12, 5), mk(g.nnz, 3), mk(5, 3), mk(5)
            go = torch.randn(9, 5, generator=gen, dtype=torch.float64)
            got = torch.autograd.grad(efp_ref.forward(g.rowptr, g.col, x, a, W, b, op, reduce), (x, a, W, b), go)
            want = efp_ref.gradients(g.rowptr, g.col, x.detach(), a.detach(), W.detach(), b.detach(), go, op, reduce)
            for name, p, q in zip(("gx", "ga", "gW", "gb"), got, want):
                _close("%s %s %s" % (name, op, reduce), p, q, 1e-12)
    x, a, go, W, b = efp_ref.inputs(g, 8, 3, torch.float32, 0, True)
    assert all(bool((t * 8 == (t * 8).round()).all()) and t.abs().max() <= 2 for t in (x, a, go, W, b))      # dyadic: k / 8


# ---- the layers --------------------------------------------------------------------------------------------------------------------

def test_gineconv_without_edge_dim_is_unchanged():
    from dgll_amd.nn.Convolution import GINEConv

    fixed, learned = GINEConv(), GINEConv(torch.nn.Linear(4, 3), init_eps=0.25, learn_eps=True)
    assert list(fixed.state_dict()) == ["eps"] and not list(fixed.parameters())
    assert list(learned.state_dict()) == ["eps", "apply_func.weight", "apply_func.bias"]
    assert not hasattr(fixed, "lin") and GINEConv(None, 0, False).eps.item() == 0.0           # positional use as before
    with pytest.raises(ValueError, match="edge features must be"):
        fixed(_graph(_SQUARE, 6), torch.randn(6, 4), torch.randn(13, 3))                      # raw attributes need edge_dim


def test_gineconv_edge_dim_state_dict_and_refusals():
    from dgll_amd.nn.Convolution import GINEConv

    conv = GINEConv(None, 0.5, learn_eps=True, edge_dim=3, in_feats=6)
    assert list(conv.state_dict()) == ["eps", "lin.weight", "lin.bias"]                        # PyG's name for the projection
    assert conv.lin.weight.shape == (6, 3) and conv.lin.bias.shape == (6,)
    with pytest.raises(ValueError, match="in_feats"):
        GINEConv(edge_dim=3)
    with pytest.raises(ValueError, match=r"1\.\.16"):
        GINEConv(edge_dim=17, in_feats=8)
    g = _graph(_SQUARE, 6)
    with pytest.raises(ValueError, match="in_feats is 6"):
        conv(g, torch.randn(6, 4), torch.randn(g.nnz, 3))
    with pytest.raises(ValueError, match=r"\[nnz, edge_dim\]"):
        conv(g, torch.randn(6, 6), torch.randn(g.nnz, 6))
    with pytest.raises(TypeError, match="one dtype"):
        conv(g, torch.randn(6, 6), torch.randn(g.nnz, 3).bfloat16())


@pytest.mark.parametrize("pair", [False, True], ids=["square", "block"])
def test_gineconv_edge_dim_host_path_against_the_reference(pair):
    from dgll_amd.nn.Convolution import GINEConv

    torch.manual_seed(3)
    g = _block() if pair else _graph(_SQUARE, 6)
    conv = GINEConv(None, 0.2, learn_eps=True, edge_dim=3, in_feats=6)
    h_src = torch.randn(g.n_cols, 6, requires_grad=True)
    a = torch.randn(g.nnz, 3, requires_grad=True)
    go = torch.randn(g.n_rows, 6)
    out = conv(g, (h_src, h_src[:g.n_rows]) if pair else h_src, a)
    params = [conv.eps, conv.lin.weight, conv.lin.bias]
    got = torch.autograd.grad(out, [h_src, a] + params, go)
    sd = {k: v.detach().double().requires_grad_() for k, v in conv.state_dict().items()}
    h64, a64 = h_src.detach().double().requires_grad_(), a.detach().double().requires_grad_()
    ref = efp_ref.gineconv(sd, g.rowptr, g.col, h64, h64[:g.n_rows], a64)
    want = torch.autograd.grad(ref, [h64, a64, sd["eps"], sd["lin.weight"], sd["lin.bias"]], go.double())
    _close("out", out.detach(), ref.detach())
    for name, p, q in zip(("h", "a", "eps", "lin.weight", "lin.bias"), got, want):
        _close("grad " + name, p, q)


def test_gine_fused_and_unfused_share_one_state_dict():
    from dgll_amd.nn.Convolution import GINE

    torch.manual_seed(0)
    plain, fused = GINE(8, 4, 16, 5, n_layers=2), GINE(8, 4, 16, 5, n_layers=2, fused_edge=True)
    assert list(plain.state_dict()) == list(fused.state_dict())
    assert [tuple(v.shape) for v in plain.state_dict().values()] == [tuple(v.shape) for v in fused.state_dict().values()]
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in fused.named_parameters()]
    fused.load_state_dict(plain.state_dict())                                       # strict: one state dict loads into both
    plain.load_state_dict(fused.state_dict())
    with pytest.raises(ValueError, match=r"1\.\.16"):
        GINE(8, 17, 16, 5, fused_edge=True)
    g = _graph(_SQUARE, 6)                                                          # the host paths of the two agree
    x, attr = torch.randn(6, 8), torch.randn(g.nnz, 4)
    _close("fused host path", fused(g, x, attr).detach(), plain(g, x, attr).detach(), 1e-6)
