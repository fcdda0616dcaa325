"""segment_attention and GPSConv without a GPU: the C entry point's argument checks, the header against the ctypes binding, the
wrapper's argument errors, and GPSConv on host tensors against a float64 torch.nn.MultiheadAttention run per graph."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

FAKE = 1 << 20      # a non-NULL, 16-byte aligned address: every case below is refused (or empty) before anything is launched


def _desc(**kw):
    from dgll_amd import _lib

    d = _lib.SegAttnDesc()
    d.pass_, d.dtype, d.n_rows, d.n_segs, d.heads, d.D, d.scale = _lib.SEG_ATTN_FORWARD, _lib.F32, 64, 2, 2, 8, 1.0
    for name in ("seg_ptr", "tile_ptr", "q", "k", "v", "out", "lse"):
        setattr(d, name, FAKE)
    d.ld_q = d.ld_k = d.ld_v = d.ld_out = 16
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,text", [
    (dict(q=None), "NULL"), (dict(v=None), "NULL"), (dict(out=None), "NULL"), (dict(lse=None), "NULL"), (dict(seg_ptr=None), "NULL"),
    (dict(pass_=1, grad_out=None), "NULL"), (dict(pass_=2, grad_out=FAKE, ld_grad_out=16, delta=FAKE, out2=None), "NULL"),
    (dict(n_rows=1 << 31), "2^31"), (dict(n_segs=1 << 31), "2^31"),
    (dict(D=6, ld_q=12), "16-byte vectors"), (dict(dtype=1, D=12), "16-byte vectors"),
    (dict(D=132, ld_q=264, ld_k=264, ld_v=264, ld_out=264), "128"),
    (dict(ld_k=8), "pitch"), (dict(ld_v=18), "16-byte boundaries"),
])
def test_entry_point_refuses(kw, text):
    from dgll_amd import _lib

    assert _lib.lib.dgll_hip_segment_attn_pass(None, ctypes.byref(_desc(**kw))) == -1
    assert text in _lib.last_error()


def test_entry_point_takes_no_rows():
    from dgll_amd import _lib

    assert _lib.lib.dgll_hip_segment_attn_pass(None, ctypes.byref(_desc(n_rows=0, n_segs=0, q=None, seg_ptr=None))) == 0


def test_header_matches_binding():
    from dgll_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dgll_hip.h")).read(), flags=re.S)
    args = re.search(r"\bdgll_hip_segment_attn_pass\s*\(([^)]*)\)", text).group(1)
    assert len(args.split(",")) == len(_lib.SIGNATURES["dgll_hip_segment_attn_pass"][1])
    body = re.search(r"typedef struct dgll_seg_attn_desc \{(.*?)\}", text, flags=re.S).group(1)
    assert [f.split()[-1].lstrip("*") for f in body.split(";") if f.strip()] == \
        [("pass" if n == "pass_" else n) for n, _ in _lib.SegAttnDesc._fields_]
    assert (_lib.SEG_ATTN_TILE, _lib.SEG_ATTN_MAX_D) == tuple(int(re.search(r"#define DGLL_SEG_ATTN_%s (\d+)" % n, text).group(1))
                                                              for n in ("TILE", "MAX_D"))


def test_wrapper_argument_errors():
    from dgll_amd.ops_dense_attn import segment_attention

    x = torch.randn(10, 16)
    with pytest.raises(RuntimeError, match="GPU only"):
        segment_attention(x, x, x, 2, segs=[4, 6])
    with pytest.raises(ValueError, match="sum to the number of rows"):
        segment_attention(x, x, x, 2, segs=[4, 5])
    with pytest.raises(ValueError, match="non-decreasing"):
        segment_attention(x, x, x, 2, batch=torch.tensor([0, 0, 1, 1, 0, 2, 2, 2, 2, 2]))
    with pytest.raises(ValueError, match="16-byte vectors"):
        segment_attention(x[:, :12], x[:, :12], x[:, :12], 2)
    with pytest.raises(ValueError, match="at most 128"):
        segment_attention(*[torch.randn(4, 132)] * 3, 1)


def mha_composition(layer, x, sizes, h1=None):
    """(out, {parameter name: float64 leaf}): GPSConv.forward restated in float64 on torch.nn.MultiheadAttention, graph by graph;
    h1: the local branch conv(graph, x), taken as given."""
    mha = torch.nn.MultiheadAttention(layer.channels, layer.heads, batch_first=True).double()
    mha.load_state_dict({k: v.detach().double().cpu() for k, v in layer.attn.state_dict().items()})
    p = {k: v.detach().double().cpu().requires_grad_() for k, v in layer.named_parameters()}
    p.update({"attn." + k: v for k, v in mha.named_parameters()})
    norm = lambda i, t: t if getattr(layer, "norm%d" % i) is None else torch.nn.functional.batch_norm(  # noqa: E731
        t, None, None, p["norm%d.weight" % i], p["norm%d.bias" % i], training=True)
    x = x.double().cpu()
    att = torch.cat([mha(s[None], s[None], s[None], need_weights=False)[0][0] for s in x.split(sizes) if len(s)])
    out = norm(2, att + x) + (0 if h1 is None else norm(1, h1.double().cpu() + x))
    h = torch.relu(out @ p["mlp.0.weight"].t() + p["mlp.0.bias"]) @ p["mlp.3.weight"].t() + p["mlp.3.bias"]
    return norm(3, out + h), p


@pytest.mark.parametrize("heads,norm", [(1, "batch_norm"), (4, "batch_norm"), (3, None)])
def test_gpsconv_host(heads, norm):
    from dgll_amd.nn.Convolution import GPSConv

    torch.manual_seed(heads)
    layer = GPSConv(24, None, heads=heads, norm=norm)
    assert {"attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "mlp.0.weight", "mlp.0.bias",
            "mlp.3.weight", "mlp.3.bias"} <= set(layer.state_dict())
    assert layer.attn.in_proj_weight.shape == (72, 24)
    with torch.no_grad():
        layer.attn.in_proj_bias.normal_()
    x, sizes = torch.randn(19, 24), [7, 0, 1, 11]
    got = layer(None, x, segs=sizes)
    want = mha_composition(layer, x, sizes)[0]
    assert (got.double() - want).abs().max() <= 1e-5 * want.abs().max()
    assert torch.equal(got, layer(None, x, batch=torch.tensor([0] * 7 + [2] + [3] * 11)))


@pytest.mark.parametrize("kw", [dict(attn_type="performer"), dict(attn_kwargs={"dropout": 0.1})])
def test_gpsconv_refuses_what_is_not_built(kw):
    from dgll_amd.nn.Convolution import GPSConv

    with pytest.raises(ValueError, match="not built"):
        GPSConv(16, None, heads=2, **kw)
