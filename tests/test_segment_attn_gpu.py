"""Dense per-graph attention on the GPU: ops_dense_attn.segment_attention (forward and its three gradients) and nn.GPSConv against
float64 torch, segment by segment: softmax(scale q k^T) v and autograd of it, on the same inputs (the bf16-rounded ones for bf16).

Bars (test_sparse_attn_gpu.py): fp32 forward max |err| <= 1e-4 max|ref|, fp32 gradients <= 2e-3 max|ref|; bf16
forward <= 2e-2 max|ref|, bf16 gradients relative L2 <= 1.5e-2.  Every check prints its fraction of the bar."""
import pytest
import torch

from test_segment_attn_host import mha_composition

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [1, 31, 32, 33, 0, 65, 130]         # query and key tile edges, the empty segment, a segment of several key tiles
DTYPES = [torch.float32, torch.bfloat16]


def _inputs(n, width, dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, width, generator=gen).to(dtype) for _ in range(4)]         # q, k, v, grad_out (host)


def _reference(q, k, v, g, heads, sizes, scale=None):
    """(out, dq, dk, dv) in float64 on the host"""
    D = q.shape[1] // heads
    q64, k64, v64 = (t.detach().double().cpu().requires_grad_() for t in (q, k, v))
    outs = []
    for qs, ks, vs in zip(q64.split(sizes), k64.split(sizes), v64.split(sizes)):
        qs, ks, vs = (t.reshape(len(t), heads, D).transpose(0, 1) for t in (qs, ks, vs))
        s = qs @ ks.transpose(1, 2) * (D ** -0.5 if scale is None else scale)
        outs.append((torch.softmax(s, -1) @ vs).transpose(0, 1).reshape(-1, heads * D))
    out = torch.cat(outs)
    return (out.detach(),) + torch.autograd.grad(out, (q64, k64, v64), g.double().cpu())


def _device(q, k, v, g, heads, shared=False, **kw):
    from dgll_amd.ops_dense_attn import segment_attention

    q, k, v = (t.detach().requires_grad_() for t in (q, k, v))
    out = segment_attention(q, k, k if shared else v, heads, **kw)
    assert out.dtype == q.dtype and out.shape == q.shape
    grads = torch.autograd.grad(out, (q, k) if shared else (q, k, v), g.to(DEV))
    return (out.detach(),) + tuple(grads)


def _check(got, want, dtype, label, rows=slice(None), names=("out", "dq", "dk", "dv")):
    bad = []
    for name, a, b in zip(names, got, want):
        a, b = a.double().cpu()[rows], b[rows]
        assert bool(torch.isfinite(a).all()), "%s %s: not finite" % (label, name)
        err_max, err_l2 = ((a - b).abs().max() / b.abs().max()).item(), ((a - b).norm() / b.norm()).item()
        if dtype == torch.float32:
            bar, err = (1e-4 if name == "out" else 2e-3), err_max
        else:
            bar, err = (2e-2, err_max) if name == "out" else (1.5e-2, err_l2)
        print("%s %-3s max/max %.3e  rel-l2 %.3e  bar %.1e  fraction %.3f" % (label, name, err_max, err_l2, bar, err / bar))
        if not err <= bar:
            bad.append((name, err, bar))
    assert not bad, "%s: %s" % (label, bad)


@pytest.mark.parametrize("D", ["vec", 32, 40, 128])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_boundaries(dtype, heads, D):
    D = (4 if dtype == torch.float32 else 8) if D == "vec" else D
    q, k, v, g = _inputs(sum(SIZES), heads * D, dtype, seed=D + heads)
    _check(_device(q.to(DEV), k.to(DEV), v.to(DEV), g, heads, segs=SIZES), _reference(q, k, v, g, heads, SIZES), dtype,
           "boundaries %s h%d D%d" % (dtype, heads, D))


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_leak_across_segments(dtype):
    """every other segment multiplied by 1e4: the others, and the padded tail of their last tiles, must not notice"""
    heads, D = 2, 32
    q, k, v, g = _inputs(sum(SIZES), heads * D, dtype, seed=3)
    big = torch.cat([torch.full((n,), bool(i % 2)) for i, n in enumerate(SIZES)])
    want = _reference(q, k, v, g, heads, SIZES)
    for t in (q, k, v):
        t[big] *= 1e4
    got = _device(q.to(DEV), k.to(DEV), v.to(DEV), g, heads, segs=SIZES)
    _check(got, want, dtype, "leak %s" % dtype, rows=~big)
    if dtype == torch.float32:
        assert torch.equal(got[0][:1].cpu(), v[:1]), "a segment of one row returns v"


@pytest.mark.parametrize("dtype", DTYPES)
def test_large_scores(dtype):
    heads, D = 2, 32
    q, k, v, g = _inputs(sum(SIZES), heads * D, dtype, seed=4)
    q = (q * 50).to(dtype)          # scores of standard deviation 50: +-200 among the 130^2 pairs of the last segment
    want = _reference(q, k, v, g, heads, SIZES)
    _check(_device(q.to(DEV), k.to(DEV), v.to(DEV), g, heads, segs=SIZES)[:1], want[:1], dtype, "scores +-200 %s" % dtype)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_column_slices_and_shared_kv(dtype, shared):
    heads, D = 3, 40
    w = heads * D
    q, k, v, g = _inputs(sum(SIZES), w, dtype, seed=5)
    buf = torch.zeros(sum(SIZES), 3 * w + 16, dtype=dtype, device=DEV)        # one projection on a padded pitch
    buf[:, :3 * w] = torch.cat([q, k, v], 1).to(DEV)
    got = _device(buf[:, :w], buf[:, w:2 * w], buf[:, 2 * w:3 * w], g, heads, shared=shared, segs=SIZES)
    want = _reference(q, k, k if shared else v, g, heads, SIZES)
    if shared:
        want = (want[0], want[1], want[2] + want[3])
    _check(got, want, dtype, "slices %s shared=%s" % (dtype, shared), names=("out", "dq", "dkv") if shared else ("out", "dq", "dk", "dv"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_equals_segs_and_reruns(dtype):
    q, k, v, g = (t.to(DEV) for t in _inputs(sum(SIZES), 64, dtype, seed=6))
    batch = torch.cat([torch.full((n,), i) for i, n in enumerate(SIZES)]).to(DEV)
    first = _device(q, k, v, g, 2, segs=SIZES)
    for other in (_device(q, k, v, g, 2, segs=SIZES), _device(q, k, v, g, 2, batch=batch)):
        assert all(torch.equal(a, b) for a, b in zip(first, other))


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_segment_and_no_rows(dtype):
    from dgll_amd.ops_dense_attn import segment_attention

    q, k, v, g = _inputs(4100, 32, dtype, seed=7)
    out = segment_attention(q.to(DEV), k.to(DEV), v.to(DEV), 1)
    _check((out,), _reference(q, k, v, g, 1, [4100])[:1], dtype, "4100 rows %s" % dtype)
    empty = segment_attention(q[:0].to(DEV), k[:0].to(DEV), v[:0].to(DEV), 1, segs=[])
    assert empty.shape == (0, 32) and empty.dtype == dtype


def _batch_graph(sizes, seed):
    from dgll_amd import CSRGraph

    gen = torch.Generator().manual_seed(seed)
    row = torch.cat([torch.randint(0, n, (4 * n,), generator=gen) + at for n, at in zip(sizes, [0, sizes[0], sizes[0] + sizes[1]])])
    col = torch.cat([torch.randint(0, n, (4 * n,), generator=gen) + at for n, at in zip(sizes, [0, sizes[0], sizes[0] + sizes[1]])])
    return CSRGraph.from_coo(row, col, None, (sum(sizes), sum(sizes))).to(DEV)


@pytest.mark.parametrize("local", [False, True])
def test_gpsconv(local):
    from dgll_amd.nn.Convolution import GatedGCNConv, GPSConv

    torch.manual_seed(8)
    sizes, C = [40, 7, 33], 32
    graph = _batch_graph(sizes, 8)
    x, e = torch.randn(sum(sizes), C, device=DEV), torch.randn(graph.nnz, C, device=DEV)
    kw = dict(edge_feat=e) if local else {}
    make = lambda: GPSConv(C, GatedGCNConv(C, C, C) if local else None, heads=4).to(DEV)       # noqa: E731
    layer = make()
    got = layer(graph, x, segs=sizes, **kw)
    want, p64 = mha_composition(layer, x, sizes, h1=layer.conv(graph, x, **kw)[0].detach() if local else None)
    # (the gradient of a bias that a batch norm follows is exactly 0, the norm removes the mean: no relative bar applies to those two)
    names = [n for n, _ in layer.named_parameters() if n.startswith(("attn", "mlp")) and n not in ("attn.out_proj.bias", "mlp.3.bias")]
    params = dict(layer.named_parameters())
    g = torch.randn(got.shape, generator=torch.Generator().manual_seed(9))
    grads = torch.autograd.grad(got, [params[n] for n in names], g.to(DEV), retain_graph=True)
    want_grads = torch.autograd.grad(want, [p64[n] for n in names], g.double())
    _check((got.detach(),) + grads, (want.detach(),) + want_grads, torch.float32, "GPSConv local=%s" % local, names=["out"] + names)
    model = torch.nn.ModuleList([layer, make()])
    opt, target, losses = torch.optim.Adam(model.parameters(), lr=1e-2), torch.randn(sum(sizes), C, device=DEV), []
    for _ in range(10):
        h = x
        for m in model:
            h = m(graph, h, segs=sizes, **kw)
        loss = (h - target).square().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses
