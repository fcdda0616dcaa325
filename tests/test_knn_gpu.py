"""kNN graphs and EdgeConv on the GPU.

The search (dgll_amd.knn.knn_graph over csrc/knn.hip) against the float64 brute force of knn_ref.py:
  * the lattice cases of test_knn_emulated.py (integer coordinates: `col` and `dist` must equal the reference EXACTLY, every row), and
    8 clouds of 1024 points at D = 3, k = 20; the [B, N, D] form equal to the segs form; two runs bit-identical; dist="cosine";
  * Gaussian fp32 inputs at D = 3 and D = 64, every row, with eps = (D + 3) 2^-23: the fp32 rounding bound of a sum of D non-negative
    squared differences ((D + 2) 2^-24: one rounding of each difference, counted twice in its square, one of the square, D - 1 of the
    sum), doubled -- derived, not measured.  dist[m] ascends; dist[m] is within eps relative of the reference's m-th smallest float64
    distance of that row (a multiplicative perturbation of all distances moves each order statistic by at most that factor); the
    float64 distance of the returned col[m] is within eps relative of dist[m]; the ids are distinct, inside the segment and not self
    when excluded; no row is left out;
  * a captured knn_graph + EdgeConv forward, replayed on new points, equal to the eager result.

nn.EdgeConv, forward and all gradients (h, both weights, both biases), against the float64 per-edge composition of knn_ref.edgeconv
(the messages materialised, a scatter max; for bf16 rounded where the layer stores) at the bars of DESIGN section 8: fp32 forward
max |err| <= 1e-4 max |ref|, gradients <= 2e-3 max |ref|; bf16 forward <= 2e-2 max |ref|, gradients relative L2 <= 1.5e-2."""
import functools

import numpy as np
import pytest
import torch

import knn_ref
from test_edge_feat_gpu import _sampler_block
from test_knn_emulated import CASES

pytestmark = pytest.mark.gpu

DEV = "cuda"
_ids = lambda v: str(v).replace("torch.", "")       # noqa: E731


def _host(graph, dist=None):
    out = [graph.rowptr.cpu().numpy(), graph.col.cpu().numpy()]
    return out + [dist.cpu().numpy()] if dist is not None else out


def _assert_graph_fields(g, n, k):
    assert (g.n_rows, g.n_cols) == (n, n) and g.val is None and g.max_degree == k
    assert g.rowptr.dtype == torch.int64 and g.col.dtype == torch.int32 and g.rowptr.is_cuda


# ---------------------------------------------------------------------------------------------------- exact, on the lattice
@pytest.mark.parametrize("k,D,dtype,excl,pad", CASES, ids=_ids)
def test_lattice_cases_are_exact(cuda_device, k, D, dtype, excl, pad):
    from dgll_amd import knn as K

    sizes, x64, (ib, ie) = knn_ref.lattice_case(k, D, K.CAND_TILE, K.QUERY_TILE)
    n = x64.shape[0]
    xp = torch.full((n, D + pad), float("nan"), dtype=dtype)
    xp[:, :D] = torch.from_numpy(x64).to(dtype)
    x = xp.to(DEV)[:, :D]                                               # a view on the wider pitch, NaN behind every row
    g, dist = K.knn_graph(x, k, sizes, exclude_self=excl, return_dist=True)
    _assert_graph_fields(g, n, k)
    rowptr, col, dist = _host(g, dist)
    want_ptr, want_col, want_dist = knn_ref.knn(x64, sizes, k, excl)
    assert np.array_equal(rowptr, want_ptr)
    bad = np.nonzero(col.astype(np.int64) != want_col)[0]
    assert bad.size == 0, (bad[:5], col[bad[:5]], want_col[bad[:5]])
    assert np.array_equal(dist.astype(np.float64), want_dist)
    for i in range(ib, ie):                                             # identical points: the first indices, self skipped by index
        assert list(col[rowptr[i]:rowptr[i + 1]]) == [j for j in range(ib, ie) if not (excl and j == i)][:k]
    g2 = K.segmented_knn_graph(x, k, torch.tensor(sizes), exclude_self=excl)      # DGL's name, sizes as a tensor, no distances
    assert torch.equal(g2.col, g.col) and torch.equal(g2.rowptr, g.rowptr)


@functools.lru_cache(maxsize=None)
def _clouds():
    """8 clouds of 1024 lattice points in 3-D and the reference at k = 20 without self"""
    rng = np.random.RandomState(3)
    x = rng.randint(-16, 17, size=(8, 1024, 3)).astype(np.float64)
    return x, knn_ref.knn(x.reshape(-1, 3), [1024] * 8, 20, True)


def test_eight_clouds_of_1024_points_are_exact(cuda_device):
    from dgll_amd import knn as K

    x64, (want_ptr, want_col, want_dist) = _clouds()
    x = torch.from_numpy(x64).float().to(DEV)
    g, dist = K.knn_graph(x, 20, exclude_self=True, return_dist=True)
    _assert_graph_fields(g, 8192, 20)
    rowptr, col, dist = _host(g, dist)
    assert np.array_equal(rowptr, want_ptr) and np.array_equal(col.astype(np.int64), want_col)
    assert np.array_equal(dist.astype(np.float64), want_dist)
    assert g.plan() is not None                                         # max_degree = k: the host-only plan


def test_batched_form_equals_the_segs_form_and_reruns_give_the_same_bits(cuda_device):
    from dgll_amd import knn as K

    x = torch.from_numpy(_clouds()[0]).float().to(DEV)
    g, dist = K.knn_graph(x, 20, exclude_self=True, return_dist=True)
    for segs in ([1024] * 8, torch.full((8,), 1024, dtype=torch.int64), [1024] * 7 + [1000, 24]):
        g2, dist2 = K.knn_graph(x.reshape(-1, 3), 20, segs, exclude_self=True, return_dist=True)
        if len(segs) == 8:
            assert torch.equal(g2.rowptr, g.rowptr) and torch.equal(g2.col, g.col) and torch.equal(dist2, dist)
        else:                                                           # unequal sizes take the other table path: the first 7 clouds agree
            cut = int(g.rowptr[7 * 1024])
            assert torch.equal(g2.col[:cut], g.col[:cut]) and torch.equal(dist2[:cut], dist[:cut])
    gauss = torch.randn(8, 1024, 64, device=DEV)
    a, da = K.knn_graph(gauss, 20, return_dist=True)
    b, db = K.knn_graph(gauss, 20, return_dist=True)
    assert torch.equal(a.col, b.col) and torch.equal(da, db)
    mod = K.KNNGraph(20)(gauss)
    assert torch.equal(mod.col, a.col)
    seg = K.SegmentedKNNGraph(20)(gauss.reshape(-1, 64), [1024] * 8)
    assert torch.equal(seg.col, a.col)


# ---------------------------------------------------------------------------------------------------- Gaussian inputs, every row
def _check_float_rows(x, sizes, k, excl, g, dist):
    """x fp32 on the host [n, D]; the properties of the module docstring, every row"""
    D = x.shape[1]
    eps = (D + 3) * 2.0 ** -23
    rowptr, col, dist = _host(g, dist)
    assert np.array_equal(rowptr, knn_ref.out_rowptr(sizes, k, excl))
    x64 = x.double().numpy()
    rows = knn_ref.all_distances(x64, sizes)
    assert len(rows) == x.shape[0] == rowptr.size - 1
    worst = 0.0
    for i, (b, d_all) in enumerate(rows):
        got_j, got_d = col[rowptr[i]:rowptr[i + 1]].astype(np.int64), dist[rowptr[i]:rowptr[i + 1]].astype(np.float64)
        keep = np.ones(d_all.size, dtype=bool)
        if excl:
            keep[i - b] = False
        want = np.sort(d_all[keep])[:k]
        assert got_j.size == want.size, i                                # no row left out, no entry missing
        assert (np.diff(got_d) >= 0).all(), i
        assert (np.abs(got_d - want) <= eps * want).all(), (i, got_d, want)
        assert ((got_j >= b) & (got_j < b + d_all.size)).all() and np.unique(got_j).size == got_j.size, i
        assert not (excl and (got_j == i).any()), i
        own = d_all[got_j - b]
        assert (np.abs(own - got_d) <= eps * got_d).all(), (i, own, got_d)
        if want.size:
            worst = max(worst, float((np.abs(got_d - want) / np.maximum(want, 1e-300)).max()))
    print("D %d  k %d  worst relative distance error %.3e  eps %.3e" % (D, k, worst, eps))


@pytest.mark.parametrize("excl", [False, True], ids=["self", "noself"])
@pytest.mark.parametrize("D", [3, 64])
def test_gaussian_inputs_every_row(cuda_device, D, excl):
    from dgll_amd import knn as K

    sizes = [300, 0, 257, 40, 7]
    x = torch.randn(sum(sizes), D, generator=torch.Generator().manual_seed(D))
    g, dist = K.knn_graph(x.to(DEV), 20, sizes, exclude_self=excl, return_dist=True)
    _check_float_rows(x, sizes, 20, excl, g, dist)


def test_cosine_normalises_and_then_searches(cuda_device):
    from dgll_amd import knn as K

    sizes = [150, 90]
    x = (torch.randn(240, 8, generator=torch.Generator().manual_seed(8)) * torch.linspace(0.1, 30.0, 240)[:, None]).to(DEV)
    g, dist = K.knn_graph(x, 5, sizes, dist="cosine", return_dist=True, exclude_self=True)
    unit = torch.nn.functional.normalize(x, dim=1)
    g2, dist2 = K.knn_graph(unit, 5, sizes, return_dist=True, exclude_self=True)
    assert torch.equal(g.col, g2.col) and torch.equal(dist, dist2)
    _check_float_rows(unit.cpu(), sizes, 5, True, g, dist)
    plain = K.knn_graph(x, 5, sizes, exclude_self=True)
    assert not torch.equal(plain.col, g.col)                            # the row scales matter to the Euclidean search


# ---------------------------------------------------------------------------------------------------- capture
def test_captured_search_and_layer_follow_new_points(cuda_device):
    from dgll_amd import knn as K
    from dgll_amd.nn.Convolution import EdgeConv

    torch.manual_seed(0)
    conv = EdgeConv(3, 16).to(DEV)
    gen = torch.Generator().manual_seed(1)
    points = [torch.randn(4, 128, 3, generator=gen).to(DEV) for _ in range(3)]
    xs = points[0].clone()

    def step():
        with torch.no_grad():
            g = K.knn_graph(xs, 8)
            return conv(g, xs.reshape(-1, 3)), g.col

    eager = []
    for p in points:
        xs.copy_(p)
        eager.append([v.clone() for v in step()])
    assert not torch.equal(eager[0][1], eager[1][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured, stream=side):
        static = step()
    for p, want in reversed(list(zip(points, eager))):
        xs.copy_(p)
        for v in static:
            v.zero_()
        captured.replay()
        torch.cuda.synchronize()
        assert torch.equal(static[1], want[1]) and torch.equal(static[0], want[0])


# ---------------------------------------------------------------------------------------------------- EdgeConv
def _check(name, got, want, kind):
    a, b = got.detach().double().cpu(), want.detach().double().cpu()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert bool(torch.isfinite(a).all()), "%s: not finite" % name
    err_max = ((a - b).abs().max() / b.abs().max()).item()
    err_l2 = ((a - b).norm() / b.norm()).item()
    bar, err = {"fwd32": (1e-4, err_max), "grad32": (2e-3, err_max), "fwd16": (2e-2, err_max), "grad16": (1.5e-2, err_l2)}[kind]
    print("%-24s max/max %.3e  rel-l2 %.3e  bar %.1e" % (name, err_max, err_l2, bar))
    assert err <= bar, (name, err, bar)


def _edgeconv_against_reference(graph, fin, fo, dtype, pair, allow_zero):
    from dgll_amd.nn.Convolution import EdgeConv

    half = dtype == torch.bfloat16
    fwd, grad = ("fwd16", "grad16") if half else ("fwd32", "grad32")
    gen = torch.Generator().manual_seed(fin + 3)
    conv = EdgeConv(fin, fo, allow_zero_in_degree=allow_zero).to(DEV)
    with torch.no_grad():
        for p in (conv.theta.bias, conv.phi.bias):
            p.copy_(torch.randn(fo, generator=gen))
    h_src = torch.randn(graph.n_cols, fin, generator=gen).to(dtype).to(DEV).requires_grad_(True)
    h_dst = torch.randn(graph.n_rows, fin, generator=gen).to(dtype).to(DEV).requires_grad_(True) if pair else h_src
    go = torch.randn(graph.n_rows, fo, generator=gen).to(dtype)
    out = conv(graph, (h_src, h_dst) if pair else h_src)
    assert out.dtype == dtype and tuple(out.shape) == (graph.n_rows, fo)
    out.backward(go.to(DEV))

    params = [conv.theta.weight, conv.theta.bias, conv.phi.weight, conv.phi.bias]
    r_src = h_src.detach().double().cpu().requires_grad_(True)
    r_dst = h_dst.detach().double().cpu().requires_grad_(True) if pair else r_src
    r_par = [p.detach().double().cpu().requires_grad_(True) for p in params]
    want = knn_ref.edgeconv(graph.rowptr.cpu(), graph.col.cpu(), r_src, r_dst, *r_par, store_dtype=dtype if half else None)
    want.backward(go.double())
    _check("out", out, want, fwd)
    _check("grad h_src", h_src.grad, r_src.grad, grad)
    if pair:
        _check("grad h_dst", h_dst.grad, r_dst.grad, grad)
    for name, p, r in zip(("theta.weight", "theta.bias", "phi.weight", "phi.bias"), params, r_par):
        _check("grad " + name, p.grad, r.grad, grad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
@pytest.mark.parametrize("fin,fo", [(5, 7), (64, 64), (65, 33)])
def test_edgeconv_on_a_knn_graph_of_unequal_clouds(cuda_device, fin, fo, dtype):
    from dgll_amd import knn as K

    sizes = [70, 33, 50]
    pts = torch.randn(sum(sizes), 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    graph = K.knn_graph(pts, 6, sizes, exclude_self=True)
    assert graph.min_degree == 6
    _edgeconv_against_reference(graph, fin, fo, dtype, pair=False, allow_zero=False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
@pytest.mark.parametrize("fin,fo", [(5, 7), (64, 64)])
def test_edgeconv_on_a_sampler_block_with_a_pair_of_features(cuda_device, fin, fo, dtype):
    from dgll_amd.nn.Convolution import EdgeConv

    block = _sampler_block().to(DEV)                                    # 40 destinations over 150 sources, row 7 without entries
    with pytest.raises(ValueError, match="rows without entries"):
        EdgeConv(fin, fo).to(DEV)(block, (torch.zeros(150, fin, device=DEV), torch.zeros(40, fin, device=DEV)))
    _edgeconv_against_reference(block, fin, fo, dtype, pair=True, allow_zero=True)


def test_edgeconv_row_without_entries_on_a_square_graph(cuda_device):
    """one tensor for sources and destinations (one dense product), a row without entries: phi(h_i) plus the biases"""
    from dgll_amd import CSRGraph

    rng = np.random.RandomState(6)
    rows = [list(rng.choice(30, 4, replace=False)) for _ in range(30)]
    rows[11] = []
    rowptr = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
    graph = CSRGraph(rowptr, torch.tensor([int(c) for r in rows for c in r], dtype=torch.int32), None, 30, 30).to(DEV)
    _edgeconv_against_reference(graph, 12, 9, torch.float32, pair=False, allow_zero=True)


def test_dgcnn_forward_and_backward(cuda_device):
    """the model on equal and on unequal clouds: logits per cloud, a gradient in every parameter"""
    from dgll_amd.nn.Convolution import DGCNN

    torch.manual_seed(0)
    model = DGCNN(3, hidden=(16, 16, 32), k=8, emb=64, n_classes=5).to(DEV)
    x = torch.randn(4, 96, 3, device=DEV)
    a = model(x)
    assert tuple(a.shape) == (4, 5) and bool(torch.isfinite(a).all())
    model.eval()
    with torch.no_grad():
        whole = model(x)
        parts = model(x.reshape(-1, 3)[:96 * 3 - 10], [96, 96, 86])    # other clouds do not matter to a cloud
    assert torch.allclose(whole[:2], parts[:2], rtol=1e-4, atol=1e-5)
    model.train()
    model(x.reshape(-1, 3), [96, 100, 92, 96]).sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
