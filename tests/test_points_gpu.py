"""points.fps / radius / radius_graph and nn.PointNetConv on the GPU against the float64 references of points_ref.py: EXACT on the
integer lattice of test_points_emulated.py; reported distances of Gaussian fp32 points within (D + 3) 2^-23 relative (the bound
test_knn_gpu.py derives; membership is checked on the lattice only); PointNetConv at DESIGN section 8's bars, as EdgeConv there."""
import numpy as np
import pytest
import torch

import points_ref
from dgll_amd import points as P
from dgll_amd.nn.Convolution import PointNet2, PointNetConv
from test_knn_gpu import _check
from test_points_emulated import FPS_CASES, RADIUS_CASES, padded

pytestmark = pytest.mark.gpu

DEV = "cuda"
_ids = lambda v: str(v).replace("torch.", "")       # noqa: E731


_padded = lambda x64, D, pad, dtype: padded(x64, D, pad, dtype).to(DEV)[:, :D]     # noqa: E731  a view on the wider pitch


@pytest.mark.parametrize("D,dtype,pad,pts", FPS_CASES, ids=_ids)
def test_fps_lattice_cases_are_exact(cuda_device, D, dtype, pad, pts):
    sizes, _, starts, x64 = points_ref.fps_case(D, pts)
    counts = P.sample_counts(sizes, ratio=0.02)                                 # 1 .. 164 samples a segment; m == size: the emulated cases
    idx, dmin = P.fps(_padded(x64, D, pad, dtype), sizes, ratio=0.02, start=torch.tensor(starts).to(DEV), return_dmin=True)
    want_idx, want_dmin = points_ref.fps(x64, sizes, counts, starts)
    assert idx.dtype == torch.int64 and idx.seg_sizes == counts and np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(dmin.cpu().numpy().astype(np.float64), want_dmin)


@pytest.mark.parametrize("K,D,dtype,pad,r2,mode", RADIUS_CASES, ids=_ids)
def test_radius_lattice_cases_are_exact(cuda_device, K, D, dtype, pad, r2, mode):
    x_sizes, x64, y_sizes, y64, _ = points_ref.radius_case(K, D, mode == "bipartite")
    x, r = _padded(x64, D, pad, dtype), float(np.sqrt(r2))
    if mode == "bipartite":
        g, dist = P.radius(x, _padded(y64, D, 0, dtype), r, x_sizes, y_sizes, max_num_neighbors=K, return_dist=True)
    else:
        g, dist = P.radius_graph(x, r, x_sizes, loop=mode == "square", max_num_neighbors=K, return_dist=True)
    want_ptr, want_col, want_dist = points_ref.radius(y64, y_sizes, x64, x_sizes, r2, K, mode == "square-noself")
    assert (g.n_rows, g.n_cols, g.max_degree) == (y64.shape[0], x64.shape[0], K) and g.col.dtype == torch.int32
    assert np.array_equal(g.rowptr.cpu().numpy(), want_ptr) and np.array_equal(g.col.cpu().numpy().astype(np.int64), want_col)
    assert np.array_equal(dist.cpu().numpy().astype(np.float64), want_dist)


def test_sampler_shapes_ratio_against_npoints_and_reruns(cuda_device):
    pos = torch.randn(5, 300, 3, generator=torch.Generator().manual_seed(0)).to(DEV)
    by_count, dmin = P.fps(pos, npoints=75, return_dmin=True)
    by_ratio = P.fps(pos.reshape(-1, 3), [300] * 5, ratio=0.25)
    assert torch.equal(by_count, by_ratio) and by_count.seg_sizes == [75] * 5 == by_ratio.seg_sizes
    again, dmin2 = P.fps(pos, npoints=75, return_dmin=True)
    assert torch.equal(again, by_count) and torch.equal(dmin2, dmin)            # two runs, the same bits
    assert bool((dmin[1:74] >= dmin[2:75]).all())                               # the coverage radius never grows inside a cloud
    off = P.farthest_point_sampler(pos, 75, start_idx=0)
    assert type(off) is torch.Tensor and torch.equal(off + torch.arange(5, device=DEV)[:, None] * 300, by_count.view(5, 75))
    rnd = P.farthest_point_sampler(pos, 75)                                     # random starts: offsets inside the cloud, no repeats
    assert bool(((rnd >= 0) & (rnd < 300)).all()) and all(len(set(r.tolist())) == 75 for r in rnd)
    g, g2 = P.radius_graph(pos, 0.5, max_num_neighbors=16), P.radius_graph(pos, 0.5, max_num_neighbors=16)
    assert torch.equal(g.col, g2.col) and torch.equal(g.rowptr, g2.rowptr)


@pytest.mark.parametrize("D", [3, 32])
def test_reported_distances_on_gaussian_points(cuda_device, D):
    sizes, x = [200, 333], torch.randn(533, D, generator=torch.Generator().manual_seed(D))
    y = x[torch.arange(0, 533, 3)]
    r = float(np.sqrt(2 * D))                                                   # about half of a cloud lies within it
    g, dist = P.radius(x.to(DEV), y.to(DEV), r, sizes, [67, 111], max_num_neighbors=32, return_dist=True)
    row = torch.repeat_interleave(torch.arange(g.n_rows), (g.rowptr[1:] - g.rowptr[:-1]).cpu())
    want = ((x.double()[g.col.cpu().long()] - y.double()[row]) ** 2).sum(1)
    rel = ((dist.cpu().double() - want).abs() / want.clamp(min=1e-300)).max().item()
    print("D %d  nnz %d  worst relative error %.3e  bound %.3e" % (D, dist.numel(), rel, (D + 3) * 2.0 ** -23))
    assert dist.numel() > 1000 and rel <= (D + 3) * 2.0 ** -23
    r32 = torch.tensor(r, dtype=torch.float32)
    assert bool((dist.cpu() <= r32 * r32).all())                                # what is reported is what was compared with r2


def test_captured_sampling_follows_new_points(cuda_device):
    gen = torch.Generator().manual_seed(1)
    clouds = [torch.randn(4, 500, 3, generator=gen).to(DEV) for _ in range(3)]
    xs = clouds[0].clone()

    def step():
        idx = P.fps(xs, ratio=0.1)
        return idx, xs.reshape(-1, 3)[idx]

    eager = [[v.clone() for v in (xs.copy_(c), step())[1]] for c in clouds]      # also the warm-up
    assert not torch.equal(eager[0][0], eager[1][0])
    torch.cuda.synchronize()
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured):
        static = step()
    for c, want in reversed(list(zip(clouds, eager))):                          # several replays, each against the eager result
        xs.copy_(c)
        captured.replay()
        torch.cuda.synchronize()
        assert torch.equal(static[0], want[0]) and torch.equal(static[1], want[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_ids)
@pytest.mark.parametrize("C,fo,relu", [(5, 7, True), (5, 7, False), (0, 16, True), (64, 33, True)])
def test_pointnetconv_on_a_radius_graph_of_unequal_clouds(cuda_device, C, fo, relu, dtype, seed=0):
    half, bits = dtype == torch.bfloat16, "16" if dtype == torch.bfloat16 else "32"
    sizes, gen = [70, 33, 50], torch.Generator().manual_seed(C + fo)
    pos = torch.randn(sum(sizes), 3, generator=gen).to(dtype).to(DEV).requires_grad_(True)
    idx = P.fps(pos, sizes, ratio=0.5)
    centres = pos.detach()[idx].requires_grad_(True)
    graph = P.radius(pos, centres, 1.0, sizes, idx.seg_sizes, max_num_neighbors=16)
    torch.manual_seed(seed)
    lin = torch.nn.Linear(C + 3, fo)
    conv = PointNetConv(torch.nn.Sequential(lin, torch.nn.ReLU()) if relu else lin).to(DEV)
    x = torch.randn(sum(sizes), C, generator=gen).to(dtype).to(DEV).requires_grad_(True) if C else None
    go = torch.randn(graph.n_rows, fo, generator=gen).to(dtype)
    out = conv(graph, x, (pos, centres))
    assert out.dtype == dtype and tuple(out.shape) == (graph.n_rows, fo) and graph.min_degree >= 1
    out.backward(go.to(DEV))

    leaves = [t for t in (x, pos, centres, lin.weight, lin.bias) if t is not None]
    refs = [t.detach().double().cpu().requires_grad_(True) for t in leaves]
    rx, (rp, rc, rw, rb) = (refs[0] if C else None), refs[-4:]
    want = points_ref.pointnetconv(graph.rowptr.cpu(), graph.col.cpu(), rx, rp, rc, rw, rb, relu, store_dtype=dtype if half else None)
    want.backward(go.double())
    _check("out", out, want, "fwd" + bits)
    for name, t, r in zip((["x"] if C else []) + ["pos", "centres", "weight", "bias"], leaves, refs):
        _check("grad " + name, t.grad, r.grad, "grad" + bits)


def test_pointnetconv_refuses_a_deeper_local_nn_and_pointnet2_trains(cuda_device):
    with pytest.raises(NotImplementedError, match=r"\[nnz, F\]"):
        PointNetConv(torch.nn.Sequential(torch.nn.Linear(6, 8), torch.nn.ReLU(), torch.nn.Linear(8, 8)))
    torch.manual_seed(0)
    model = PointNet2(2, 4, hidden=(16, 32, 64), radii=(0.8, 1.6), max_num_neighbors=16).to(DEV)
    out = model(torch.randn(3, 64, 5, device=DEV))
    out.sum().backward()
    assert tuple(out.shape) == (3, 4) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
