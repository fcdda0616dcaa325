"""ops_typed.typed_spmm (csrc/typed_spmm.hip) and RelGraphConv on the GPU against the float64 restatements of typed_ref.py (per-edge
tensors, autograd).  For bf16 the reference runs on the bf16-rounded inputs.

Bars (test_sparse_attn_gpu.py): fp32 forward max |err| <= 1e-4 max|ref|, fp32 gradients <= 2e-3 max|ref|; bf16
forward <= 2e-2 max|ref|, bf16 gradients relative L2 <= 1.5e-2.  The bf16 LAYER bar is not one of those (test_gatv2_gpu.py checks its
layer in fp32 only): it is twice the error of the same layer computed in float64 torch with the operands rounded to bf16 at the places
the device path rounds them (`_emulated_layer`), measured against the same float64 reference, per quantity -- plus 1e-4, the project's
fp32 forward bar, for the fp32 accumulation of the device's sums (up to ~10^6 terms in a weight gradient: sqrt(n) 2^-24 ~ 6e-5), which
a float64 emulation does not have."""
import copy

import numpy as np
import pytest
import torch

from typed_ref import relgraphconv_reference, typed_spmm_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("z", "dx", "dc")


def _hash_types(graph, R):
    k = torch.arange(graph.nnz, dtype=torch.int64)
    return ((k * 7919 + graph.col.cpu().long() * 31 + 5) % R).to(torch.int32)


@pytest.fixture(scope="module")
def rmat():
    from dgll_amd import synth

    g = synth.rmat_graph(10, 10, symmetric=True, self_loops=True).to(DEV)
    assert g.n_rows == 1024 and int(g.degrees().max()) > 300
    return g


@pytest.fixture(scope="module")
def edge_graph():
    """70 x 90: rows 0 empty, 1 one entry, 2 exactly 64, 3 65, 4 one column five times, 5 LONG_ROW, 6 LONG_ROW + 1, 7 3000 entries
    (columns drawn with repetition), then short rows; the last row is empty and source 89 is never referenced."""
    from dgll_amd import CSRGraph, ops_typed

    rng = np.random.RandomState(5)
    rows = [[], [17], list(rng.permutation(89)[:64]), list(rng.permutation(89)[:65]), [33] * 5,
            list(rng.randint(0, 89, ops_typed.LONG_ROW)), list(rng.randint(0, 89, ops_typed.LONG_ROW + 1)), list(rng.randint(0, 89, 3000))]
    rows += [list(rng.randint(0, 89, rng.randint(1, 12))) for _ in range(61)] + [[]]
    assert len(rows) == 70 and all(c < 89 for r in rows for c in r)
    rowptr = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
    col = torch.tensor([int(c) for r in rows for c in r], dtype=torch.int32)
    return CSRGraph(rowptr, col, None, 70, 90).to(DEV)


def _edges(graph, R, with_norm=True, seed=0):
    from dgll_amd.ops_typed import TypedEdges

    gen = torch.Generator().manual_seed(seed + 17)
    norm = (torch.rand(graph.nnz, generator=gen) + 0.25).to(DEV) if with_norm else None
    return TypedEdges(graph, _hash_types(graph, R).to(DEV), R, norm)


def _inputs(graph, F, B, R, dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(graph.n_cols, F, generator=gen).to(dtype).to(DEV)
    coeff = torch.randn(R, B, generator=gen).to(DEV)
    g = torch.randn(graph.n_rows, B * F, generator=gen).to(dtype).to(DEV)
    return x, coeff, g


def _reference(graph, edges, x, coeff, g):
    """(Z, dX, dC) in float64 on the host."""
    x64, c64 = x.detach().double().cpu().requires_grad_(), coeff.detach().double().cpu().requires_grad_()
    z = typed_spmm_reference(graph.rowptr, graph.col, edges.etypes, None if edges.norm is None else edges.norm.cpu(), x64, c64)
    return (z.detach(),) + tuple(torch.autograd.grad(z, (x64, c64), g.double().cpu()))


def _device(graph, edges, x, coeff, g):
    from dgll_amd import ops_typed

    x, coeff = x.detach().clone().requires_grad_(), coeff.detach().clone().requires_grad_()
    z = ops_typed.typed_spmm(graph, edges, x, coeff)
    assert z.dtype == x.dtype and z.shape == (graph.n_rows, coeff.shape[1] * x.shape[1])
    dx, dc = torch.autograd.grad(z, (x, coeff), g)
    assert dx.shape == x.shape and dc.shape == coeff.shape and dc.dtype == torch.float32
    return z.detach(), dx, dc


def _check(got, want, dtype, label="", names=NAMES, bf16_bars=None):
    bad = []
    for name, a, b in zip(names, got, want):
        a, b = a.double().cpu(), b.double().cpu()
        assert bool(torch.isfinite(a).all()), "%s %s: not finite" % (label, name)
        err_max = ((a - b).abs().max() / b.abs().max()).item()
        err_l2 = ((a - b).norm() / b.norm()).item()
        forward = name in ("z", "out")
        if dtype == torch.float32:
            bar, err = (1e-4 if forward else 2e-3), err_max
        elif bf16_bars is not None:
            bar, err = bf16_bars[name], (err_max if forward else err_l2)
        else:
            bar, err = (2e-2, err_max) if forward else (1.5e-2, err_l2)
        print("%s %-22s max/max %.3e  rel-l2 %.3e  bar %.2e" % (label, name, err_max, err_l2, bar))
        if not err <= bar:
            bad.append((name, err, bar))
    assert not bad, "%s: %s" % (label, bad)


CASES = [(8, 1, 1, torch.float32), (40, 2, 3, torch.float32), (64, 4, 16, torch.float32), (256, 8, 16, torch.float32), (512, 2, 4, torch.float32),
         (48, 3, 5, torch.bfloat16), (64, 5, 50, torch.bfloat16), (256, 4, 16, torch.bfloat16), (64, 32, 40, torch.bfloat16),
         (72, 2, 3, torch.float32), (128, 4, 16, torch.float32),        # 32 lanes a row in fp32: with idle lanes, full
         (72, 3, 5, torch.bfloat16)]                                    # 16 lanes a row with idle lanes


@pytest.mark.parametrize("with_norm", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("F,B,R,dtype", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_forward_and_gradients_on_rmat(rmat, F, B, R, dtype, with_norm):
    edges = _edges(rmat, R, with_norm)
    x, coeff, g = _inputs(rmat, F, B, R, dtype, seed=F * 100 + B)
    _check(_device(rmat, edges, x, coeff, g), _reference(rmat, edges, x, coeff, g), dtype, "rmat F%d B%d R%d" % (F, B, R))


@pytest.mark.parametrize("with_norm", [True, False], ids=["norm", "nonorm"])
def test_coefficient_table_above_the_lds_cap(rmat, with_norm):
    from dgll_amd import ops_typed

    cap = getattr(ops_typed, "COEFF_LDS", None)
    if cap is None:
        pytest.skip("the kernels have no cap on the LDS-staged coefficient table")
    B = 8
    R = cap // B + 8
    assert R * B > cap
    edges = _edges(rmat, R, with_norm)
    x, coeff, g = _inputs(rmat, 16, B, R, torch.float32, seed=3)
    _check(_device(rmat, edges, x, coeff, g), _reference(rmat, edges, x, coeff, g), torch.float32, "R * B = %d > %d" % (R * B, cap))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_edge_case_rows(edge_graph, dtype):
    edges = _edges(edge_graph, 7)
    x, coeff, g = _inputs(edge_graph, 32, 3, 7, dtype, seed=11)
    got = _device(edge_graph, edges, x, coeff, g)
    _check(got, _reference(edge_graph, edges, x, coeff, g), dtype, "edge rows")
    assert got[0][0].abs().max().item() == 0.0 and got[0][69].abs().max().item() == 0.0     # the empty rows
    assert got[1][89].abs().max().item() == 0.0                                            # the source no row references


# ---- exactness: integer data whose every partial sum is exact in fp32, so the result must EQUAL the reference ------------------------
def _exact_data(graph, F, B, R, dtype, seed):
    from dgll_amd.ops_typed import TypedEdges

    gen = torch.Generator().manual_seed(seed)
    ints = lambda *shape: torch.randint(-2, 3, shape, generator=gen).float()        # noqa: E731
    x, coeff, g = ints(graph.n_cols, F).to(dtype).to(DEV), ints(R, B).to(DEV), ints(graph.n_rows, B * F).to(dtype).to(DEV)
    norm = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (graph.nnz,), generator=gen)].to(DEV)
    return TypedEdges(graph, _hash_types(graph, R).to(DEV), R, norm), x, coeff, g


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("F,B,R", [(64, 3, 5), (16, 9, 4)])
def test_exact_on_integer_data(edge_graph, F, B, R, dtype):
    edges, x, coeff, g = _exact_data(edge_graph, F, B, R, dtype, seed=F + B)
    # sum |term| of every output element: every term is a multiple of 0.5 (norm), so sums below 2^23 (a fortiori the 2^24 of whole
    # numbers) are exact in fp32 in any order -- Z, dX and dC (whose terms are norm_e <x_j, dZ[i, b, :]>, themselves sums of terms)
    mags = _reference(edge_graph, edges, x.abs(), coeff.abs(), g.abs())
    for name, m in zip(NAMES, mags):
        assert m.max().item() < 2 ** 23, name
    want = _reference(edge_graph, edges, x, coeff, g)
    z, dx, dc = _device(edge_graph, edges, x, coeff, g)
    assert torch.equal(z.cpu(), want[0].to(dtype)), "z"            # bf16: ONE round-to-nearest-even of an exactly known number
    assert torch.equal(dx.cpu(), want[1].to(dtype)), "dx"
    assert torch.equal(dc.cpu(), want[2].float()), "dc"


def test_exactness_reference_has_power(edge_graph):
    """On the reference alone: dropping one edge of the 3000-entry row, or swapping the types of two of its edges, changes Z."""
    edges, x, coeff, g = _exact_data(edge_graph, 64, 3, 5, torch.float32, seed=67)
    rowptr, col, ety, norm = edge_graph.rowptr.cpu(), edge_graph.col.cpu(), edges.etypes.cpu(), edges.norm.cpu()
    base = typed_spmm_reference(rowptr, col, ety, norm, x.cpu(), coeff.cpu())
    b, e = int(rowptr[7]), int(rowptr[8])
    assert e - b == 3000
    keep = torch.ones(col.numel(), dtype=torch.bool)
    keep[b] = False
    dropped_ptr = rowptr.clone()
    dropped_ptr[8:] -= 1
    dropped = typed_spmm_reference(dropped_ptr, col[keep], ety[keep], norm[keep], x.cpu(), coeff.cpu())
    assert not torch.equal(dropped[7], base[7]) and torch.equal(dropped[8:], base[8:]) and torch.equal(dropped[:7], base[:7])
    other = b + 1 + int(((ety[b + 1:e] != ety[b]) & (col[b + 1:e] != col[b])).nonzero()[0])
    swapped_types = ety.clone()
    swapped_types[b], swapped_types[other] = ety[other], ety[b]
    swapped = typed_spmm_reference(rowptr, col, swapped_types, norm, x.cpu(), coeff.cpu())
    assert not torch.equal(swapped[7], base[7])


# ---- layout and bounds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_layout_and_bounds(edge_graph, dtype):
    from dgll_amd import ops_typed

    F, B, R = 24, 3, 5
    epv = 4 if dtype == torch.float32 else 8
    pad = 2 * epv
    edges = _edges(edge_graph, R)
    x, coeff, g = _inputs(edge_graph, F, B, R, dtype, seed=29)
    xbuf = torch.full((90, F + pad), float("nan"), dtype=dtype, device=DEV)       # NaN in the padding columns ...
    xbuf[:89, :F] = x[:89]                                                        # ... and in the row of the never-referenced source
    xv = xbuf[:, :F]
    gbuf = torch.full((70, B * F + pad), float("nan"), dtype=dtype, device=DEV)
    gbuf[:, :B * F] = g
    gv = gbuf[:, :B * F]
    zbuf = torch.full((70, B * F + pad), 7.0, dtype=dtype, device=DEV)
    z = ops_typed.typed_spmm_forward_raw(edge_graph, edges, xv, coeff, out=zbuf[:, :B * F])
    assert bool((zbuf[:, B * F:] == 7.0).all())                                   # Z's pitch padding keeps its sentinel
    assert bool(torch.isfinite(z).all())
    assert z[0].abs().max().item() == 0.0 and z[69].abs().max().item() == 0.0     # the empty rows
    dx, dc = ops_typed.typed_spmm_backward_raw(edge_graph, edges, xv, coeff, gv)
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dc).all())
    assert dx[89].abs().max().item() == 0.0                                       # the unreferenced source
    p = torch.full((edge_graph.nnz, 4), float("nan"), dtype=torch.float32, device=DEV)
    ops_typed._launch(ops_typed._lib.TYPED_EDGE_DOTS, edge_graph, None, None, R, B, F, None, x=xv, dz=gv, p=p)
    assert bool(torch.isfinite(p).all()) and p[:, B:].abs().max().item() == 0.0    # P's padding column
    want = _reference(edge_graph, edges, x[:89].new_zeros(90, F).index_copy_(0, torch.arange(89, device=DEV), x[:89]), coeff, g)
    _check((z, dx, dc), want, dtype, "padded buffers")


# ---- reproducibility and capture ------------------------------------------------------------------------------------------------------
def test_reruns_are_bit_identical(rmat):
    edges = _edges(rmat, 16)
    x, coeff, g = _inputs(rmat, 64, 4, 16, torch.bfloat16, seed=41)
    a, b = _device(rmat, edges, x, coeff, g), _device(rmat, edges, x, coeff, g)
    for name, u, v in zip(NAMES, a, b):
        assert torch.equal(u, v), name


def test_forward_backward_can_be_captured(rmat):
    from dgll_amd import ops_typed

    edges = _edges(rmat, 16)
    x, coeff, g = _inputs(rmat, 64, 4, 16, torch.bfloat16, seed=81)
    x, coeff = x.requires_grad_(), coeff.requires_grad_()

    def step():
        z = ops_typed.typed_spmm(rmat, edges, x, coeff)
        return (z.detach(),) + tuple(torch.autograd.grad(z, (x, coeff), g))

    eager = [t.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static = step()
    for t in static:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(NAMES, static, eager):
        assert torch.equal(a, b), name


# ---- identities that tie it to the existing kernels -----------------------------------------------------------------------------------
def test_one_basis_of_ones_is_the_weighted_spmm(rmat):
    from dgll_amd import ops, ops_typed

    edges = _edges(rmat, 3)
    x, _, _ = _inputs(rmat, 64, 1, 3, torch.float32, seed=51)
    z = ops_typed.typed_spmm(rmat, edges, x, torch.ones(3, 1, device=DEV))
    want = ops.spmm(rmat.with_values(edges.norm), x)
    assert (z - want).abs().max().item() <= 1e-6 * want.abs().max().item()


def test_identity_table_splits_the_graph_by_type(rmat):
    from dgll_amd import CSRGraph, ops, ops_typed

    R, F = 4, 32
    edges = _edges(rmat, R)
    x, _, _ = _inputs(rmat, F, R, R, torch.float32, seed=52)
    z = ops_typed.typed_spmm(rmat, edges, x, torch.eye(R, device=DEV))
    row = rmat.row_index()
    for r in range(R):
        sel = (edges.etypes == r).nonzero().flatten()
        sub = CSRGraph.from_coo(row[sel], rmat.col[sel].long(), edges.norm[sel], (1024, 1024), coalesce=False)
        want = ops.spmm(sub, x)
        assert (z[:, r * F:(r + 1) * F] - want).abs().max().item() <= 1e-6 * want.abs().max().item(), r


def test_input_handling(rmat):
    from dgll_amd import CSRGraph, ops_typed

    edges = _edges(rmat, 3)
    coeff = torch.ones(3, 2, device=DEV)
    with pytest.raises(ValueError, match="pads"):                  # 6 fp32 columns: no whole number of 16-byte vectors
        ops_typed.typed_spmm(rmat, edges, torch.ones(1024, 6, device=DEV), coeff)
    with pytest.raises(ValueError):
        ops_typed.typed_spmm(rmat, edges, torch.ones(1000, 8, device=DEV), coeff)
    with pytest.raises(ValueError):
        ops_typed.typed_spmm(rmat, edges, torch.ones(1024, 8, device=DEV), torch.ones(4, 2, device=DEV))
    # a view whose rows are not on a 16-byte pitch is copied once (as_rows16) and gives the same result
    x = torch.randn(1024, 9, device=DEV)
    assert torch.equal(ops_typed.typed_spmm(rmat, edges, x[:, 1:], coeff), ops_typed.typed_spmm(rmat, edges, x[:, 1:].contiguous(), coeff))
    # no entries: zeros with zero gradients, no launch
    empty = CSRGraph(torch.zeros(6, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), None, 5, 7)
    none = ops_typed.TypedEdges(empty, torch.zeros(0, dtype=torch.int64, device=DEV), 3)
    xe, ce = torch.ones(7, 8, device=DEV, requires_grad=True), coeff.clone().requires_grad_()
    z = ops_typed.typed_spmm(empty, none, xe, ce)
    gx, gc = torch.autograd.grad(z.sum(), (xe, ce))
    assert z.shape == (5, 16) and z.abs().max().item() == 0.0 and gx.abs().max().item() == 0.0 and gc.abs().max().item() == 0.0


# ---- the layer ------------------------------------------------------------------------------------------------------------------------
class _RoundBf16(torch.autograd.Function):
    """Rounds to bf16 on the way forward and the gradient on the way back: a bf16 tensor of the device path."""

    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _emulated_layer(layer, graph, edges, feat, relu):
    """The layer in float64 torch on the host with the operands rounded to bf16 where the device path holds bf16: the features, Z, the
    weights and the bias inside the products and sums, every stored product / sum (the one-launch transform stores once; the other
    path stores the basis product, the normalised rows, the sum with the bias, the loop product and the sum with it), and the gradients of those tensors."""
    rnd = _RoundBf16.apply
    wr = lambda w: w + (w.detach().to(torch.bfloat16).double() - w.detach())         # noqa: E731  (bf16 inside the product, fp32 gradient)
    W, coeff = layer.linear_r.W, layer._coeff()
    z = rnd(typed_spmm_reference(graph.rowptr, graph.col, edges.etypes, edges.norm, feat, coeff))
    vstack = wr(W).reshape(-1, W.shape[2])
    feat_dst = feat[:graph.n_rows]
    one_launch = layer.loop_weight is not None and layer.layer_norm_weight is None and not (relu and layer.h_bias is not None)
    if one_launch:
        h = z @ vstack + feat_dst @ wr(layer.loop_weight)
        h = rnd(torch.relu(h) if relu else h)
        if layer.h_bias is not None:
            h = rnd(h + rnd(layer.h_bias))
        return h
    h = rnd(z @ vstack)
    if layer.layer_norm_weight is not None:
        ln = layer.layer_norm_weight
        h = rnd(torch.nn.functional.layer_norm(h, ln.normalized_shape, rnd(ln.weight), rnd(ln.bias), ln.eps))
    if layer.h_bias is not None:
        h = rnd(h + rnd(layer.h_bias))
    if layer.loop_weight is not None:
        h = rnd(h + rnd(feat_dst @ wr(layer.loop_weight)))
    return rnd(torch.relu(h)) if relu else h


def _layer_case(name):
    """(layer, graph slice, R): the four shapes of the layer check."""
    from dgll_amd.nn.Convolution import RelGraphConv

    torch.manual_seed(61)
    if name == "64x32":
        return RelGraphConv(64, 32, 16, regularizer="basis", num_bases=4, activation=torch.relu), None, 16
    if name == "19x7-padded":
        return RelGraphConv(19, 7, 16, regularizer="basis", num_bases=4, bias=False, activation=torch.relu), None, 16
    if name == "block-300x1024":
        return RelGraphConv(32, 16, 16, regularizer="basis", num_bases=4), 300, 16
    return RelGraphConv(16, 8, 4, regularizer=None, layer_norm=True), None, 4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", ["64x32", "19x7-padded", "block-300x1024", "none-R4"])
def test_layer_against_the_reference(rmat, case, dtype):
    from dgll_amd import CSRGraph
    from dgll_amd.ops_typed import TypedEdges

    layer, n_dst, R = _layer_case(case)
    graph = rmat
    if n_dst is not None:
        cut = int(rmat.rowptr[n_dst])
        graph = CSRGraph(rmat.rowptr[:n_dst + 1].clone(), rmat.col[:cut].clone(), None, n_dst, 1024)
    edges = _edges(graph, R, seed=5)
    if layer.h_bias is not None:
        torch.nn.init.normal_(layer.h_bias, std=0.1)
    relu = layer.activation is not None
    host = copy.deepcopy(layer).double()
    host_graph = graph.to("cpu")
    host_edges = TypedEdges(host_graph, edges.etypes.cpu(), R, edges.norm.cpu())
    gen = torch.Generator().manual_seed(7)
    feat = torch.randn(1024, layer.in_feat, generator=gen).to(dtype)
    g = torch.randn(graph.n_rows, layer.out_feat, generator=gen).to(dtype)
    names = ["out", "input"] + [n for n, _ in layer.named_parameters()]

    def run(fn, params, leaf, gout):
        out = fn(leaf)
        return [out.detach()] + list(torch.autograd.grad(out, [leaf] + params, gout))

    sd = dict(host.named_parameters())
    ref_leaf = feat.double().requires_grad_()
    want = run(lambda f: relgraphconv_reference(host_graph.rowptr, host_graph.col, host_edges.etypes, host_edges.norm, f, sd["linear_r.W"],
                                                sd.get("linear_r.coeff"), sd.get("h_bias"), sd.get("loop_weight"),
                                                sd.get("layer_norm_weight.weight"), sd.get("layer_norm_weight.bias"), torch.relu if relu else None),
               list(host.parameters()), ref_leaf, g.double())
    bars = None
    if dtype == torch.bfloat16:
        emu_leaf = feat.double().requires_grad_()
        emu = run(lambda f: _emulated_layer(host, host_graph, host_edges, f, relu), list(host.parameters()), emu_leaf, g.double())
        bars = {}
        for name, a, b in zip(names, emu, want):
            e = ((a - b).abs().max() / b.abs().max()).item() if name == "out" else ((a - b).norm() / b.norm()).item()
            bars[name] = 2.0 * e + 1e-4
            print("%s bf16 emulation %-22s error %.3e -> bar %.3e" % (case, name, e, bars[name]))
    dev_layer = layer.to(DEV)
    dev_leaf = feat.to(DEV).requires_grad_()
    got = run(lambda f: dev_layer(graph, f, edges), list(dev_layer.parameters()), dev_leaf, g.to(DEV))
    assert got[0].shape == (graph.n_rows, layer.out_feat) and got[0].dtype == dtype
    _check(got, want, dtype, case, names=names, bf16_bars=bars)


def test_layer_loads_a_dgl_state_dict(rmat):
    from dgll_amd.nn.Convolution import RelGraphConv

    torch.manual_seed(3)
    gen = torch.Generator().manual_seed(4)
    sd = {"linear_r.W": torch.randn(3, 16, 8, generator=gen) * 0.2, "linear_r.coeff": torch.randn(6, 3, generator=gen),
          "h_bias": torch.randn(8, generator=gen), "loop_weight": torch.randn(16, 8, generator=gen) * 0.2}
    layer = RelGraphConv(16, 8, 6, regularizer="basis", num_bases=3)
    layer.load_state_dict(sd, strict=True)
    edges = _edges(rmat, 6)
    feat = torch.randn(1024, 16, generator=gen)
    out = layer.to(DEV)(rmat, feat.to(DEV), edges)
    want = relgraphconv_reference(rmat.rowptr, rmat.col, edges.etypes, edges.norm.cpu(), feat, sd["linear_r.W"], sd["linear_r.coeff"],
                                  sd["h_bias"], sd["loop_weight"])
    assert (out.double().cpu() - want).abs().max().item() <= 1e-4 * want.abs().max().item()


def test_model_trains_on_typed_labels():
    """Two-layer RGCN on synth.typed_graph (labels: a function of WHICH edge types reach a node; a constant feature column lets a sum
    over typed neighbours say so): the loss falls and the training nodes are fitted.  On host tensors the same run takes the loss from
    about 2 to below 1e-3; the bars leave three decades for the arithmetic of the device path."""
    from dgll_amd import synth
    from dgll_amd.nn.Convolution import RGCN
    from dgll_amd.ops_typed import typed_graph_from_coo

    d = synth.typed_graph(9, num_rels=6, n_classes=4, seed=1, device=DEV)
    graph, edges = typed_graph_from_coo(d["src"], d["dst"], d["etypes"], d["norm"], d["num_nodes"], d["num_nodes"], d["num_rels"])
    torch.manual_seed(0)
    model = RGCN(16, 32, 4, d["num_rels"], 3).to(DEV)
    feat = torch.randn(d["num_nodes"], 16)
    feat[:, 0] = 1.0
    feat = feat.to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=2e-2)
    first = None
    for _ in range(60):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(graph, feat, edges).float(), d["labels"])
        loss.backward()
        opt.step()
        first = loss.item() if first is None else first
    acc = (model(graph, feat, edges).argmax(1) == d["labels"]).float().mean().item()
    print("rgcn: loss %.3f -> %.4f, accuracy %.3f" % (first, loss.item(), acc))
    assert loss.item() < 0.1 * first and acc > 0.95
