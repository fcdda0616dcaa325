"""nn.GMMConv / nn.MoNet / ops_gmm without a GPU: the state dict and the initialisers of DGL's GMMConv, the layer on host tensors against
the float64 restatement of gmm_ref.py (fp64 1e-10, fp32 1e-5 of max |ref|), pairs of features and sampler blocks (n_dst < n_src), every
argument check of ops_gmm.gmm_expand, the refused aggregator, and MoNet with degree_pseudo on a 6-node graph."""
import math

import pytest
import torch

import gmm_ref
from test_pna_emulated import _graph


def _close(got, want, bar):
    err = ((got.double() - want).abs().max() / want.abs().max()).item()
    assert err <= bar, err


def test_state_dict_and_shapes():
    from dgll_amd.nn import GMMConv

    layer = GMMConv(5, 7, 2, 3, residual=True)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == {
        "mu": (3, 2), "inv_sigma": (3, 2), "bias": (7,), "fc.weight": (21, 5), "res_fc.weight": (7, 5)}
    same = GMMConv(7, 7, 2, 3, residual=True)              # equal widths: the residual is the identity and owns no parameter
    assert sorted(same.state_dict()) == ["bias", "fc.weight", "inv_sigma", "mu"]
    assert isinstance(same.res_fc, torch.nn.Identity)
    plain = GMMConv((5, 4), 7, 3, 2, bias=False)
    assert sorted(plain.state_dict()) == ["fc.weight", "inv_sigma", "mu"] and plain.res_fc is None and plain.bias is None
    pair = GMMConv((5, 4), 7, 3, 2, residual=True)
    assert tuple(pair.res_fc.weight.shape) == (7, 4) and tuple(pair.fc.weight.shape) == (14, 5)


def test_initialisers():
    from dgll_amd.nn import GMMConv

    torch.manual_seed(0)
    layer = GMMConv(200, 100, 8, 64, residual=True)
    gain = math.sqrt(2.0)
    assert torch.equal(layer.inv_sigma, torch.ones(64, 8)) and torch.equal(layer.bias, torch.zeros(100))
    assert abs(layer.mu.std().item() - 0.1) < 0.02 and abs(layer.mu.mean().item()) < 0.02
    for w in (layer.fc.weight, layer.res_fc.weight):        # Xavier-normal with the ReLU gain
        want = gain * math.sqrt(2.0 / (w.shape[0] + w.shape[1]))
        assert abs(w.std().item() / want - 1.0) < 0.05


def _layer_case(dtype, reduce, residual, in_feats, graph, seed=3):
    from dgll_amd.nn import GMMConv

    torch.manual_seed(seed)
    K, dim, out = 3, 2, 6
    layer = GMMConv(in_feats, out, dim, K, aggregator_type=reduce, residual=residual, allow_zero_in_degree=True).to(dtype)
    with torch.no_grad():
        layer.mu.copy_(0.5 * torch.randn(K, dim))
        layer.inv_sigma.copy_(0.5 + 1.5 * torch.rand(K, dim))
        layer.bias.copy_(torch.randn(out))
    pair = isinstance(in_feats, tuple)
    fs, fd = in_feats if pair else (in_feats, in_feats)
    x_src = torch.randn(graph.n_cols, fs, dtype=dtype)
    x_dst = torch.randn(graph.n_rows, fd, dtype=dtype) if pair else x_src[:graph.n_rows]
    pseudo = (torch.rand(graph.nnz, dim) * 2 - 1).to(dtype)
    got = layer(graph, (x_src, x_dst) if pair else x_src, pseudo)
    res_w = layer.res_fc.weight if isinstance(layer.res_fc, torch.nn.Linear) else None
    want = gmm_ref.layer(graph.rowptr, graph.col, x_src, x_dst, pseudo, layer.mu.detach(), layer.inv_sigma.detach(), layer.fc.weight.detach(),
                         None if res_w is None else res_w.detach(), layer.bias.detach(), reduce, residual)
    assert got.shape == (graph.n_rows, out) and got.dtype == dtype
    _close(got.detach(), want, 1e-10 if dtype == torch.float64 else 1e-5)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("residual", [False, True])
def test_layer_on_host_tensors(dtype, reduce, residual):
    _layer_case(dtype, reduce, residual, 5, _graph(full=True))        # a block: 24 destinations of 30 sources (the first 24)
    _layer_case(dtype, reduce, residual, 6, _graph(full=False))       # in == out: the identity residual


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_pairs_and_blocks(reduce):
    g = _graph(full=True)
    assert g.n_rows < g.n_cols
    _layer_case(torch.float64, reduce, True, (5, 4), g)
    _layer_case(torch.float64, reduce, True, (5, 6), g)              # in_dst == out: identity on feat_dst


def test_host_path_gradients_match_the_reference():
    from dgll_amd.nn.Convolution.gmmconv import _host_aggregate

    g = _graph(full=False)
    x, pseudo, mu, sigma, go = gmm_ref.inputs(g, 4, 3, 2, torch.float64, 5)
    leaves = [t.double().requires_grad_() for t in (x, pseudo, mu, sigma)]
    for reduce in ("sum", "mean"):
        z = _host_aggregate(g, *leaves, reduce)
        _close(z.detach(), gmm_ref.expand(g.rowptr, g.col, x, pseudo, mu, sigma, reduce), 1e-12)
        grads = torch.autograd.grad(z, leaves, go.double())
        want = gmm_ref.gradients(g.rowptr, g.col, x, pseudo, mu, sigma, go, reduce)[:4]
        for a, b in zip(grads, want):
            _close(a, b, 1e-10)


def test_zero_in_degree():
    from dgll_amd.nn import GMMConv

    g = _graph(full=False)
    layer = GMMConv(4, 4, 2, 3)
    with pytest.raises(ValueError, match="allow_zero_in_degree"):
        layer(g, torch.randn(g.n_cols, 4), torch.rand(g.nnz, 2))
    layer.set_allow_zero_in_degree(True)
    out = layer(g, torch.randn(g.n_cols, 4), torch.rand(g.nnz, 2))
    assert torch.equal(out[0], layer.bias.detach()) and torch.equal(out[-1], layer.bias.detach())     # rows without entries: the bias alone


def test_max_and_bad_arguments_raise():
    from dgll_amd.nn import GMMConv

    with pytest.raises(NotImplementedError, match='"sum".*"mean"'):
        GMMConv(4, 4, 2, 3, aggregator_type="max")
    with pytest.raises(ValueError, match="aggregator_type"):
        GMMConv(4, 4, 2, 3, aggregator_type="min")
    with pytest.raises(ValueError, match="dim"):
        GMMConv(4, 4, 9, 3)
    with pytest.raises(ValueError, match="n_kernels"):
        GMMConv(4, 4, 2, 65)
    g = _graph(full=False)
    layer = GMMConv(4, 4, 2, 3, allow_zero_in_degree=True)
    with pytest.raises(ValueError, match="pseudo"):
        layer(g, torch.randn(g.n_cols, 4), torch.rand(g.nnz, 3))
    with pytest.raises(ValueError, match="features"):
        layer(g, torch.randn(g.n_cols, 5), torch.rand(g.nnz, 2))


def test_op_argument_checks():
    """every check of ops_gmm.gmm_expand comes before anything touches a GPU: host tensors that pass them all raise RuntimeError"""
    from dgll_amd import ops_gmm

    g = _graph(full=False)
    x, ps, mu, sg = torch.randn(g.n_cols, 8), torch.rand(g.nnz, 2), torch.zeros(3, 2), torch.ones(3, 2)
    with pytest.raises(TypeError, match="CSRGraph"):
        ops_gmm.gmm_expand(None, x, ps, mu, sg)
    with pytest.raises(ValueError, match="reduce"):
        ops_gmm.gmm_expand(g, x, ps, mu, sg, reduce="max")
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        ops_gmm.gmm_expand(g, x.double(), ps, mu, sg)
    with pytest.raises(ValueError, match="the layers pad"):
        ops_gmm.gmm_expand(g, torch.randn(g.n_cols, 6), ps, mu, sg)
    with pytest.raises(ValueError, match="the layers pad"):
        ops_gmm.gmm_expand(g, torch.randn(g.n_cols, 12).bfloat16(), ps, mu, sg)
    with pytest.raises(ValueError, match="rows"):
        ops_gmm.gmm_expand(g, torch.randn(g.n_cols + 1, 8), ps, mu, sg)
    with pytest.raises(ValueError, match=r"pseudo must be .*\[nnz, dim\]"):
        ops_gmm.gmm_expand(g, x, ps[:-1], mu, sg)
    with pytest.raises(ValueError, match=r"pseudo must be .*\[nnz, dim\]"):
        ops_gmm.gmm_expand(g, x, ps.long(), mu, sg)
    with pytest.raises(ValueError, match=r"mu must be .*\[K, dim\]"):
        ops_gmm.gmm_expand(g, x, ps, torch.zeros(3, 3), sg)
    with pytest.raises(ValueError, match=r"inv_sigma must be .*\[K, dim\]"):
        ops_gmm.gmm_expand(g, x, ps, mu, torch.ones(3))
    with pytest.raises(ValueError, match="one shape"):
        ops_gmm.gmm_expand(g, x, ps, mu, torch.ones(4, 2))
    with pytest.raises(ValueError, match="dim must be in 1..8"):
        ops_gmm.gmm_expand(g, x, torch.rand(g.nnz, 9), torch.zeros(3, 9), torch.ones(3, 9))
    with pytest.raises(ValueError, match="K must be in 1..64"):
        ops_gmm.gmm_expand(g, x, ps, torch.zeros(65, 2), torch.ones(65, 2))
    with pytest.raises(RuntimeError, match="GPU"):
        ops_gmm.gmm_expand(g, x, ps, mu, sg)


def test_monet_and_degree_pseudo_on_six_nodes():
    from dgll_amd import CSRGraph
    from dgll_amd.nn import MoNet, degree_pseudo

    # rows (destinations) 0..5 with 2, 1, 0, 3, 1, 1 entries
    rowptr = torch.tensor([0, 2, 3, 3, 6, 7, 8])
    col = torch.tensor([1, 3, 0, 0, 2, 5, 3, 4], dtype=torch.int32)
    g = CSRGraph(rowptr, col, None, 6, 6)
    deg = torch.tensor([2.0, 1.0, 0.0, 3.0, 1.0, 1.0])
    row = gmm_ref.row_index(rowptr)
    want = torch.stack([(deg[row] + 1).rsqrt(), (deg[col.long()] + 1).rsqrt()], 1)
    ps = degree_pseudo(g)
    assert ps.shape == (8, 2) and torch.allclose(ps, want, atol=1e-7)

    torch.manual_seed(0)
    model = MoNet(4, 8, 3, dim=2, n_kernels=3, n_layers=2)
    assert len(model.layers) == 2 and len(model.pseudo_proj) == 2
    assert isinstance(model.pseudo_proj[0][0], torch.nn.Linear) and isinstance(model.pseudo_proj[0][1], torch.nn.Tanh)
    assert (model.pseudo_proj[0][0].in_features, model.pseudo_proj[0][0].out_features) == (2, 2)
    x = torch.randn(6, 4)
    out = model(g, x)                                       # degree_pseudo by default
    assert out.shape == (6, 3) and torch.equal(out, model(g, x, ps))
    # layer by layer against the reference
    h = x.double()
    for k, (layer, proj) in enumerate(zip(model.layers, model.pseudo_proj)):
        u = torch.tanh(ps.double() @ proj[0].weight.detach().double().t() + proj[0].bias.detach().double())
        h = gmm_ref.layer(rowptr, col, h, h, u, layer.mu.detach(), layer.inv_sigma.detach(), layer.fc.weight.detach(), None,
                          layer.bias.detach(), "sum", False)
        if k == 0:
            h = torch.relu(h)
    _close(out.detach(), h, 1e-5)
    out.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
