"""Attention dropout drawn inside the second-generation GAT passes (gat2_kernel<..., DROP>, csrc/gat_dropout.hpp): the device mask
against the host one, the three passes against CPU autograd and against the first-generation kernels fed the same mask as an
edge_scale array, SpGAT in training mode layer by layer and under graph capture, and the memory the step no longer needs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED_WORDS = (0x1234ABCD, 0x0F1E2D3C)
P = 0.6
CASES = [(8, 32), (4, 8), (1, 48), (2, 24)]
DTYPES = [torch.float32, torch.bfloat16]


def _seed(device, words=SEED_WORDS):
    return torch.from_numpy(np.array(words, np.uint32).view(np.int32).copy()).to(device)


def _graph(device, n=600, seed=5):
    """Self-loops, short rows, and one row of 500 edges: above the plan's long-row threshold, so it runs as chunks + finalize."""
    import dgll_amd

    rng = np.random.default_rng(seed)
    dense = rng.random((n, n)) < 6.0 / n
    dense[0, rng.choice(n, 500, replace=False)] = True
    np.fill_diagonal(dense, True)
    r, c = np.nonzero(dense)
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rowptr[1:])
    g_cpu = dgll_amd.CSRGraph(torch.from_numpy(rowptr), torch.from_numpy(c.astype(np.int32)), None, n, n)
    g = g_cpu.to(device)
    assert g.num_long_rows() >= 1
    return g_cpu, g


def _host_mask(g_cpu, heads, p, seed):
    from dgll_amd import ops

    return ops.gat_dropout_mask(g_cpu, heads, p, seed.cpu())


def _close(name, got, want, dtype, grad):
    """The project's bars for these quantities: fp32 rtol/atol 1e-4/1e-5 forward, 2e-3/2e-4 gradients (tests/test_ops_gpu.py);
    bf16 2e-2 of the largest reference value (tests/test_gat_strided_gpu.py)."""
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    assert torch.isfinite(got).all(), name
    err, top = float((got - want).abs().max()), float(want.abs().max())
    print("%-28s %s max |err| %.3e  max |ref| %.3e" % (name, str(dtype).replace("torch.", ""), err, top))
    if dtype == torch.bfloat16:
        assert err <= 2e-2 * top, (name, err, top)
    else:
        rtol, atol = (2e-3, 2e-4) if grad else (1e-4, 1e-5)
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=rtol, atol=atol, err_msg=name)


def _reference(g_cpu, h, s, t, mask, heads, fo, gout, A=None):
    """CPU autograd of the formula (tests/test_ops_gpu.py's, mode 0): the multipliers apply AFTER the row sum.  A given: s, t = h . A."""
    n = g_cpu.n_rows
    row, col = g_cpu.row_index(), g_cpu.col.long()
    h = h.clone().requires_grad_()
    leaves = [h]
    if A is not None:
        A = A.clone().requires_grad_()
        st = h @ A
        s, t = st[:, :heads], st[:, heads:]
        leaves.append(A)
    else:
        s, t = s.clone().requires_grad_(), t.clone().requires_grad_()
        leaves += [s, t]
    w = torch.exp(-torch.nn.functional.leaky_relu(s[row] + t[col], 0.2))
    den = torch.zeros(n, heads).index_add_(0, row, w)
    num = torch.zeros(n, heads, fo).index_add_(0, row, (w * mask)[:, :, None] * h.view(-1, heads, fo)[col])
    out = torch.nn.functional.elu(num / den[:, :, None]).reshape(n, heads * fo)
    grads = torch.autograd.grad(out, leaves, gout)
    return (out.detach(),) + grads


def _inputs(n, heads, fo, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    h = (torch.randn(n, heads * fo, generator=gen) * 0.5).to(dtype).float()
    s, t = torch.randn(n, heads, generator=gen) * 0.5, torch.randn(n, heads, generator=gen) * 0.5
    A = torch.zeros(heads * fo, 2 * heads)
    for k in range(heads):
        A[k * fo:(k + 1) * fo, k] = torch.randn(fo, generator=gen) * 0.3
        A[k * fo:(k + 1) * fo, heads + k] = torch.randn(fo, generator=gen) * 0.3
    A = A.to(dtype).float()
    gout = torch.randn(n, heads * fo, generator=gen).to(dtype).float()
    return h, s, t, A, gout


def test_device_mask_equals_host_mask(cuda_device):
    from dgll_amd import ops

    g_cpu, g = _graph(cuda_device, n=3000, seed=9)
    for words in (SEED_WORDS, (0xFFFFFFFF, 1)):
        for heads in (1, 3, 8, 10):
            for p in (0.1, 0.6):
                seed = _seed(cuda_device, words)
                dev = ops.gat_dropout_mask(g, heads, p, seed)
                assert torch.equal(dev.cpu(), _host_mask(g_cpu, heads, p, seed))
                assert 0 < int((dev == 0).sum()) < dev.numel()


@pytest.mark.parametrize("row_scores", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,fo", CASES)
def test_passes_with_dropout_match_cpu_autograd_and_first_generation(cuda_device, monkeypatch, heads, fo, dtype, row_scores):
    """ops.gat_aggregate (grad_h, grad_s, grad_t) and ops.gat_layer (grad_h, grad_A) with (p, seed) against
    (a) CPU autograd with the host mask, (b) the first-generation kernels with that mask as edge_scale (per-head width padded to a
    power of two of vectors where they need it).  row_scores False = DGLL_GAT_ROW_SCORES=0 / DGLL_GAT_ROW_SCORES_BWD=0: the record-phase
    forms of the forward and the rows pass."""
    from dgll_amd import ops, ops_edge

    monkeypatch.setattr(ops_edge, "ROW_SCORES", row_scores)
    monkeypatch.setattr(ops_edge, "ROW_SCORES_BWD", row_scores)
    d = cuda_device
    g_cpu, g = _graph(d)
    n = g.n_rows
    h, s, t, A, gout = _inputs(n, heads, fo, dtype, seed=heads * 100 + fo)
    seed = _seed(d)
    mask = _host_mask(g_cpu, heads, P, seed)
    tag = "%dx%d %s" % (heads, fo, "rowscore" if row_scores else "records")

    # ---- gat_aggregate: explicit scores
    ref_out, ref_gh, ref_gs, ref_gt = _reference(g_cpu, h, s, t, mask, heads, fo, gout)
    hd, sd, td = h.to(d).to(dtype).requires_grad_(), s.to(d).requires_grad_(), t.to(d).requires_grad_()
    with ops.LaunchTimer() as timer:
        out = ops.gat_aggregate(g, hd, sd, td, heads, 0.2, apply_elu=True, mode=0, dropout_p=P, dropout_seed=seed)
        gh, gs, gt = torch.autograd.grad(out, (hd, sd, td), gout.to(d).to(dtype))
    tags = [k for k in timer.summary() if k[0] == "gat"]
    assert len(tags) == 3 and all("dropout" in k[-1] for k in tags), tags
    _close(tag + " aggregate out", out, ref_out, dtype, False)
    _close(tag + " aggregate grad_h", gh, ref_gh, dtype, True)
    _close(tag + " aggregate grad_s", gs, ref_gs, dtype, True)
    _close(tag + " aggregate grad_t", gt, ref_gt, dtype, True)

    # (b) first generation, the mask as an array; heads padded to a power-of-two number of 16-byte vectors
    fo1 = ops.head_width_padded(fo, dtype, pow2=True)
    pad = lambda x: torch.nn.functional.pad(x.view(n, heads, fo), (0, fo1 - fo)).reshape(n, heads * fo1)     # noqa: E731
    h1, s1, t1 = pad(h).to(d).to(dtype).requires_grad_(), s.to(d).requires_grad_(), t.to(d).requires_grad_()
    out1 = ops.gat_aggregate(g, h1, s1, t1, heads, 0.2, apply_elu=True, mode=0, edge_scale=mask.to(d))
    gh1, gs1, gt1 = torch.autograd.grad(out1, (h1, s1, t1), pad(gout).to(d).to(dtype))
    unpad = lambda x: x.view(n, heads, fo1)[:, :, :fo].reshape(n, heads * fo)                                 # noqa: E731
    _close(tag + " vs gen1 out", out, unpad(out1), dtype, False)
    _close(tag + " vs gen1 grad_h", gh, unpad(gh1), dtype, True)
    _close(tag + " vs gen1 grad_s", gs, gs1, dtype, True)
    _close(tag + " vs gen1 grad_t", gt, gt1, dtype, True)

    # ---- gat_layer: scores formed from h (the row-score forms when enabled), score gradients in the transposed pass's epilogue
    ref_out, ref_gh, ref_gA = _reference(g_cpu, h, None, None, mask, heads, fo, gout, A=A)
    hd, Ad = h.to(d).to(dtype).requires_grad_(), A.to(d).requires_grad_()
    with ops.LaunchTimer() as timer:
        out = ops.gat_layer(g, hd, Ad, heads, 0.2, apply_elu=True, pack_scores=True, dropout_p=P, dropout_seed=seed)
        gh, gA = torch.autograd.grad(out, (hd, Ad), gout.to(d).to(dtype), retain_graph=True)
    tags = [k for k in timer.summary() if k[0] == "gat"]
    assert len(tags) == 3 and all("dropout" in k[-1] for k in tags), tags
    assert sum("rowscore" in k[-1] for k in tags) == (2 if row_scores else 0), tags
    nz = A != 0
    _close(tag + " layer out", out, ref_out, dtype, False)
    _close(tag + " layer grad_h", gh, ref_gh, dtype, True)
    _close(tag + " layer grad_A", gA.cpu()[nz], ref_gA[nz], dtype, True)

    # the backward draws the forward's mask again: a second backward from the same forward gives the same gradients
    gh2, gA2 = torch.autograd.grad(out, (hd, Ad), gout.to(d).to(dtype))
    assert torch.equal(gh, gh2) and torch.equal(gA, gA2)
    # another seed, another mask
    other = ops.gat_layer(g, hd, Ad, heads, 0.2, apply_elu=True, pack_scores=True, dropout_p=P, dropout_seed=_seed(d, (7, 9)))
    assert not torch.equal(other, out)
    # no seed given: drawn from torch's generator on the device, reproducible under torch.manual_seed
    torch.manual_seed(3)
    a = ops.gat_layer(g, hd, Ad, heads, 0.2, dropout_p=P)
    b = ops.gat_layer(g, hd, Ad, heads, 0.2, dropout_p=P)
    torch.manual_seed(3)
    c = ops.gat_layer(g, hd, Ad, heads, 0.2, dropout_p=P)
    assert torch.equal(a, c) and not torch.equal(a, b)


def test_entry_points_refuse_p_outside_the_unit_interval(cuda_device):
    import ctypes

    from dgll_amd import _lib, ops

    _, g = _graph(cuda_device)
    n = g.n_rows
    h = torch.zeros(n, 8, device=cuda_device)
    s = torch.zeros(n, 1, device=cuda_device)
    out, rowsum, seed = torch.zeros_like(h), torch.zeros_like(s), _seed(cuda_device)
    d = _lib.GatDesc()
    d.pass_, d.dtype, d.apply_elu, d.rowptr, d.col, d.n_rows, d.n_cols = _lib.GAT_FORWARD, _lib.F32, 1, g.rowptr.data_ptr(), g.col.data_ptr(), n, n
    d.heads, d.fo, d.alpha, d.h, d.ld_h, d.out, d.ld_out = 1, 8, 0.2, h.data_ptr(), 8, out.data_ptr(), 8
    d.row_score = d.col_score = s.data_ptr()
    d.col_score_stride, d.rowsum, d.drop_seed = 1, rowsum.data_ptr(), seed.data_ptr()
    for bad in (1.0, -0.25, float("nan")):
        d.drop_p = bad
        code = _lib.lib.dgll_hip_gat_pass(None, ctypes.byref(d))
        assert code == -1 and "[0, 1)" in _lib.last_error()
    with pytest.raises(ValueError):
        ops.gat_aggregate(g, h, s, s, 1, 0.2, dropout_p=1.0)
    with pytest.raises(ValueError):
        ops.gat_aggregate(g, h, s, s, 1, 0.2, mode=1, dropout_p=0.5)


def _record_heads(monkeypatch):
    """Every call of gatconv._heads with its input, output and the seed it drew."""
    from dgll_amd import ops
    from dgll_amd.nn.Convolution import gatconv

    calls, seeds = [], []
    real_heads, real_seed = gatconv._heads, ops.dropout_seed

    def seed_spy(device):
        s = real_seed(device)
        seeds.append(s)
        return s

    def heads_spy(x, adj, Ws, a1s, a2s, alpha, concat, mode, dropout, training):
        out = real_heads(x, adj, Ws, a1s, a2s, alpha, concat, mode, dropout, training)
        calls.append((x.detach(), [w.detach() for w in Ws], [a.detach() for a in a1s], [a.detach() for a in a2s], alpha, concat, dropout,
                      out.detach(), seeds[-1]))
        return out

    monkeypatch.setattr(ops, "dropout_seed", seed_spy)
    monkeypatch.setattr(gatconv, "_heads", heads_spy)
    return calls


@pytest.mark.parametrize("dtype", DTYPES)
def test_spgat_training_matches_host_arithmetic_layer_by_layer(cuda_device, monkeypatch, dtype):
    """SpGAT(dropout=0.6).train(): each of its two attention layers, given the input it saw and the seed it drew, equals the host
    arithmetic of gatconv._host_heads with the mask of that seed in place of F.dropout."""
    from dgll_amd import nn as dnn

    d = cuda_device
    g_cpu, g = _graph(d)
    n = g.n_rows
    torch.manual_seed(0)
    model = dnn.SpGAT(50, 32, 47, dropout=0.6, alpha=0.2, nheads=8).to(d).to(dtype).train()
    x = torch.randn(n, 50, device=d).to(dtype)
    calls = _record_heads(monkeypatch)
    out = model(x, g)
    out.float().sum().backward()
    assert torch.isfinite(out).all() and all(torch.isfinite(p.grad).all() for p in model.parameters())
    assert len(calls) == 2
    row, col = g_cpu.row_index(), g_cpu.col.long()
    for xin, Ws, a1s, a2s, alpha, concat, p, got, seed in calls:
        heads = len(Ws)
        mask = _host_mask(g_cpu, heads, p, seed)
        outs = []
        for k, (W, a1, a2) in enumerate(zip(Ws, a1s, a2s)):
            h = (xin.float().cpu() @ W.float().cpu()).to(dtype).float()       # the transform stores h in the layer's dtype
            w = torch.exp(-torch.nn.functional.leaky_relu((h @ a1.float().cpu())[row] + (h @ a2.float().cpu())[col], alpha))
            den = torch.zeros(n).index_add_(0, row, w)
            hp = torch.zeros(n, h.shape[1]).index_add_(0, row, (w * mask[:, k]).unsqueeze(1) * h[col]) / den.unsqueeze(1)
            outs.append(torch.nn.functional.elu(hp) if concat else hp)
        want = torch.cat(outs, dim=1)
        assert got.shape == want.shape
        _close("SpGAT layer, %d head(s)" % heads, got, want, dtype, False)


def test_spgat_training_under_graph_capture_draws_a_fresh_mask_per_replay(cuda_device):
    from dgll_amd import nn as dnn

    d = cuda_device
    _, g = _graph(d, n=2000, seed=3)
    torch.manual_seed(0)
    model = dnn.SpGAT(50, 32, 47, dropout=0.0, alpha=0.2, nheads=8).to(d).to(torch.bfloat16).train()
    model.out_att.dropout.p = 0.6       # F.dropout on the activations is off: the output layer's attention dropout is all that is random
    x = torch.randn(g.n_rows, 50, device=d).to(torch.bfloat16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            model(x, g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        static_out = model(x, g)
    outs = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        outs.append(static_out.clone())
    assert all(torch.isfinite(o).all() for o in outs)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])


@pytest.mark.parametrize("inactive", ["eval", "p0"])
def test_inactive_dropout_is_bit_equal_to_the_mask_path(cuda_device, monkeypatch, inactive):
    """.eval(), or p = 0 in training: outputs and gradients are torch.equal to those under DGLL_GAT_DROPOUT=mask -- the same kernels
    run either way."""
    from dgll_amd import nn as dnn

    d = cuda_device
    _, g = _graph(d)
    torch.manual_seed(0)
    model = dnn.SpGAT(50, 32, 47, dropout=0.6 if inactive == "eval" else 0.0, alpha=0.2, nheads=8).to(d).to(torch.bfloat16)
    model.eval() if inactive == "eval" else model.train()
    x = torch.randn(g.n_rows, 50, device=d).to(torch.bfloat16)
    results = []
    for env in ("kernel", "mask"):
        monkeypatch.setenv("DGLL_GAT_DROPOUT", env)
        model.zero_grad(set_to_none=True)
        out = model(x, g)
        out.float().sum().backward()
        results.append([out.detach().clone()] + [p.grad.detach().clone() for p in model.parameters()])
    for a, b in zip(*results):
        assert torch.equal(a, b)


def _peak_of_step(model, x, g, labels):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    model.zero_grad(set_to_none=True)
    out = model(x, g)
    loss = torch.nn.functional.nll_loss(out, labels)
    loss.backward()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_training_step_with_dropout_needs_no_per_edge_array(cuda_device, monkeypatch):
    """nnz x heads x 4 >= 64 MB: the peak of a training step with p = 0.6 exceeds that of the same step with p = 0 by less than ONE
    [nnz, heads] fp32 array; with DGLL_GAT_DROPOUT=mask it does not stay under that bound (so the bound can fail)."""
    import dgll_amd
    from dgll_amd import nn as dnn

    d = cuda_device
    # 20 000 nodes of degree ~130 with self-loops: the per-NODE state that dropout legitimately adds to a step (F.dropout's outputs and
    # masks on the [n, 64] input and the [n, 256] hidden activations, 3 bytes per element: 19 MB) is small next to one per-EDGE array
    n = 20000
    gen = torch.Generator().manual_seed(1)
    row = torch.cat([torch.arange(n).repeat_interleave(130), torch.arange(n)])
    col = torch.cat([torch.randint(0, n, (n * 130,), generator=gen), torch.arange(n)])
    g = dgll_amd.CSRGraph.from_coo(row, col, None, (n, n)).to(d)
    heads = 8
    one_array = g.nnz * heads * 4
    assert one_array >= 64 * 2 ** 20, one_array
    torch.manual_seed(0)
    model = dnn.SpGAT(64, 32, 47, dropout=0.6, alpha=0.2, nheads=heads).to(d).to(torch.bfloat16).train()
    x = torch.randn(g.n_rows, 64, device=d).to(torch.bfloat16)
    labels = torch.randint(0, 47, (g.n_rows,), device=d)

    def peak(p, env):
        monkeypatch.setenv("DGLL_GAT_DROPOUT", env)
        model.dropout = p
        for att in list(model.attentions) + [model.out_att]:
            att.dropout.p = p
        _peak_of_step(model, x, g, labels)                  # warm-up: plans, transposes, caches
        return _peak_of_step(model, x, g, labels)

    p0 = peak(0.0, "kernel")
    in_kernel = peak(0.6, "kernel")
    masked = peak(0.6, "mask")
    print("peak of a step: p=0 %.1f MB, p=0.6 in-kernel %.1f MB, p=0.6 mask path %.1f MB; one [nnz, heads] array %.1f MB"
          % (p0 / 2 ** 20, in_kernel / 2 ** 20, masked / 2 ** 20, one_array / 2 ** 20))
    assert in_kernel - p0 < one_array, (in_kernel, p0, one_array)
    assert not (masked - p0 < one_array), (masked, p0, one_array)
