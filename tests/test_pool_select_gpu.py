"""segment_topk / select / sort_pool and the selection-pooling layers (csrc/seg_sort.hip) against plain restatements: the order bit for
bit against numpy's lexsort on the same fp32 values, the scaled gather and its backward against float64 torch on the CPU."""
import functools

import numpy as np
import pytest
import torch

from dgll_amd import _lib, ops_pool

pytestmark = pytest.mark.gpu

T = _lib.SEGSORT_TILE
# the first list crosses every path boundary in one launch (all of it then runs the long path's kernels); the others hold max_seg
# inside one instance each: the wave kernel, and the workgroup kernel with 1, 2, 4, 8 and 16 keys per lane
SEG_LISTS = {"all": [0, 1, 2, 63, 64, 65, 100, T - 1, T, T + 1, 2 * T + 3, 3 * T], "wave": [0, 1, 2, 63, 64], "kpl1": [65, 100, 256, 1],
             "kpl2": [257, 0, 512, 3], "kpl4": [513, 1000], "kpl8": [1025, T // 2, 64], "kpl16": [T // 2 + 1, T]}
RULES = {"half": dict(ratio=0.5), "all": dict(ratio=1.0), "k1": dict(k=1), "k70": dict(k=70)}
TOL = {torch.float32: 1e-4, torch.bfloat16: 3e-2}           # tests/test_pooling_gpu.py, scaled by the reference's largest magnitude


@functools.lru_cache(maxsize=None)
def scores(content, n):
    g = torch.Generator().manual_seed(n + len(content))
    if content == "ties":
        return torch.randint(-2, 3, (n,), generator=g).float()
    s = torch.randn(n, generator=g)
    if content == "special":
        where = torch.randint(0, n, (n // 3,), generator=g)
        s[where] = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), -float("nan")])[torch.arange(n // 3) % 6]
    return s


def ref_topk(s32, sizes, counts):
    """(idx, inv): per segment, score descending, ties to the smaller index, -0 == +0, NaNs last by index; cut to the counts"""
    s, idx, start = s32.astype(np.float64) + 0.0, [], 0
    for size, m in zip(sizes, counts):
        seg = s[start:start + size]
        nan = np.isnan(seg)
        idx.append(start + np.lexsort((np.arange(size), np.where(nan, 0.0, -seg), nan))[:m])
        start += size
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    inv = np.full(len(s32), -1, np.int32)
    inv[idx] = np.arange(len(idx), dtype=np.int32)
    return torch.from_numpy(idx.astype(np.int64)), torch.from_numpy(inv)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("content", ["normal", "ties", "special"])
@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("segs", sorted(SEG_LISTS))
def test_order_is_the_contract_bit_for_bit(segs, rule, content, dtype):
    sizes = SEG_LISTS[segs]
    score = scores(content, sum(sizes)).to(dtype)
    idx, inv = ops_pool.segment_topk(score.cuda(), sizes, return_inverse=True, **RULES[rule])
    want_idx, want_inv = ref_topk(score.float().numpy(), sizes, idx.seg_sizes)
    assert idx.seg_sizes == ops_pool.keep_counts(sizes, **RULES[rule]) and idx.dtype == torch.int64 and inv.dtype == torch.int32
    assert torch.equal(idx.cpu(), want_idx) and torch.equal(inv.cpu(), want_inv)


def test_batch_vector_gives_the_same_and_must_be_sorted():
    sizes = SEG_LISTS["all"]
    score = scores("ties", sum(sizes)).cuda()
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).cuda()
    a, a_inv = ops_pool.segment_topk(score, sizes, ratio=0.5, return_inverse=True)
    b, b_inv = ops_pool.segment_topk(score.view(-1, 1), batch=batch, ratio=0.5, return_inverse=True)
    assert torch.equal(a, b) and torch.equal(a_inv, b_inv) and a.seg_sizes == b.seg_sizes
    with pytest.raises(ValueError, match="non-decreasing"):
        ops_pool.segment_topk(score, batch=batch.flip(0), ratio=0.5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("F,wide", [(1, False), (7, False), (7, True), (8, False), (64, False), (200, False)])
@pytest.mark.parametrize("act", sorted(ops_pool.ACTS))
def test_select_forward_and_backward(act, F, wide, dtype):
    sizes, tol = [0, 1, 65, 300], TOL[dtype]
    n = sum(sizes)
    g = torch.Generator().manual_seed(F)
    buf = torch.randn(n, F + wide, generator=g).to(dtype).cuda()
    x = buf[:, :F].detach().requires_grad_(True)                   # wide: a row pitch of F + 1 = 8 elements, whole 16-byte vectors
    s = torch.randn(n, generator=g).to(dtype).cuda().requires_grad_(True)
    perm, inv = ops_pool.segment_topk(s, sizes, ratio=0.5, return_inverse=True)
    w = torch.randn(perm.numel(), F, generator=g)
    out = ops_pool.select(x, s, perm, inv, act=act)
    (out.float() * w.cuda()).sum().backward()

    xr, sr = x.detach().double().cpu().requires_grad_(True), s.detach().double().cpu().requires_grad_(True)
    mult = {"none": torch.ones_like, "identity": lambda v: v, "tanh": torch.tanh, "sigmoid": torch.sigmoid}[act](sr[perm.cpu()])
    ref = xr[perm.cpu()] * mult.unsqueeze(1)
    (ref * w).sum().backward()
    ref_gs = torch.zeros(n, dtype=torch.float64) if sr.grad is None else sr.grad
    for got, want in ((out, ref.detach()), (x.grad, xr.grad), (s.grad, ref_gs)):
        torch.testing.assert_close(got.double().cpu(), want, rtol=tol, atol=tol * float(want.abs().max()))
    # the backward writes every row itself: poisoned buffers come back with exact zeros outside perm
    gx, gs = torch.full((n, F), float("nan"), dtype=dtype).cuda(), torch.full((n,), float("nan")).cuda()
    gout = torch.zeros(perm.numel(), F + wide, dtype=dtype).cuda()[:, :F].copy_(w)
    ops_pool.select_bwd_raw(x.detach(), s.detach(), inv, gout, perm.numel(), ops_pool.ACTS[act], grad_x=gx, grad_score=gs)
    torch.testing.assert_close(gx.double().cpu(), xr.grad, rtol=tol, atol=tol * float(xr.grad.abs().max()))
    dropped = inv < 0
    assert dropped.sum() == n - perm.numel() and not gx.isnan().any() and not gs.isnan().any()
    assert (gx[dropped] == 0).all() and (gs[dropped] == 0).all() and (x.grad[dropped] == 0).all() and (s.grad[dropped] == 0).all()
    poisoned = torch.full((perm.numel(), F), float("nan"), dtype=dtype).cuda()
    assert torch.equal(ops_pool.select_raw(x.detach(), s.detach(), perm, ops_pool.ACTS[act], out=poisoned), out.detach())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sort_pool_orders_by_the_last_channel_and_pads_with_zeros(dtype):
    from dgll_amd.nn.GlobalPooling import SortPooling, global_sort_pool

    sizes, k, F, tol = [0, 3, 10, 40], 10, 5, TOL[dtype]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(sum(sizes), F, generator=g)
    x[:, -1] = torch.randint(0, 4, (sum(sizes),), generator=g).float()                      # ties in the sorting channel
    xd = x.to(dtype).cuda().requires_grad_(True)
    w = torch.randn(len(sizes), k * F, generator=g)
    out = SortPooling(k)(xd, sizes)
    (out.float() * w.cuda()).sum().backward()
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).cuda()
    assert torch.equal(global_sort_pool(xd.detach(), batch=batch, k=k), out.detach())

    xr = xd.detach().double().cpu().requires_grad_(True)
    idx, _ = ref_topk(xr.detach()[:, -1].numpy().astype(np.float32), sizes, [min(k, s) for s in sizes])
    rows, start = [], 0
    for s in sizes:                                                                          # a short graph: zero rows behind its own
        m = min(k, s)
        rows.append(torch.cat([xr[idx[start:start + m]], torch.zeros(k - m, F, dtype=torch.float64)]))
        start += m
    ref = torch.stack(rows).reshape(len(sizes), k * F)
    (ref * w).sum().backward()
    assert out.shape == ref.shape and (out[0] == 0).all() and (out[1, 3 * F:] == 0).all()
    torch.testing.assert_close(out.double().cpu(), ref.detach(), rtol=tol, atol=tol * float(ref.detach().abs().max()))
    torch.testing.assert_close(xd.grad.double().cpu(), xr.grad, rtol=tol, atol=tol * float(xr.grad.abs().max()))


@pytest.mark.parametrize("layer", ["topk", "sag"])
def test_layers_on_a_small_batched_graph(layer):
    from dgll_amd.graph import CSRGraph
    from dgll_amd.nn.GlobalPooling import SAGPooling, TopKPooling
    from dgll_amd.sampling.subgraph import node_subgraph

    sizes, F = [5, 0, 12], 16
    n, rng = sum(sizes), np.random.default_rng(7)
    adj = np.zeros((n, n), bool)
    adj[:5, :5] = rng.random((5, 5)) < 0.5
    adj[5:, 5:] = rng.random((12, 12)) < 0.3
    rowptr = np.concatenate([[0], np.cumsum(adj.sum(1))]).astype(np.int64)
    col = np.nonzero(adj)[1].astype(np.int32)
    graph = CSRGraph(torch.from_numpy(rowptr), torch.from_numpy(col), torch.ones(len(col)), n, n).to("cuda")
    torch.manual_seed(11)
    pool = (TopKPooling(F) if layer == "topk" else SAGPooling(F)).cuda()
    x = torch.randn(n, F).cuda().requires_grad_(True)
    x_out, graph_out, segs_out, perm, score_kept = pool(graph, x, sizes)
    score = pool.score(graph, x).detach().reshape(-1)
    want_perm, _ = ref_topk(score.float().cpu().numpy(), sizes, [3, 0, 6])
    assert segs_out == [3, 0, 6] and torch.equal(perm.cpu(), want_perm)
    want = x.detach()[perm] * torch.tanh(score[perm]).unsqueeze(1)
    torch.testing.assert_close(x_out.detach(), want, rtol=1e-4, atol=1e-4 * float(want.abs().max()))
    torch.testing.assert_close(score_kept.detach(), torch.tanh(score[perm]))
    sub = node_subgraph(graph, perm)
    assert torch.equal(graph_out.rowptr, sub.rowptr) and torch.equal(graph_out.col, sub.col) and graph_out.n_rows == 9
    x_out.sum().backward()
    param = pool.p if layer == "topk" else pool.gnn.weight
    assert param.grad is not None and bool(param.grad.abs().sum() > 0) and bool(x.grad.abs().sum() > 0)
