"""The message-passing family on the GPU: dgll_amd.ops_mp (edge_softmax, u_mul_e_sum, u_dot_v, u_add_v, copy_e_sum, each with its
gradients) and nn.AGNNConv against the float64 restatements of mp_ref.py / attn_ref.py (per-edge tensors, autograd).  For bf16 the
reference runs on the bf16-rounded inputs, so only accumulation order and the output rounding differ.

Bars (as test_sparse_attn_gpu.py states them).  Node matrices: fp32 forward max |err| <= 1e-4 max |ref|, fp32
gradients <= 2e-3 max |ref|; bf16 forward <= 2e-2 max |ref|, bf16 gradients relative L2 <= 1.5e-2.  Per-edge and per-row outputs are
fp32 whatever the node dtype: forwards meet the fp32 forward bar, backwards the fp32 gradient bar."""
import copy

import numpy as np
import pytest
import torch

import mp_ref
from attn_ref import sparse_attention_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
NEG = -float("inf")


@pytest.fixture(scope="module")
def rmat():
    from dgll_amd import synth

    g = synth.rmat_graph(10, 10, symmetric=True, self_loops=True).to(DEV)
    assert g.n_rows == 1024 and int(g.degrees().max()) > 300
    return g


@pytest.fixture(scope="module")
def edge_graph():
    """The 70 x 90 graph of test_sparse_attn_gpu.py, rebuilt: rows 0 empty, 1 one entry, 2 exactly 64, 3 65, 4 one column five times,
    5 LONG_ROW, 6 LONG_ROW + 1, 7 3000 entries (columns drawn with repetition), then short rows; the last row is empty and source 89
    is never referenced."""
    from dgll_amd import CSRGraph, ops_mp

    rng = np.random.RandomState(5)
    rows = [[], [17], list(rng.permutation(89)[:64]), list(rng.permutation(89)[:65]), [33] * 5,
            list(rng.randint(0, 89, ops_mp.LONG_ROW)), list(rng.randint(0, 89, ops_mp.LONG_ROW + 1)), list(rng.randint(0, 89, 3000))]
    rows += [list(rng.randint(0, 89, rng.randint(1, 12))) for _ in range(61)] + [[]]
    assert len(rows) == 70 and all(c < 89 for r in rows for c in r)
    rowptr = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
    col = torch.tensor([int(c) for r in rows for c in r], dtype=torch.int32)
    return CSRGraph(rowptr, col, None, 70, 90).to(DEV)


@pytest.fixture(params=["rmat", "edge"])
def graph(request, rmat, edge_graph):
    return rmat if request.param == "rmat" else edge_graph


def _check(label, name, got, want, kind):
    """kind: 'fwd32' / 'grad32' max |err| over max |ref| at 1e-4 / 2e-3; 'fwd16' the same at 2e-2; 'grad16' relative L2 at 1.5e-2."""
    a, b = got.detach().double(), want.detach().double().to(got.device)
    assert a.shape == b.shape, (label, name, a.shape, b.shape)
    assert bool(torch.isfinite(a).all()), "%s %s: not finite" % (label, name)
    err_max = ((a - b).abs().max() / b.abs().max()).item()
    err_l2 = ((a - b).norm() / b.norm()).item()
    bar, err = {"fwd32": (1e-4, err_max), "grad32": (2e-3, err_max), "fwd16": (2e-2, err_max), "grad16": (1.5e-2, err_l2)}[kind]
    print("%s %-6s max/max %.3e  rel-l2 %.3e  bar %.1e" % (label, name, err_max, err_l2, bar))
    assert err <= bar, (label, name, err, bar)


def _node_kinds(dtype):
    return ("fwd32", "grad32") if dtype == torch.float32 else ("fwd16", "grad16")


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


# the (heads, D, dtype) set of test_sparse_attn_gpu.CASES: idle lanes, idle heads, two column blocks, one head, 16 rows per wavefront
CASES = [(1, 8, torch.float32), (5, 8, torch.float32), (8, 8, torch.float32), (4, 64, torch.float32), (8, 128, torch.float32),
         (1, 48, torch.bfloat16), (3, 24, torch.bfloat16), (8, 32, torch.bfloat16), (8, 64, torch.bfloat16)]
EDGE_CASES = [(8, 32, torch.float32), (8, 32, torch.bfloat16)]
_ids = lambda v: str(v).replace("torch.", "")       # noqa: E731


def _node_ops(graph, heads, D, dtype, label, seed):
    """u_mul_e_sum and u_dot_v, forward and every gradient; returns the device results for the exact-zero checks."""
    from dgll_amd import ops_mp

    gen = torch.Generator().manual_seed(seed)
    F = heads * D
    x = _randn(gen, graph.n_cols, F).to(dtype).to(DEV).requires_grad_()
    y = _randn(gen, graph.n_rows, F).to(dtype).to(DEV).requires_grad_()
    w = _randn(gen, graph.nnz, heads).to(DEV).requires_grad_()
    g_out = _randn(gen, graph.n_rows, F).to(dtype).to(DEV)
    g_dot = _randn(gen, graph.nnz, heads).to(DEV)
    fwd, grad = _node_kinds(dtype)
    rp, col = graph.rowptr, graph.col
    x64, y64, w64 = (t.detach().double().requires_grad_() for t in (x, y, w))

    out = ops_mp.u_mul_e_sum(graph, x, w)           # heads from w
    assert out.dtype == dtype and out.shape == (graph.n_rows, F)
    gx, gw = torch.autograd.grad(out, (x, w), g_out)
    ref = mp_ref.u_mul_e_sum_reference(rp, col, x64.view(-1, heads, D), w64).reshape(-1, F)
    rx, rw = torch.autograd.grad(ref, (x64, w64), g_out.double())
    _check(label, "mul", out, ref, fwd)
    _check(label, "mul.gx", gx, rx, grad)
    _check(label, "mul.gw", gw, rw, "grad32")
    assert gw.dtype == torch.float32 and gx.dtype == dtype

    dot = ops_mp.u_dot_v(graph, x, y, heads)
    assert dot.dtype == torch.float32 and dot.shape == (graph.nnz, heads)
    dx, dy = torch.autograd.grad(dot, (x, y), g_dot)
    ref = mp_ref.u_dot_v_reference(rp, col, x64.view(-1, heads, D), y64.view(-1, heads, D))
    rx, ry = torch.autograd.grad(ref, (x64, y64), g_dot.double())
    _check(label, "dot", dot, ref, "fwd32")
    _check(label, "dot.gx", dx, rx, grad)
    _check(label, "dot.gy", dy, ry, grad)
    return out, gx, dx, dy


@pytest.mark.parametrize("heads,D,dtype", CASES, ids=_ids)
def test_node_matrix_ops_on_rmat(rmat, heads, D, dtype):
    _node_ops(rmat, heads, D, dtype, "rmat %dx%d" % (heads, D), heads * 1000 + D)


@pytest.mark.parametrize("heads,D,dtype", EDGE_CASES + [(3, 24, torch.bfloat16), (5, 8, torch.float32)], ids=_ids)
def test_node_matrix_ops_on_edge_case_rows(edge_graph, heads, D, dtype):
    out, gx, dx, dy = _node_ops(edge_graph, heads, D, dtype, "edge %dx%d" % (heads, D), 11)
    assert out[0].abs().max().item() == 0.0 and out[69].abs().max().item() == 0.0       # the empty rows
    assert dy[0].abs().max().item() == 0.0 and dy[69].abs().max().item() == 0.0
    assert gx[89].abs().max().item() == 0.0 and dx[89].abs().max().item() == 0.0        # the source no row references


def _logits(graph, heads, gen, scale=3.0):
    """fp32 [nnz, heads] on the device with -inf entries: a few in the longest row and in a short one, and (the 70 x 90 graph) the
    five-entry row -inf alone."""
    e = _randn(gen, graph.nnz, heads) * scale
    rp = graph.rowptr.tolist()
    deg = [rp[i + 1] - rp[i] for i in range(graph.n_rows)]
    longest = max(range(graph.n_rows), key=lambda i: deg[i])
    e[rp[longest] + 3, :] = NEG
    e[rp[longest] + 200, 0] = NEG
    short = next(i for i in range(8, graph.n_rows) if 2 <= deg[i] <= 11)
    e[rp[short], :] = NEG
    alone = None
    if graph.n_rows == 70:
        alone = slice(rp[4], rp[5])
        e[alone, :] = NEG
    return e.to(DEV), alone


@pytest.mark.parametrize("heads", [1, 3, 8, 17, 4, 12])
def test_per_edge_ops(graph, heads):
    """edge_softmax by destination and by source (with -inf entries), u_add_v, copy_e_sum: forward and every gradient.  Heads 1, 3
    and 17 = 8 + 8 + 1 go by scalars, 4, 8 and 12 = 8 + 4 by 16-byte vectors of four heads."""
    from dgll_amd import ops_mp

    label = "%dx%d h%d" % (graph.n_rows, graph.n_cols, heads)
    gen = torch.Generator().manual_seed(100 + heads)
    rp, col = graph.rowptr, graph.col
    e, alone = _logits(graph, heads, gen)
    g = _randn(gen, graph.nnz, heads).to(DEV)
    for by in ("dst", "src"):
        ed = e.clone().requires_grad_()
        sm = ops_mp.edge_softmax(graph, ed, norm_by=by)
        (gb,) = torch.autograd.grad(sm, ed, g)
        e64 = e.double().requires_grad_()
        ref = mp_ref.edge_softmax_reference(rp, col, graph.n_cols, e64, by)
        (rb,) = torch.autograd.grad(ref, e64, g.double())
        _check(label, "sm." + by, sm, ref, "fwd32")
        _check(label, "smb." + by, gb, rb, "grad32")
        assert sm[torch.isinf(e)].abs().max().item() == 0.0 and gb[torch.isinf(e)].abs().max().item() == 0.0
        if by == "dst" and alone is not None:
            assert sm[alone].abs().max().item() == 0.0 and gb[alone].abs().max().item() == 0.0      # -inf alone: zeros, never NaN
    flat = ops_mp.edge_softmax(graph, e[:, 0].contiguous())                                        # [nnz] in, [nnz] out
    assert flat.shape == (graph.nnz,) and torch.equal(flat, ops_mp.edge_softmax(graph, e[:, :1].contiguous())[:, 0])

    a = _randn(gen, graph.n_cols, heads).to(DEV).requires_grad_()
    b = _randn(gen, graph.n_rows, heads).to(DEV).requires_grad_()
    uav = ops_mp.u_add_v(graph, a, b)
    ga, gb = torch.autograd.grad(uav, (a, b), g)
    a64, b64 = a.detach().double().requires_grad_(), b.detach().double().requires_grad_()
    ref = mp_ref.u_add_v_reference(rp, col, a64, b64)
    ra, rb = torch.autograd.grad(ref, (a64, b64), g.double())
    _check(label, "uav", uav, ref, "fwd32")
    _check(label, "uav.ga", ga, ra, "grad32")
    _check(label, "uav.gb", gb, rb, "grad32")
    if graph.n_rows == 70:
        assert ga[89].abs().max().item() == 0.0 and gb[0].abs().max().item() == 0.0 and gb[69].abs().max().item() == 0.0

    w = _randn(gen, graph.nnz, heads).to(DEV).requires_grad_()
    for by, n in (("dst", graph.n_rows), ("src", graph.n_cols)):
        gs = _randn(gen, n, heads).to(DEV)
        s = ops_mp.copy_e_sum(graph, w, norm_by=by)
        (gw,) = torch.autograd.grad(s, w, gs)
        w64 = w.detach().double().requires_grad_()
        ref = mp_ref.copy_e_sum_reference(rp, col, graph.n_cols, w64, by)
        (rw,) = torch.autograd.grad(ref, w64, gs.double())
        _check(label, "ces." + by, s, ref, "fwd32")
        _check(label, "ces.gw." + by, gw, rw, "grad32")
        if graph.n_rows == 70:
            assert s[-1].abs().max().item() == 0.0          # the empty last row / the unreferenced source


def test_softmax_by_source_is_softmax_by_destination_of_the_transpose(graph):
    """norm_by="src" on A equals norm_by="dst" on A^T with the logits permuted into A^T's entry order, bit for bit."""
    from dgll_amd import ops_mp

    gen = torch.Generator().manual_seed(7)
    e, _ = _logits(graph, 3, gen)
    gt, perm = graph.transpose()
    by_src = ops_mp.edge_softmax(graph, e, norm_by="src")
    on_t = ops_mp.edge_softmax(gt, e[perm].contiguous(), norm_by="dst")
    assert torch.equal(by_src[perm], on_t)


def test_vector_and_scalar_forms_give_the_same_bits(graph):
    """Eight heads on 16-byte boundaries go four at a time; the same values one float off those boundaries go by scalars."""
    from dgll_amd import ops_mp

    heads = 8
    gen = torch.Generator().manual_seed(9)
    e, _ = _logits(graph, heads, gen)
    g = _randn(gen, graph.nnz, heads).to(DEV)
    a = _randn(gen, graph.n_cols, heads).to(DEV)
    b = _randn(gen, graph.n_rows, heads).to(DEV)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, device=DEV)
        out = buf[1:].view(t.shape)
        out.copy_(t)
        assert out.is_contiguous() and out.data_ptr() % 16 == 4
        return out

    for by_src in (False, True):
        alpha = ops_mp.edge_softmax_raw(graph, e, by_src)
        assert torch.equal(alpha, ops_mp.edge_softmax_raw(graph, shifted(e), by_src))
        assert torch.equal(ops_mp.edge_softmax_bwd_raw(graph, alpha, g, by_src), ops_mp.edge_softmax_bwd_raw(graph, shifted(alpha), g, by_src))
        assert torch.equal(ops_mp.e_sum_raw(graph, g, by_src), ops_mp.e_sum_raw(graph, shifted(g), by_src))
    assert torch.equal(ops_mp.u_add_v_raw(graph, a, b, heads), ops_mp.u_add_v_raw(graph, shifted(a), b, heads))


def test_softmax_of_large_logits(rmat):
    """max |e| between 100 and 300: a softmax without max subtraction overflows fp32 (exp(89) is its largest finite value)."""
    from dgll_amd import ops_mp

    gen = torch.Generator().manual_seed(21)
    e = _randn(gen, rmat.nnz, 4)
    e = (e * (250.0 / e.abs().max().item())).to(DEV)
    assert 100.0 <= e.abs().max().item() <= 300.0
    g = _randn(gen, rmat.nnz, 4).to(DEV)
    ed = e.clone().requires_grad_()
    sm = ops_mp.edge_softmax(rmat, ed)
    (gb,) = torch.autograd.grad(sm, ed, g)
    e64 = e.double().requires_grad_()
    ref = mp_ref.edge_softmax_reference(rmat.rowptr, rmat.col, rmat.n_cols, e64)
    (rb,) = torch.autograd.grad(ref, e64, g.double())
    _check("large logits", "sm", sm, ref, "fwd32")
    _check("large logits", "smb", gb, rb, "grad32")


# ---- the composition: attention written with the family alone -----------------------------------------------------------------------

def _attention_inputs(graph, heads, D, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    q = _randn(gen, graph.n_rows, heads * D).to(dtype).to(DEV)
    k = _randn(gen, graph.n_cols, heads * D).to(dtype).to(DEV)
    v = _randn(gen, graph.n_cols, heads * D).to(dtype).to(DEV)
    g = _randn(gen, graph.n_rows, heads * D).to(dtype).to(DEV)
    return q, k, v, g


def _composed(graph, q, k, v, g, heads, scale):
    """(out, dq, dk, dv) of u_mul_e_sum(v, edge_softmax(scale * u_dot_v(k, q)))"""
    from dgll_amd import ops_mp

    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    alpha = ops_mp.edge_softmax(graph, scale * ops_mp.u_dot_v(graph, k, q, heads))
    out = ops_mp.u_mul_e_sum(graph, v, alpha, heads)
    return (out.detach(),) + tuple(torch.autograd.grad(out, (q, k, v), g))


def _attention_reference(graph, q, k, v, g, heads, scale):
    D = q.shape[1] // heads
    q64, k64, v64 = (t.detach().double().requires_grad_() for t in (q, k, v))
    out, _ = sparse_attention_reference(graph.rowptr, graph.col, q64.view(-1, heads, D), k64.view(-1, heads, D), v64.view(-1, heads, D), scale)
    out = out.reshape(graph.n_rows, heads * D)
    return (out.detach(),) + tuple(torch.autograd.grad(out, (q64, k64, v64), g.double()))


@pytest.mark.parametrize("heads,D,dtype", [(4, 16, torch.float32), (5, 8, torch.float32), (8, 32, torch.bfloat16), (3, 24, torch.bfloat16)], ids=_ids)
def test_composed_attention_meets_the_bars_of_the_fused_op(graph, heads, D, dtype):
    """Both paths are measured against the float64 reference of attn_ref.py (the yardstick of test_sparse_attn_gpu.py), neither
    against the other."""
    q, k, v, g = _attention_inputs(graph, heads, D, dtype, heads * 1000 + D)
    scale = D ** -0.5
    got = _composed(graph, q, k, v, g, heads, scale)
    want = _attention_reference(graph, q, k, v, g, heads, scale)
    fwd, grad = _node_kinds(dtype)
    label = "composed %dx%d %dx%d" % (graph.n_rows, graph.n_cols, heads, D)
    for name, a, b in zip(("out", "dq", "dk", "dv"), got, want):
        _check(label, name, a, b, fwd if name == "out" else grad)
    if graph.n_rows == 70:
        assert got[0][0].abs().max().item() == 0.0 and got[0][69].abs().max().item() == 0.0 and got[1][0].abs().max().item() == 0.0
        assert got[2][89].abs().max().item() == 0.0 and got[3][89].abs().max().item() == 0.0


def test_gradients_are_skipped_where_not_needed(rmat):
    """Only v needs a gradient: the result is that of the full backward, bit for bit, and only u_mul_e_sum's transposed pass runs."""
    from dgll_amd import ops, ops_mp

    heads, D = 8, 32
    q, k, v, g = _attention_inputs(rmat, heads, D, torch.bfloat16, 61)
    full = _composed(rmat, q, k, v, g, heads, D ** -0.5)
    vs = v.clone().requires_grad_()
    with ops.LaunchTimer() as timer:
        out = ops_mp.u_mul_e_sum(rmat, vs, ops_mp.edge_softmax(rmat, (D ** -0.5) * ops_mp.u_dot_v(rmat, k, q, heads)), heads)
        (gv,) = torch.autograd.grad(out, (vs,), g)
    assert torch.equal(out.detach(), full[0]) and torch.equal(gv, full[3])
    counts = {}
    for tag, (n, _) in timer.summary().items():
        counts[tag[0]] = counts.get(tag[0], 0) + n
    assert counts == {"mp_u_dot_v": 1, "mp_edge_softmax": 1, "mp_u_mul_e_sum": 2}, counts


def _everything(graph, heads, D, dtype, seed):
    """forward and all gradients of the composition, and of u_add_v and copy_e_sum"""
    from dgll_amd import ops_mp

    q, k, v, g = _attention_inputs(graph, heads, D, dtype, seed)
    res = list(_composed(graph, q, k, v, g, heads, D ** -0.5))
    gen = torch.Generator().manual_seed(seed)
    a = _randn(gen, graph.n_cols, heads).to(DEV).requires_grad_()
    b = _randn(gen, graph.n_rows, heads).to(DEV).requires_grad_()
    ge = _randn(gen, graph.nnz, heads).to(DEV)
    gs = _randn(gen, graph.n_cols, heads).to(DEV)
    uav = ops_mp.u_add_v(graph, a, b)
    res += [uav.detach()] + list(torch.autograd.grad(uav, (a, b), ge))
    w = ge.clone().requires_grad_()
    s = ops_mp.copy_e_sum(graph, w, norm_by="src")
    res += [s.detach()] + list(torch.autograd.grad(s, (w,), gs))
    return res


def test_reruns_are_bit_identical(graph):
    first = _everything(graph, 8, 32, torch.bfloat16, 41)
    again = _everything(graph, 8, 32, torch.bfloat16, 41)
    for i, (x, y) in enumerate(zip(first, again)):
        assert torch.equal(x, y), i


def test_forward_backward_can_be_captured(rmat):
    """The shape of test_sparse_attn_gpu.py::test_forward_backward_can_be_captured; the inputs change between the replays."""
    from dgll_amd import ops_mp

    heads, D = 8, 32
    q, k, v, g = _attention_inputs(rmat, heads, D, torch.bfloat16, 81)
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    rmat.transpose()                                # the cached structure: built outside the capture

    def step():
        alpha = ops_mp.edge_softmax(rmat, (D ** -0.5) * ops_mp.u_dot_v(rmat, k, q, heads))
        out = ops_mp.u_mul_e_sum(rmat, v, alpha, heads)
        return (out.detach(), alpha.detach()) + tuple(torch.autograd.grad(out, (q, k, v), g))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured, stream=side):
        static = step()
    for seed in (82, 83):
        fresh = _attention_inputs(rmat, heads, D, torch.bfloat16, seed)
        with torch.no_grad():
            for t, new in zip((q, k, v, g), fresh):
                t.copy_(new)
        eager = [t.clone() for t in step()]
        for t in static:
            t.zero_()
        captured.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("out", "alpha", "dq", "dk", "dv"), static, eager):
            assert torch.equal(a, b), name


def test_nothing_to_gather(rmat):
    """nnz == 0 or no rows: zeros, with zero gradients, and no launch."""
    from dgll_amd import CSRGraph, ops, ops_mp

    empty = CSRGraph(torch.zeros(6, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None, 5, 7).to(DEV)
    none = CSRGraph(torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None, 0, 7).to(DEV)
    x = torch.randn(7, 16, device=DEV, requires_grad=True)
    y = torch.randn(5, 16, device=DEV, requires_grad=True)
    w = torch.zeros(0, 2, device=DEV, requires_grad=True)
    a = torch.randn(7, 2, device=DEV, requires_grad=True)
    b = torch.randn(5, 2, device=DEV, requires_grad=True)
    with ops.LaunchTimer() as timer:
        out = ops_mp.u_mul_e_sum(empty, x, w)
        assert out.shape == (5, 16) and out.abs().max().item() == 0.0
        gx, gw = torch.autograd.grad(out.sum(), (x, w))
        assert gx.abs().max().item() == 0.0 and gw.shape == (0, 2)
        dot = ops_mp.u_dot_v(empty, x, y, 2)
        assert dot.shape == (0, 2) and all(t.abs().max().item() == 0.0 for t in torch.autograd.grad(dot.sum(), (x, y)))
        assert ops_mp.edge_softmax(empty, w).shape == (0, 2)
        uav = ops_mp.u_add_v(empty, a, b)
        assert uav.shape == (0, 2) and all(t.abs().max().item() == 0.0 for t in torch.autograd.grad(uav.sum(), (a, b)))
        s = ops_mp.copy_e_sum(empty, w)
        assert s.shape == (5, 2) and s.abs().max().item() == 0.0 and ops_mp.copy_e_sum(empty, w, norm_by="src").shape == (7, 2)
        assert ops_mp.u_mul_e_sum(none, x, w).shape == (0, 16) and ops_mp.u_dot_v(none, x, y[:0], 2).shape == (0, 2)
    assert timer.summary() == {}
    # strided and unaligned views are copied once: the same result as their contiguous copies
    wide = torch.randn(1024, 20, device=DEV)
    wr = torch.randn(rmat.nnz, 3, device=DEV)
    assert torch.equal(ops_mp.u_mul_e_sum(rmat, wide[:, 1:17], wr[:, :2]), ops_mp.u_mul_e_sum(rmat, wide[:, 1:17].contiguous(), wr[:, :2].contiguous()))


# ---- AGNNConv -----------------------------------------------------------------------------------------------------------------------

def _agnn_reference(graph, h_src, h_dst, beta):
    norm = lambda h: torch.nn.functional.normalize(h, p=2, dim=-1)      # noqa: E731
    rp, col = graph.rowptr.cpu(), graph.col.cpu()
    e = beta * mp_ref.u_dot_v_reference(rp, col, norm(h_src).unsqueeze(1), norm(h_dst).unsqueeze(1))
    p = mp_ref.edge_softmax_reference(rp, col, graph.n_cols, e)
    return mp_ref.u_mul_e_sum_reference(rp, col, h_src.unsqueeze(1), p).squeeze(1)


def _agnn_against_host(graph, h_src, n_dst, pair, dtype, label):
    """The device layer against its own host path AND the mp_ref restatement, both in float64 on the (rounded) device inputs:
    output, input gradient and beta.grad."""
    from dgll_amd.nn.Convolution import AGNNConv

    layer = AGNNConv(init_beta=1.5)
    host = copy.deepcopy(layer).double()
    layer = layer.to(DEV)
    leaf = h_src.to(dtype).to(DEV).requires_grad_()
    leaf_h = leaf.detach().double().cpu().requires_grad_()
    out = layer(graph, (leaf, leaf[:n_dst]) if pair else leaf)
    out_h = host(graph.to("cpu"), (leaf_h, leaf_h[:n_dst]) if pair else leaf_h)
    ref = _agnn_reference(graph, leaf_h, leaf_h[:n_dst], host.beta)
    assert out.dtype == dtype and out.shape == out_h.shape == (n_dst, h_src.shape[1])
    assert (out_h - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    gen = torch.Generator().manual_seed(7)
    g = _randn(gen, *out.shape)
    gx, gbeta = torch.autograd.grad(out, (leaf, layer.beta), g.to(dtype).to(DEV))
    rx, rbeta = torch.autograd.grad(out_h, (leaf_h, host.beta), g.to(dtype).double())
    fwd, grad = _node_kinds(dtype)
    _check(label, "out", out, out_h, fwd)
    _check(label, "gx", gx, rx, grad)
    _check(label, "gbeta", gbeta, rbeta, grad)
    assert gbeta.dtype == torch.float32 and gbeta.shape == (1,)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_agnnconv_matches_its_host_path(rmat, dtype):
    torch.manual_seed(61)
    _agnn_against_host(rmat, torch.randn(1024, 20), 1024, False, dtype, "agnn rmat")        # 20 columns: padded to whole vectors


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_agnnconv_on_a_sampled_block(rmat, dtype):
    from dgll_amd.nn.Convolution import AGNNConv
    from dgll_amd.sampling.neighbor import NeighborSampler

    torch.manual_seed(71)
    sampler = NeighborSampler([6], rmat)
    input_nodes, _, blocks = sampler.sample_seeded(None, torch.arange(0, 200, device=DEV), 71)
    block = blocks[0]
    assert block.n_rows == 200 and block.n_cols > block.n_rows
    h_src = torch.randn(1024, 20)[input_nodes.cpu()]
    _agnn_against_host(block, h_src, 200, True, dtype, "agnn block")
    with torch.no_grad():                           # one tensor on a block: its first rows are the destinations
        layer, h = AGNNConv().to(DEV), h_src.to(dtype).to(DEV)
        assert torch.equal(layer(block, h), layer(block, (h, h[:200])))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_agnn_trains_on_planted_communities(dtype):
    """40 Adam steps of the AGNN model on the planted communities of test_sparse_attn_gpu.py::test_training_on_planted_communities,
    at that test's threshold (the final loss below half the first, accuracy >= 0.9), which it set for its own attention layer on this
    graph.  On the host path in fp32 this seed and learning rate take the loss from 1.41 to below 0.01 at accuracy 0.9975."""
    from dgll_amd import synth
    from dgll_amd.nn.Convolution import AGNN

    n, k = 400, 4
    gen = torch.Generator().manual_seed(3)
    labels = torch.arange(n) % k
    prob = torch.where(labels[:, None] == labels[None, :], torch.tensor(0.05), torch.tensor(0.005))
    src, dst = (torch.rand(n, n, generator=gen) < prob).nonzero(as_tuple=True)
    graph = synth.build_graph(src, dst, n, symmetric=True, self_loops=True, weighted=False).to(DEV)
    x = (torch.nn.functional.one_hot(labels, k).float().repeat(1, 4) + torch.randn(n, 4 * k, generator=gen)).to(dtype).to(DEV)
    labels = labels.to(DEV)
    torch.manual_seed(3)
    model = AGNN(4 * k, 16, k).to(DEV)
    beta0 = model.layers[1].beta.item()
    opt = torch.optim.Adam(model.parameters(), lr=0.02)
    losses = []
    for _ in range(40):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(graph, x).float(), labels)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    acc = (model(graph, x).argmax(1) == labels).float().mean().item()
    print("loss %.4f -> %.4f, accuracy %.3f, beta %.3f -> %.3f" % (losses[0], losses[-1], acc, beta0, model.layers[1].beta.item()))
    assert losses[-1] < 0.5 * losses[0] and acc >= 0.9
    assert model.layers[1].beta.item() != beta0 and model.layers[0].beta.item() == 1.0      # the learnable scale learns, the buffer stays
