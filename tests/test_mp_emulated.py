"""csrc/mp_ops.hip without a GPU: the kernel source and csrc/row_tiles.hpp, both UNMODIFIED, compiled with g++ against the host
stand-ins of tests/kernel_emu/ and run in lock step (tests/kernel_emu.py; test_sparse_attn_emulated.py says what that checks and
what it cannot) against the float64 restatements of mp_ref.py.  All six passes run over A, and over A^T with perm where a backward
of dgll_amd/ops_mp.py uses them so.

Bars: per-edge outputs are fp32 whatever the node dtype -- forward max |err| <= 1e-4 max |ref|, the softmax
backward <= 2e-3 max |ref|; node matrices fp32 forward 1e-4 / gradient 2e-3 of max |ref|, bf16 forward 2e-2 of max |ref| / gradient
relative L2 1.5e-2, the reference computed on the bf16-rounded inputs."""
import os
import subprocess

import numpy as np
import pytest
import torch

import mp_ref
from kernel_emu import build_emulator

NEG = -float("inf")


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return build_emulator(tmp_path_factory, "mp_ops.hip", "mp_ops_main.cpp")


def _graph(full):
    """The two graphs of test_sparse_attn_emulated.py (same seed, same rows).  full -- 24 x 30: an empty row, one entry, 64, 65, one
    column five times, LONG_ROW, LONG_ROW + 1 and 400 entries, short rows, an empty last row; the last source is never referenced.
    Not full -- 9 x 12: empty, one entry, LONG_ROW + 1, short rows, empty."""
    from dgll_amd import CSRGraph, ops_mp

    rng = np.random.RandomState(9)
    n_src = 30 if full else 12
    draw = lambda k: list(rng.randint(0, n_src - 1, k))         # noqa: E731
    if full:
        rows = [[], [7], draw(64), draw(65), [11] * 5, draw(ops_mp.LONG_ROW), draw(ops_mp.LONG_ROW + 1), draw(400)]
        rows += [draw(rng.randint(1, 9)) for _ in range(15)] + [[]]
    else:
        rows = [[], [7], draw(ops_mp.LONG_ROW + 1)] + [draw(rng.randint(1, 9)) for _ in range(5)] + [[]]
    rowptr = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
    return CSRGraph(rowptr, torch.tensor([int(c) for r in rows for c in r], dtype=torch.int32), None, len(rows), n_src)


def _dump(t, path):
    (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).contiguous().numpy().tofile(path)


def _read(path, dtype, shape):
    if dtype == torch.bfloat16:
        return torch.from_numpy(np.fromfile(path, dtype=np.int16)).view(torch.bfloat16).reshape(shape)
    return torch.from_numpy(np.fromfile(path, dtype=np.float32)).reshape(shape)


def _logits(graph, heads, gen):
    """fp32 [nnz, heads] with -inf entries: a few in a short and in the longest row, and one short row (full: the five-entry row; else
    the one-entry row) that is -inf alone."""
    e = torch.randn(graph.nnz, heads, generator=gen) * 3.0
    rp = graph.rowptr.tolist()
    deg = [rp[i + 1] - rp[i] for i in range(graph.n_rows)]
    longest = max(range(graph.n_rows), key=lambda i: deg[i])
    e[rp[longest] + 3, :] = NEG
    e[rp[longest] + 200, 0] = NEG
    short = next(i for i in range(graph.n_rows) if 2 <= deg[i] <= 9 and i > 4)
    e[rp[short], :] = NEG
    alone = 4 if graph.n_rows == 24 else 1
    e[rp[alone]:rp[alone + 1], :] = NEG
    return e, alone


def _err(name, got, want, kind):
    """kind: 'fwd32' / 'grad32' max |err| over max |ref| at 1e-4 / 2e-3; 'fwd16' the same at 2e-2; 'grad16' relative L2 at 1.5e-2."""
    a, b = got.double(), want.double()
    assert bool(torch.isfinite(a).all()), name
    err_max = ((a - b).abs().max() / b.abs().max()).item()
    err_l2 = ((a - b).norm() / b.norm()).item()
    bar, err = {"fwd32": (1e-4, err_max), "grad32": (2e-3, err_max), "fwd16": (2e-2, err_max), "grad16": (1.5e-2, err_l2)}[kind]
    print("%-6s max/max %.3e  rel-l2 %.3e  bar %.1e" % (name, err_max, err_l2, bar))
    assert err <= bar, (name, err, bar)


def _run(emulator, tmp_path, graph, heads, D, dtype):
    gen = torch.Generator().manual_seed(heads * 100 + D)
    d, F = str(tmp_path), heads * D
    gt, perm = graph.transpose()
    e, alone = _logits(graph, heads, gen)
    w = torch.randn(graph.nnz, heads, generator=gen)
    g = torch.randn(graph.nnz, heads, generator=gen)
    a = torch.randn(graph.n_cols, heads, generator=gen)
    b = torch.randn(graph.n_rows, heads, generator=gen)
    files = [("rowptr", graph.rowptr), ("col", graph.col), ("trowptr", gt.rowptr), ("tcol", gt.col), ("perm", perm), ("e", e), ("w", w), ("g", g),
             ("a", a), ("b", b)]
    if D:
        x = torch.randn(graph.n_cols, F, generator=gen).to(dtype)
        y = torch.randn(graph.n_rows, F, generator=gen).to(dtype)
        gy = torch.randn(graph.n_rows, F, generator=gen).to(dtype)
        files += [("x", x), ("y", y), ("gy", gy)]
    for name, t in files:
        _dump(t, os.path.join(d, name + ".bin"))
    res = subprocess.run([emulator, d, str(graph.n_rows), str(graph.n_cols), str(heads), str(D), "0" if dtype == torch.float32 else "1"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "emu ok" in res.stdout, res.stdout + res.stderr
    edge = lambda n: _read(os.path.join(d, n + ".bin"), torch.float32, (graph.nnz, heads))      # noqa: E731
    rp, col = graph.rowptr, graph.col
    rowA = mp_ref.rows_of(rp)

    for by, fwd, bwd in (("dst", "sm", "smb"), ("src", "smt", "smtb")):
        e64 = e.double().requires_grad_()
        want = mp_ref.edge_softmax_reference(rp, col, graph.n_cols, e64, by)
        (want_b,) = torch.autograd.grad(want, e64, g.double())
        got = edge(fwd)
        _err(fwd, got, want.detach(), "fwd32")
        _err(bwd, edge(bwd), want_b, "grad32")
        assert got[torch.isinf(e)].abs().max().item() == 0.0                       # an entry of -inf: exactly 0
    assert edge("sm")[rp[alone]:rp[alone + 1]].abs().max().item() == 0.0           # the row of -inf alone: zeros, not NaN
    seg = mp_ref.rows_of(rp)
    sums = torch.zeros(graph.n_rows, heads).index_add_(0, seg, edge("sm"))
    live = torch.zeros(graph.n_rows, heads).index_add_(0, seg, (~torch.isinf(e)).float()) > 0
    assert (sums[live] - 1.0).abs().max().item() <= 1e-5 and sums[~live].abs().max().item() == 0.0

    es = _read(os.path.join(d, "es.bin"), torch.float32, (graph.n_rows, heads))
    est = _read(os.path.join(d, "est.bin"), torch.float32, (graph.n_cols, heads))
    _err("es", es, mp_ref.copy_e_sum_reference(rp, col, graph.n_cols, w.double(), "dst"), "fwd32")
    _err("est", est, mp_ref.copy_e_sum_reference(rp, col, graph.n_cols, w.double(), "src"), "fwd32")
    assert es[0].abs().max().item() == 0.0 and es[-1].abs().max().item() == 0.0 and est[-1].abs().max().item() == 0.0
    _err("uav", edge("uav"), mp_ref.u_add_v_reference(rp, col, a.double(), b.double()), "fwd32")
    assert torch.equal(edge("uavt"), a[col.long()])                                # the row side alone over A^T: a copy, bit for bit
    if not D:
        return
    half = dtype == torch.bfloat16
    x64 = x.double().view(-1, heads, D).requires_grad_()
    out = mp_ref.u_mul_e_sum_reference(rp, col, x64, w.double())
    (want_t,) = torch.autograd.grad(out, x64, gy.double().view(-1, heads, D))
    mul = _read(os.path.join(d, "mul.bin"), dtype, (graph.n_rows, F))
    mult = _read(os.path.join(d, "mult.bin"), dtype, (graph.n_cols, F))
    _err("mul", mul, out.detach().reshape(-1, F), "fwd16" if half else "fwd32")
    _err("mult", mult, want_t.reshape(-1, F), "grad16" if half else "grad32")
    assert mul[0].abs().max().item() == 0.0 and mul[-1].abs().max().item() == 0.0  # the empty rows
    assert mult[-1].abs().max().item() == 0.0                                      # the unreferenced source
    _err("dot", edge("dot"), mp_ref.u_dot_v_reference(rp, col, x.double().view(-1, heads, D), y.double().view(-1, heads, D)), "fwd32")
    assert rowA.numel() == graph.nnz


# the node-matrix geometries of test_sparse_attn_emulated.py (lanes per head / per row, idle lanes and heads, two column blocks)
@pytest.mark.parametrize("heads,D,dtype", [(8, 16, torch.float32), (3, 24, torch.bfloat16), (5, 8, torch.float32), (3, 128, torch.float32),
                                           (1, 48, torch.bfloat16)], ids=lambda v: str(v).replace("torch.", ""))
def test_all_passes_in_lock_step(emulator, tmp_path, heads, D, dtype):
    _run(emulator, tmp_path, _graph(full=D < 128), heads, D, dtype)


# the per-edge passes alone: register blocks of 1, 4 (one head masked), 8 and 8 + 8 + 1 heads by scalars; 4, 8 and 8 + 4 heads (half of
# the second block masked) by 16-byte vectors of four heads
@pytest.mark.parametrize("heads", [1, 3, 8, 17, 4, 12])
def test_per_edge_passes_in_lock_step(emulator, tmp_path, heads):
    _run(emulator, tmp_path, _graph(full=True), heads, 0, torch.float32)
