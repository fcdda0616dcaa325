"""csrc/multi_agg.hip without a GPU: the kernel source and csrc/row_tiles.hpp, both UNMODIFIED, compiled with g++ against the host
stand-ins of tests/kernel_emu/ and run in lock step (tests/kernel_emu.py; test_sparse_attn_emulated.py says what that checks and what
it cannot) against the float64 per-edge restatement of pna_ref.py.  All three passes, all six aggregators and three scalers, with and
without the per-row addend y.

Bars, applied PER aggregator x scaler block against that block's own max |ref| (a wrong std must not hide behind a
large sum; the backward is linear in the output gradient, so the emulator runs it once per block with the others zeroed): fp32
forward max |err| <= 1e-4 max |ref|, gradients <= 2e-3 max |ref|; bf16 forward <= 2e-2 max |ref|, gradients relative L2 <= 1.5e-2, the
reference computed on the bf16-rounded inputs."""
import os
import subprocess

import numpy as np
import pytest
import torch

import pna_ref
from kernel_emu import build_emulator

AGGS, SCALERS, DELTA = pna_ref.AGGREGATORS, pna_ref.SCALERS, 1.7
ONE, FIVE = 1, 4        # rows of the full graph: one entry; one column five times


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return build_emulator(tmp_path_factory, "multi_agg.hip", "multi_agg_main.cpp")


def _graph(full):
    """The two graphs of test_mp_emulated.py (same seed, same rows).  full -- 24 x 30: an empty row, one entry, 64, 65, one column five
    times, LONG_ROW, LONG_ROW + 1 and 400 entries, short rows, an empty last row; the last source is never referenced.  Not full --
    9 x 12: empty, one entry, LONG_ROW + 1, short rows, empty."""
    from dgll_amd import CSRGraph, ops_agg

    rng = np.random.RandomState(9)
    n_src = 30 if full else 12
    draw = lambda k: list(rng.randint(0, n_src - 1, k))         # noqa: E731
    if full:
        rows = [[], [7], draw(64), draw(65), [11] * 5, draw(ops_agg.LONG_ROW), draw(ops_agg.LONG_ROW + 1), draw(400)]
        rows += [draw(rng.randint(1, 9)) for _ in range(15)] + [[]]
    else:
        rows = [[], [7], draw(ops_agg.LONG_ROW + 1)] + [draw(rng.randint(1, 9)) for _ in range(5)] + [[]]
    rowptr = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
    return CSRGraph(rowptr, torch.tensor([int(c) for r in rows for c in r], dtype=torch.int32), None, len(rows), n_src)


def _dump(t, path):
    (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).contiguous().numpy().tofile(path)


def _read(path, dtype, shape):
    if dtype == torch.bfloat16:
        return torch.from_numpy(np.fromfile(path, dtype=np.int16)).view(torch.bfloat16).reshape(shape)
    return torch.from_numpy(np.fromfile(path, dtype={torch.float32: np.float32, torch.int32: np.int32}[dtype])).reshape(shape)


def _err(name, got, want, kind):
    """kind: 'fwd32' / 'grad32' max |err| over max |ref| at 1e-4 / 2e-3; 'fwd16' the same at 2e-2; 'grad16' relative L2 at 1.5e-2.  A
    reference that is zero but for its own float64 rounding residue (the gradient of var / std with respect to y: below 1e-10 with inputs
    and gradients of order 1) must be met with exact zeros."""
    a, b = got.double(), want.double()
    assert bool(torch.isfinite(a).all()), name
    if b.abs().max().item() < 1e-10:
        assert a.abs().max().item() == 0.0, name
        return
    err_max = ((a - b).abs().max() / b.abs().max()).item()
    err_l2 = ((a - b).norm() / b.norm()).item()
    bar, err = {"fwd32": (1e-4, err_max), "grad32": (2e-3, err_max), "fwd16": (2e-2, err_max), "grad16": (1.5e-2, err_l2)}[kind]
    print("%-12s max/max %.3e  rel-l2 %.3e  bar %.1e" % (name, err_max, err_l2, bar))
    assert err <= bar, (name, err, bar)


def _run(emulator, tmp_path, graph, F, dtype, with_y):
    d, half = str(tmp_path), dtype == torch.bfloat16
    n_dst, n_src, blocks = graph.n_rows, graph.n_cols, len(AGGS) * len(SCALERS)
    gen = torch.Generator().manual_seed(F + 7)
    gt, _ = graph.transpose()
    x64 = pna_ref.spread_features(n_src, F, seed=F)
    x = x64.to(dtype)
    y = torch.randn(n_dst, F, generator=gen).to(dtype)
    go = torch.randn(n_dst, blocks * F, generator=gen).to(dtype)
    for name, t in (("rowptr", graph.rowptr), ("col", graph.col), ("trowptr", gt.rowptr), ("tcol", gt.col), ("x", x), ("y", y), ("go", go)):
        _dump(t, os.path.join(d, name + ".bin"))
    res = subprocess.run([emulator, d, str(n_dst), str(n_src), str(F), "1" if half else "0", "1" if with_y else "0",
                          "".join(str(pna_ref.AGGREGATORS.index(a)) for a in AGGS), "".join(str(pna_ref.SCALERS.index(s)) for s in SCALERS),
                          repr(DELTA)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "emu ok" in res.stdout, res.stdout + res.stderr
    read = lambda n, dt, shape: _read(os.path.join(d, n + ".bin"), dt, shape)      # noqa: E731

    # the generator keeps distinct values apart: the smallest non-zero row variance is at least (2 / n_src)^2 (float64, before rounding)
    parts = {}
    pna_ref.multi_aggregate_reference(graph.rowptr, graph.col, x64, None, AGGS, SCALERS, DELTA, parts)
    floor = (2.0 / n_src) ** 2
    assert parts["var"][parts["var"] > 0].min().item() >= floor
    xr = x.double().requires_grad_()
    yr = y.double().requires_grad_() if with_y else None
    parts = {}
    want = pna_ref.multi_aggregate_reference(graph.rowptr, graph.col, xr, yr, AGGS, SCALERS, DELTA, parts)
    if not half:
        assert parts["var"][parts["var"] > 0].min().item() >= floor * (1 - 1e-5)

    out = read("out", dtype, (n_dst, blocks * F))
    stats = read("stats", torch.float32, (n_dst, 2 * F))
    arg = read("arg", torch.int32, (n_dst, 2 * F))
    coef = read("coef", torch.float32, (n_dst, 5 * F))
    for k in range(blocks):
        name = "%s*%s" % (SCALERS[k // len(AGGS)][:3], AGGS[k % len(AGGS)])
        sl = slice(k * F, (k + 1) * F)
        _err(name, out[:, sl], want.detach()[:, sl], "fwd16" if half else "fwd32")
        mask = torch.zeros_like(go, dtype=torch.float64)
        mask[:, sl] = go.double()[:, sl]
        grads = torch.autograd.grad(want, (xr, yr) if with_y else (xr,), mask, retain_graph=True)
        _err("gx " + name, read("gx_%d" % k, dtype, (n_src, F)), grads[0], "grad16" if half else "grad32")
        if with_y:
            _err("gy " + name, read("gy_%d" % k, dtype, (n_dst, F)), grads[1], "grad16" if half else "grad32")
    grads = torch.autograd.grad(want, (xr, yr) if with_y else (xr,), go.double())
    gx = read("gx", dtype, (n_src, F))
    _err("gx", gx, grads[0], "grad16" if half else "grad32")
    of_x = {}                       # stats are those of x alone, without y
    pna_ref.multi_aggregate_reference(graph.rowptr, graph.col, x.double(), None, AGGS, SCALERS, DELTA, of_x)
    _err("stats", stats, torch.cat([of_x["mean"], of_x["var"]], 1), "fwd32")

    # the tie rule: arg is the reference's, whatever the dtype (the reference sees the rounded inputs)
    assert torch.equal(arg.long(), torch.cat([parts["argmax"], parts["argmin"]], 1))
    if not half and not with_y:     # the max / min blocks under the identity scaler: bit for bit an entry of x
        i_max, i_min = AGGS.index("max"), AGGS.index("min")
        assert torch.equal(out[:, i_max * F:(i_max + 1) * F], want.detach()[:, i_max * F:(i_max + 1) * F].float())
        assert torch.equal(out[:, i_min * F:(i_min + 1) * F], want.detach()[:, i_min * F:(i_min + 1) * F].float())
    # rows of equal entries (one entry; one column five times): var exactly 0, std exactly sqrt(1e-30), a variance coefficient of exactly 0
    tiny = torch.sqrt(torch.tensor(1e-30, dtype=torch.float32)).to(dtype)
    i_var, i_std = AGGS.index("var"), AGGS.index("std")
    for r in (ONE, FIVE) if n_dst == 24 else (ONE,):
        assert stats[r, F:].abs().max().item() == 0.0
        assert out[r, i_var * F:(i_var + 1) * F].abs().max().item() == 0.0
        assert torch.equal(out[r, i_std * F:(i_std + 1) * F], tiny.expand(F))
        assert coef[r, F:2 * F].abs().max().item() == 0.0
    # the empty rows: zeros in every block, no gradient for y, arg -1; the unreferenced source: no gradient
    for r in (0, n_dst - 1):
        assert out[r].abs().max().item() == 0.0 and stats[r].abs().max().item() == 0.0 and bool((arg[r] == -1).all())
        assert read("gy", dtype, (n_dst, F))[r].abs().max().item() == 0.0 and coef[r].abs().max().item() == 0.0
    assert gx[-1].abs().max().item() == 0.0


# fp32: F = 8 (two vectors on eight lanes: idle lanes), 20 (five vectors, not a power of two), 64; bf16: 8 (one vector), 24; fp32 260:
# 65 vectors, two column blocks (on the small graph)
@pytest.mark.parametrize("with_y", [False, True], ids=["noy", "y"])
@pytest.mark.parametrize("F,dtype", [(8, torch.float32), (20, torch.float32), (64, torch.float32), (8, torch.bfloat16), (24, torch.bfloat16),
                                     (260, torch.float32)], ids=lambda v: str(v).replace("torch.", ""))
def test_all_passes_in_lock_step(emulator, tmp_path, F, dtype, with_y):
    _run(emulator, tmp_path, _graph(full=F < 260), F, dtype, with_y)
