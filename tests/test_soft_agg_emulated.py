"""csrc/soft_agg.hip without a GPU: the kernel source and csrc/row_tiles.hpp, both UNMODIFIED, compiled with g++ against the host
stand-ins of tests/kernel_emu/ and run in lock step (tests/kernel_emu.py; test_sparse_attn_emulated.py says what that checks and what
it cannot) against the float64 per-entry restatement of softagg_ref.py.  All three passes, both modes, with and without e, both
dtypes, on the graphs of test_pna_emulated.py (empty rows, one entry, 64, 65, one column five times, LONG_ROW, LONG_ROW + 1, 400);
x and grad_x on a pitch wider than F with NaN behind the row; the scalar gradient over the full and over a bounded grid of three
workgroups; the rows pass with grad_e alone.  t = 8 makes the running maximum of a column change often and the long-row merge rescale;
t = -0.5 turns the softmax towards the smallest message.

Bars: fp32 forward max |err| <= 1e-4 max |ref|, gradients <= 2e-3 max |ref|; bf16 forward <= 2e-2 max |ref|,
gradients relative L2 <= 1.5e-2, the reference computed on the bf16-rounded inputs; grad_t / grad_p: |err| <= 2e-3 (fp32) / 1.5e-2
(bf16) of the reference's sum |g * d out / d theta| (one sum over the whole graph that may cancel).  No element is excluded."""
import os
import subprocess

import numpy as np
import pytest
import torch

import softagg_ref
from kernel_emu import build_emulator
from test_pna_emulated import _dump, _graph, _read

FILL = {torch.float32: (np.int32, -842150451), torch.bfloat16: (np.int16, -12851)}      # 0xCD bytes: what the kernel did not write
EPS = 1e-7


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return build_emulator(tmp_path_factory, "soft_agg.hip", "soft_agg_main.cpp")


def _err(name, got, want, kind):
    a, b = got.double(), want.double()
    assert bool(torch.isfinite(a).all()), name
    err_max = ((a - b).abs().max() / b.abs().max()).item()
    err_l2 = ((a - b).norm() / b.norm()).item()
    bar, err = {"fwd32": (1e-4, err_max), "grad32": (2e-3, err_max), "fwd16": (2e-2, err_max), "grad16": (1.5e-2, err_l2)}[kind]
    print("%-10s max/max %.3e  rel-l2 %.3e  bar %.1e" % (name, err_max, err_l2, bar))
    assert err <= bar, (name, err, bar)


def _run(emulator, tmp_path, graph, F, dtype, ld, mode, theta, with_e, semi=False):
    from dgll_amd import ops_agg, ops_softagg

    assert ops_softagg.LONG_ROW == ops_agg.LONG_ROW                                 # the graphs' long rows are this pass's long rows
    d, half = str(tmp_path), dtype == torch.bfloat16
    n_dst, n_src, nnz = graph.n_rows, graph.n_cols, graph.nnz
    gen = torch.Generator().manual_seed(F + 5)
    gt, perm = graph.transpose()
    x, go = (torch.randn(n, F, generator=gen).to(dtype) for n in (n_src, n_dst))
    e = torch.randn(nnz, F, generator=gen).to(dtype) if with_e else None
    xp = torch.full((n_src, ld), float("nan"), dtype=dtype)
    xp[:, :F] = x
    th = torch.tensor([theta], dtype=torch.float32)
    for name, t in (("rowptr", graph.rowptr), ("col", graph.col), ("trowptr", gt.rowptr), ("tcol", gt.col), ("perm", perm.long()),
                    ("theta", th), ("x", xp), ("go", go)) + ((("e", e),) if with_e else ()):
        _dump(t, os.path.join(d, name + ".bin"))
    res = subprocess.run([emulator, d, str(n_dst), str(n_src), str(F), "1" if half else "0", str(ld), str(softagg_ref.MODES.index(mode)),
                          "1" if with_e else "0", "1" if semi else "0", repr(EPS)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "emu ok" in res.stdout, res.stdout + res.stderr
    read = lambda n, dt, shape: _read(os.path.join(d, n + ".bin"), dt, shape)      # noqa: E731

    assert not torch.equal(perm, torch.arange(nnz))                                 # the transposed order really differs from A's
    want = softagg_ref.reference(graph.rowptr, graph.col, x, e, th.item(), go, mode, EPS, semi)
    fwd, grad = ("fwd16", "grad16") if half else ("fwd32", "grad32")

    out, stats = read("out", dtype, (n_dst, F)), read("stats", torch.float32, (n_dst, 2 * F))
    _err("out", out, want["out"], fwd)
    _err("stats out", stats[:, F:] if mode == "softmax" else stats[:, :F], want["out"], "fwd32")      # the unrounded out, fp32 in both dtypes
    gx = read("gx", dtype, (n_src, ld))
    _err("gx", gx[:, :F], want["grad_x"], grad)
    if with_e:
        ge = read("ge", dtype, (nnz, F))
        _err("ge", ge, want["grad_e"], grad)
        assert torch.equal(read("ge_only", dtype, (nnz, F)), ge)                    # grad_e alone: the same bits
    if not semi:
        bar = (1.5e-2 if half else 2e-3) * want["scale"]
        for name in ("gth", "gth3"):
            got = float(np.fromfile(os.path.join(d, name + ".bin"), dtype=np.float32)[0])
            print("%-10s %.6e  ref %.6e  |err| %.3e  bar %.3e" % (name, got, want["grad_theta"], abs(got - want["grad_theta"]), bar))
            assert np.isfinite(got) and abs(got - want["grad_theta"]) <= bar, (name, got, want["grad_theta"], bar)
    # rows without entries give zeros (statistics included); the source no row references gets no gradient; the pitch's padding is
    # not written
    for r in (0, n_dst - 1):
        assert out[r].abs().max().item() == 0.0 and stats[r].abs().max().item() == 0.0
    assert gx[-1, :F].abs().max().item() == 0.0
    if ld > F:
        np_dtype, fill = FILL[dtype]
        raw = np.fromfile(os.path.join(d, "gx.bin"), dtype=np_dtype).reshape(n_src, ld)
        assert (raw[:, F:] == fill).all()


def test_long_row_threshold_is_the_one_the_graphs_are_built_for():
    from dgll_amd import ops_agg, ops_softagg

    assert ops_softagg.LONG_ROW == ops_agg.LONG_ROW


# one vector (seven idle lanes of the group), six vectors (not a power of two; x and grad_x on a wider pitch), 65 vectors (two column
# blocks, on the small graph)
WIDTHS = [(4, torch.float32, 0), (24, torch.float32, 8), (260, torch.float32, 0), (8, torch.bfloat16, 0), (48, torch.bfloat16, 8),
          (520, torch.bfloat16, 16)]
_ids = lambda v: str(v).replace("torch.", "")       # noqa: E731


@pytest.mark.parametrize("with_e", [False, True], ids=["noe", "e"])
@pytest.mark.parametrize("t", [1.0, -0.5, 8.0])
@pytest.mark.parametrize("F,dtype,pad", WIDTHS, ids=_ids)
def test_softmax_passes_in_lock_step(emulator, tmp_path, F, dtype, pad, t, with_e):
    _run(emulator, tmp_path, _graph(full=F < 260), F, dtype, F + pad, "softmax", t, with_e)


@pytest.mark.parametrize("with_e", [False, True], ids=["noe", "e"])
@pytest.mark.parametrize("p", [0.5, 2.0])
@pytest.mark.parametrize("F,dtype,pad", WIDTHS, ids=_ids)
def test_power_mean_passes_in_lock_step(emulator, tmp_path, F, dtype, pad, p, with_e):
    _run(emulator, tmp_path, _graph(full=F < 260), F, dtype, F + pad, "power", p, with_e)


@pytest.mark.parametrize("F,dtype,pad", [(24, torch.float32, 8), (48, torch.bfloat16, 8)], ids=_ids)
def test_semi_grad_passes_in_lock_step(emulator, tmp_path, F, dtype, pad):
    """the softmax weights as constants of the backward: grad_x and grad_e without the t (m - out) term, and no scalar gradient"""
    _run(emulator, tmp_path, _graph(full=True), F, dtype, F + pad, "softmax", 2.0, True, semi=True)
