"""csrc/gated.hip without a GPU: the kernel source and csrc/row_tiles.hpp, both UNMODIFIED, compiled with g++ against the host
stand-ins of tests/kernel_emu/ and run in lock step (tests/kernel_emu.py; test_sparse_attn_emulated.py says what that checks and what
it cannot) against the float64 per-edge restatement of gated_ref.py.  All three passes, both dtypes, on the graphs of
test_pna_emulated.py; c, ehat and grad_c on a pitch wider than F; with and without a gradient through ehat; the rows pass that only
leaves w and the cols pass with one output alone.

Bars: fp32 forward max |err| <= 1e-4 max |ref|, gradients <= 2e-3 max |ref|; bf16 forward <= 2e-2 max |ref|,
gradients relative L2 <= 1.5e-2, the reference computed on the bf16-rounded inputs.  No element is excluded (gated_ref.py)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import gated_ref
from kernel_emu import build_emulator
from test_pna_emulated import _dump, _graph, _read

FILL = {torch.float32: (np.int32, -842150451), torch.bfloat16: (np.int16, -12851)}      # 0xCD bytes: what the kernel did not write
EPS = 1e-6


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return build_emulator(tmp_path_factory, "gated.hip", "gated_main.cpp")


def _err(name, got, want, kind):
    a, b = got.double(), want.double()
    assert bool(torch.isfinite(a).all()), name
    err_max = ((a - b).abs().max() / b.abs().max()).item()
    err_l2 = ((a - b).norm() / b.norm()).item()
    bar, err = {"fwd32": (1e-4, err_max), "grad32": (2e-3, err_max), "fwd16": (2e-2, err_max), "grad16": (1.5e-2, err_l2)}[kind]
    print("%-10s max/max %.3e  rel-l2 %.3e  bar %.1e" % (name, err_max, err_l2, bar))
    assert err <= bar, (name, err, bar)


def _run(emulator, tmp_path, graph, F, dtype, ld_c, with_ge):
    d, half = str(tmp_path), dtype == torch.bfloat16
    n_dst, n_src, nnz = graph.n_rows, graph.n_cols, graph.nnz
    gen = torch.Generator().manual_seed(F + 5)
    gt, perm = graph.transpose()
    a, b, v = (torch.randn(n, F, generator=gen).to(dtype) for n in (n_dst, n_src, n_src))
    c_pitched = torch.randn(nnz, ld_c, generator=gen).to(dtype)
    go, ge = torch.randn(n_dst, F, generator=gen).to(dtype), torch.randn(nnz, F, generator=gen).to(dtype)
    for name, t in (("rowptr", graph.rowptr), ("col", graph.col), ("trowptr", gt.rowptr), ("tcol", gt.col), ("perm", perm),
                    ("a", a), ("b", b), ("v", v), ("c", c_pitched), ("go", go), ("ge", ge)):
        _dump(t, os.path.join(d, name + ".bin"))
    res = subprocess.run([emulator, d, str(n_dst), str(n_src), str(F), "1" if half else "0", str(ld_c), "1" if with_ge else "0"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "emu ok" in res.stdout, res.stdout + res.stderr
    read = lambda n, dt, shape: _read(os.path.join(d, n + ".bin"), dt, shape)      # noqa: E731

    assert not torch.equal(perm, torch.arange(nnz))                                 # the transposed order really differs from A's
    ins = [t.double() for t in (a, b, c_pitched[:, :F], v)]
    want_out, want_ehat = gated_ref.forward(graph.rowptr, graph.col, *ins, EPS)
    want = gated_ref.gradients(graph.rowptr, graph.col, *ins, EPS, go.double(), ge.double() if with_ge else None)
    fwd, grad = ("fwd16", "grad16") if half else ("fwd32", "grad32")

    out, ehat = read("out", dtype, (n_dst, F)), read("ehat", dtype, (nnz, ld_c))
    _err("out", out, want_out, fwd)
    _err("ehat", ehat[:, :F], want_ehat, fwd)
    _err("out32", read("o32", torch.float32, (n_dst, F)), want_out, fwd)
    got = {n: read(n, dtype, (rows, F)) for n, rows in (("ga", n_dst), ("gb", n_src), ("gv", n_src))}
    gc = read("gc", dtype, (nnz, ld_c))
    for name, g, w in zip(("ga", "gb", "gc", "gv"), (got["ga"], got["gb"], gc[:, :F], got["gv"]), want):
        _err(name, g, w, grad)
    # one output alone, and w from the rows pass that sweeps nothing: the same bits
    assert torch.equal(read("gb_only", dtype, (n_src, F)), got["gb"]) and torch.equal(read("gv_only", dtype, (n_src, F)), got["gv"])
    # rows without entries give zeros; the source no row references gets no gradient; the pitch's padding is not written
    for r in (0, n_dst - 1):
        assert out[r].abs().max().item() == 0.0 and got["ga"][r].abs().max().item() == 0.0
    assert got["gb"][-1].abs().max().item() == 0.0 and got["gv"][-1].abs().max().item() == 0.0
    if ld_c > F:
        np_dtype, fill = FILL[dtype]
        for name in ("ehat", "gc"):
            raw = np.fromfile(os.path.join(d, name + ".bin"), dtype=np_dtype).reshape(nnz, ld_c)
            assert (raw[:, F:] == fill).all(), name


# one vector (seven idle lanes of the group), six vectors (not a power of two; c, ehat and grad_c on a wider pitch), 65 vectors (two
# column blocks, on the small graph)
@pytest.mark.parametrize("F,dtype,pad,with_ge", [(4, torch.float32, 0, True), (24, torch.float32, 8, False), (260, torch.float32, 0, True),
                                                 (8, torch.bfloat16, 0, False), (48, torch.bfloat16, 8, True), (520, torch.bfloat16, 16, False)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_all_passes_in_lock_step(emulator, tmp_path, F, dtype, pad, with_ge):
    _run(emulator, tmp_path, _graph(full=F < 260), F, dtype, F + pad, with_ge)
