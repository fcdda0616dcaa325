"""csrc/res_gated.hip without a GPU: the kernel source and csrc/row_tiles.hpp, both UNMODIFIED, compiled with g++ against the host
stand-ins of tests/kernel_emu/ and run in lock step (tests/kernel_emu.py; test_sparse_attn_emulated.py says what that checks and what
it cannot) against the float64 per-edge restatement of res_gated_ref.py.  All three passes, both dtypes, on the graphs of
test_pna_emulated.py; q, v and grad_q on a pitch wider than F with NaN behind the row; one case with `mean`; the cols pass with one
output alone.

Bars: fp32 forward max |err| <= 1e-4 max |ref|, gradients <= 2e-3 max |ref|; bf16 forward <= 2e-2 max |ref|,
gradients relative L2 <= 1.5e-2, the reference computed on the bf16-rounded inputs.  No element is excluded (res_gated_ref.py)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import res_gated_ref
from kernel_emu import build_emulator
from test_pna_emulated import _dump, _graph, _read

FILL = {torch.float32: (np.int32, -842150451), torch.bfloat16: (np.int16, -12851)}      # 0xCD bytes: what the kernel did not write


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return build_emulator(tmp_path_factory, "res_gated.hip", "res_gated_main.cpp")


def _err(name, got, want, kind):
    a, b = got.double(), want.double()
    assert bool(torch.isfinite(a).all()), name
    err_max = ((a - b).abs().max() / b.abs().max()).item()
    err_l2 = ((a - b).norm() / b.norm()).item()
    bar, err = {"fwd32": (1e-4, err_max), "grad32": (2e-3, err_max), "fwd16": (2e-2, err_max), "grad16": (1.5e-2, err_l2)}[kind]
    print("%-10s max/max %.3e  rel-l2 %.3e  bar %.1e" % (name, err_max, err_l2, bar))
    assert err <= bar, (name, err, bar)


def _run(emulator, tmp_path, graph, F, dtype, ld, mean):
    d, half = str(tmp_path), dtype == torch.bfloat16
    n_dst, n_src, nnz = graph.n_rows, graph.n_cols, graph.nnz
    gen = torch.Generator().manual_seed(F + 5)
    gt, perm = graph.transpose()
    k, q, v, go = (torch.randn(n, F, generator=gen).to(dtype) for n in (n_dst, n_src, n_src, n_dst))

    def pitched(t):
        buf = torch.full((t.shape[0], ld), float("nan"), dtype=dtype)
        buf[:, :F] = t
        return buf

    for name, t in (("rowptr", graph.rowptr), ("col", graph.col), ("trowptr", gt.rowptr), ("tcol", gt.col),
                    ("k", k), ("q", pitched(q)), ("v", pitched(v)), ("go", go)):
        _dump(t, os.path.join(d, name + ".bin"))
    res = subprocess.run([emulator, d, str(n_dst), str(n_src), str(F), "1" if half else "0", str(ld), "1" if mean else "0"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "emu ok" in res.stdout, res.stdout + res.stderr
    read = lambda n, dt, shape: _read(os.path.join(d, n + ".bin"), dt, shape)      # noqa: E731

    assert not torch.equal(perm, torch.arange(nnz))                                 # the transposed order really differs from A's
    ins = [t.double() for t in (k, q, v)]
    want_out = res_gated_ref.forward(graph.rowptr, graph.col, *ins, mean=mean)
    want = res_gated_ref.gradients(graph.rowptr, graph.col, *ins, go.double())      # rows and cols do not read `mean`
    fwd, grad = ("fwd16", "grad16") if half else ("fwd32", "grad32")

    out = read("out", dtype, (n_dst, F))
    _err("out", out, want_out, fwd)
    gk, gq, gv = read("gk", dtype, (n_dst, F)), read("gq", dtype, (n_src, ld)), read("gv", dtype, (n_src, F))
    for name, g, w in zip(("gk", "gq", "gv"), (gk, gq[:, :F], gv), want):
        _err(name, g, w, grad)
    # one output alone: the same bits
    assert torch.equal(read("gq_only", dtype, (n_src, ld))[:, :F], gq[:, :F]) and torch.equal(read("gv_only", dtype, (n_src, F)), gv)
    # rows without entries give zeros; the source no row references gets no gradient; the pitch's padding is not written
    for r in (0, n_dst - 1):
        assert out[r].abs().max().item() == 0.0 and gk[r].abs().max().item() == 0.0
    assert gq[-1, :F].abs().max().item() == 0.0 and gv[-1].abs().max().item() == 0.0
    if ld > F:
        np_dtype, fill = FILL[dtype]
        for name in ("gq", "gq_only"):
            raw = np.fromfile(os.path.join(d, name + ".bin"), dtype=np_dtype).reshape(n_src, ld)
            assert (raw[:, F:] == fill).all(), name


# one vector (seven idle lanes of the group), six vectors (not a power of two; q, v and grad_q on a wider pitch), 65 vectors (two
# column blocks, on the small graph); one case with the mean
@pytest.mark.parametrize("F,dtype,pad,mean", [(4, torch.float32, 0, False), (24, torch.float32, 8, True), (260, torch.float32, 0, False),
                                              (8, torch.bfloat16, 0, False), (48, torch.bfloat16, 8, False), (520, torch.bfloat16, 16, False)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_all_passes_in_lock_step(emulator, tmp_path, F, dtype, pad, mean):
    _run(emulator, tmp_path, _graph(full=F < 260), F, dtype, F + pad, mean)
