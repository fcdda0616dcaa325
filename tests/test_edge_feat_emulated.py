"""csrc/edge_feat.hip without a GPU: the kernel source and csrc/row_tiles.hpp, both UNMODIFIED, compiled with g++ against the host
stand-ins of tests/kernel_emu/ and run in lock step (tests/kernel_emu.py; test_sparse_attn_emulated.py says what that checks and what
it cannot) against the float64 per-edge restatement of ef_ref.py.  All three passes, all three ops, with and without the per-row
scale of the mean reduce, on the graphs of test_pna_emulated.py.

Bars: fp32 forward max |err| <= 1e-4 max |ref|, gradients <= 2e-3 max |ref|; bf16 forward <= 2e-2 max |ref|,
gradients relative L2 <= 1.5e-2, the reference computed on the bf16-rounded inputs.  No element is excluded (ef_ref.py says why the
gates agree)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import ef_ref
from kernel_emu import build_emulator
from test_pna_emulated import _dump, _graph, _read

FILL = {torch.float32: (np.int32, -842150451), torch.bfloat16: (np.int16, -12851)}      # 0xCD bytes: what the kernel did not write


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return build_emulator(tmp_path_factory, "edge_feat.hip", "edge_feat_main.cpp")


def _err(name, got, want, kind):
    a, b = got.double(), want.double()
    assert bool(torch.isfinite(a).all()), name
    err_max = ((a - b).abs().max() / b.abs().max()).item()
    err_l2 = ((a - b).norm() / b.norm()).item()
    bar, err = {"fwd32": (1e-4, err_max), "grad32": (2e-3, err_max), "fwd16": (2e-2, err_max), "grad16": (1.5e-2, err_l2)}[kind]
    print("%-16s max/max %.3e  rel-l2 %.3e  bar %.1e" % (name, err_max, err_l2, bar))
    assert err <= bar, (name, err, bar)


def _run(emulator, tmp_path, graph, F, dtype, ld_e, nulls):
    d, half = str(tmp_path), dtype == torch.bfloat16
    n_dst, n_src, nnz = graph.n_rows, graph.n_cols, graph.nnz
    gen = torch.Generator().manual_seed(F + 3)
    gt, perm = graph.transpose()
    x = torch.randn(n_src, F, generator=gen).to(dtype)
    e_pitched = torch.randn(nnz, ld_e, generator=gen).to(dtype)
    go = torch.randn(n_dst, F, generator=gen).to(dtype)
    deg = graph.degrees().to(torch.float32)
    scale = torch.where(deg > 0, 1.0 / deg.clamp(min=1.0), torch.zeros_like(deg))
    for name, t in (("rowptr", graph.rowptr), ("col", graph.col), ("trowptr", gt.rowptr), ("tcol", gt.col), ("perm", perm),
                    ("scale", scale), ("x", x), ("e", e_pitched), ("go", go)):
        _dump(t, os.path.join(d, name + ".bin"))
    res = subprocess.run([emulator, d, str(n_dst), str(n_src), str(F), "1" if half else "0", str(ld_e), str(nulls)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "emu ok" in res.stdout, res.stdout + res.stderr

    # the transposed order really differs from A's, and the five-times column has five different e rows
    assert not torch.equal(perm, torch.arange(nnz))
    x64, e64, g64 = x.double(), e_pitched[:, :F].double(), go.double()
    fwd, grad = ("fwd16", "grad16") if half else ("fwd32", "grad32")
    for o, op in enumerate(ef_ref.OPS):
        for m, reduce in enumerate(("sum", "mean")):
            tag = "_%d_%d" % (o, m)
            name = "%s/%s" % (op, reduce)
            out = _read(os.path.join(d, "out" + tag + ".bin"), dtype, (n_dst, F))
            gx = _read(os.path.join(d, "gx" + tag + ".bin"), dtype, (n_src, F))
            ge = _read(os.path.join(d, "ge" + tag + ".bin"), dtype, (nnz, ld_e))
            want_gx, want_ge = ef_ref.gradients(graph.rowptr, graph.col, x64, e64, g64, op, reduce)
            _err("out " + name, out, ef_ref.forward(graph.rowptr, graph.col, x64, e64, op, reduce), fwd)
            _err("gx " + name, gx, want_gx, grad)
            _err("ge " + name, ge[:, :F], want_ge, grad)
            # rows without entries give zeros; the source no row references gets no gradient; the pitch's padding is not written
            assert out[0].abs().max().item() == 0.0 and out[-1].abs().max().item() == 0.0
            assert gx[-1].abs().max().item() == 0.0
            if ld_e > F:
                np_dtype, fill = FILL[dtype]
                raw = np.fromfile(os.path.join(d, "ge" + tag + ".bin"), dtype=np_dtype).reshape(nnz, ld_e)
                assert (raw[:, F:] == fill).all(), name
            if op == "add_relu":            # the gates are the reference's, element for element: a closed gate writes an exact 0
                assert torch.equal(ge[:, :F] != 0, want_ge != 0), name


# one vector (seven idle lanes of the group), six vectors (not a power of two; e and grad_e on a wider pitch), 65 vectors (two column
# blocks, on the small graph).  nulls: the operands a (pass, op) does not read are NULL; 0: all are given, and must make no difference
@pytest.mark.parametrize("F,dtype,pad,nulls", [(4, torch.float32, 0, 1), (24, torch.float32, 8, 1), (260, torch.float32, 0, 0),
                                               (8, torch.bfloat16, 0, 0), (48, torch.bfloat16, 8, 1), (520, torch.bfloat16, 16, 1)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_all_passes_in_lock_step(emulator, tmp_path, F, dtype, pad, nulls):
    _run(emulator, tmp_path, _graph(full=F < 260), F, dtype, F + pad, nulls)
