"""csrc/typed_spmm.hip without a GPU: the kernel source and csrc/row_tiles.hpp, both UNMODIFIED, compiled with g++ against host
stand-ins for common.hpp and edge_args.hpp (tests/kernel_emu/) and run in lock step -- a fiber per lane, 256 per workgroup, wave
shuffles and __syncthreads as collectives that fail when a lane does not reach them, every buffer ending at a guard page -- against
the float64 restatement of typed_ref.py, at the project's bars.

It checks what the source says (lane layout, index batches, basis blocks, the coefficient table, the long-row merge, the dot
products' butterfly, bounds and alignment of every access); it cannot check what only the card shows (execution masks, LDS, timing)."""
import os
import subprocess

import numpy as np
import pytest
import torch

from kernel_emu import build_emulator
from typed_ref import edge_dots_reference, typed_spmm_reference


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return build_emulator(tmp_path_factory, "typed_spmm.hip", "typed_spmm_main.cpp")


def _graph(full, R):
    """full -- 24 x 30: an empty row, one entry, 64, 65, one column five times (types 0 .. 4 mod R), LONG_ROW, LONG_ROW + 1 and 400
    entries (columns with repetition), short rows, an empty last row; the last source is never referenced.  Not full -- 9 x 12: empty,
    one entry, LONG_ROW + 1, short rows, empty (the wide case, whose emulation costs most per entry).  -> (CSRGraph, etype, norm)."""
    from dgll_amd import CSRGraph, _lib

    long_row = _lib.TYPED_LONG_ROW
    rng = np.random.RandomState(9)
    n_src = 30 if full else 12
    draw = lambda k: list(rng.randint(0, n_src - 1, k))         # noqa: E731
    if full:
        rows = [[], [7], draw(64), draw(65), [11] * 5, draw(long_row), draw(long_row + 1), draw(400)]
        rows += [draw(rng.randint(1, 9)) for _ in range(15)] + [[]]
    else:
        rows = [[], [7], draw(long_row + 1)] + [draw(rng.randint(1, 9)) for _ in range(5)] + [[]]
    rowptr = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
    nnz = int(rowptr[-1])
    etype = torch.from_numpy(rng.randint(0, R, nnz)).to(torch.int32)
    if full:
        etype[int(rowptr[4]):int(rowptr[5])] = torch.arange(5, dtype=torch.int32) % R
    norm = torch.from_numpy(rng.choice([0.25, 0.5, 1.0, 1.5], nnz)).to(torch.float32)
    return CSRGraph(rowptr, torch.tensor([int(c) for r in rows for c in r], dtype=torch.int32), None, len(rows), n_src), etype, norm


def _dump(t, path):
    (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).contiguous().numpy().tofile(path)


def _read(path, dtype, shape):
    if dtype == torch.bfloat16:
        return torch.from_numpy(np.fromfile(path, dtype=np.int16)).view(torch.bfloat16).reshape(shape)
    return torch.from_numpy(np.fromfile(path, dtype=np.float32)).reshape(shape)


# lanes per row / basis block: 16 fp32 = 4 of 8 lanes, block of 1; 24 bf16 = 3 of 8 lanes, 3 bases in a block of 4; 64 fp32 = 16 lanes,
# block of 4; 8 bf16 x 9 bases = 1 of 8 lanes, two blocks of 8 (the second with one basis), R * B = 360; 256 fp32 = 64 lanes in two
# column blocks (the 9-row graph).  A sixth case beyond the five of the feature's plan: R * B = 4160 > TYPED_COEFF_LDS, the table
# read from global memory
@pytest.mark.parametrize("F,B,R,dtype", [(16, 1, 3, torch.float32), (24, 3, 7, torch.bfloat16), (64, 4, 5, torch.float32),
                                         (8, 9, 40, torch.bfloat16), (256, 2, 3, torch.float32), (8, 8, 520, torch.bfloat16)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_kernel_source_in_lock_step(emulator, tmp_path, F, B, R, dtype):
    graph, etype, norm = _graph(full=F < 256, R=R)
    gen = torch.Generator().manual_seed(F * 100 + B)
    d = str(tmp_path)
    x = torch.randn(graph.n_cols, F, generator=gen).to(dtype)
    dz = torch.randn(graph.n_rows, B * F, generator=gen).to(dtype)
    coeff = torch.randn(R, B, generator=gen)
    gt, perm = graph.transpose()
    for name, t in (("rowptr", graph.rowptr), ("col", graph.col), ("etype", etype), ("norm", norm), ("trowptr", gt.rowptr), ("tcol", gt.col),
                    ("tetype", etype[perm]), ("tnorm", norm[perm]), ("coeff", coeff), ("x", x), ("dz", dz)):
        _dump(t, os.path.join(d, name + ".bin"))
    res = subprocess.run([emulator, d, str(graph.n_rows), str(graph.n_cols), str(F), str(B), str(R), "0" if dtype == torch.float32 else "1", "1"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "emu ok" in res.stdout, res.stdout + res.stderr
    ldp = (B + 3) // 4 * 4
    z = _read(os.path.join(d, "z.bin"), dtype, (graph.n_rows, B * F))
    dx = _read(os.path.join(d, "dx.bin"), dtype, (graph.n_cols, F))
    p = _read(os.path.join(d, "p.bin"), torch.float32, (graph.nnz, ldp))

    x64 = x.double().requires_grad_()
    want_z = typed_spmm_reference(graph.rowptr, graph.col, etype, norm, x64, coeff)
    want_dx, = torch.autograd.grad(want_z, x64, dz.double())
    want_p = edge_dots_reference(graph.rowptr, graph.col, x, dz, B)
    for name, a, b in (("z", z, want_z.detach()), ("dx", dx, want_dx), ("p", p[:, :B], want_p)):
        a = a.double()
        assert bool(torch.isfinite(a).all()), name
        if dtype == torch.float32:
            assert ((a - b).abs().max() / b.abs().max()).item() <= (1e-4 if name == "z" else 2e-3), name
        elif name == "z":
            assert ((a - b).abs().max() / b.abs().max()).item() <= 2e-2, name
        else:
            assert ((a - b).norm() / b.norm()).item() <= 1.5e-2, name
    assert z[0].abs().max().item() == 0.0 and z[-1].abs().max().item() == 0.0           # the empty rows
    assert dx[-1].abs().max().item() == 0.0                                            # the unreferenced source
    assert ldp == B or p[:, B:].abs().max().item() == 0.0                                 # P's padding columns
