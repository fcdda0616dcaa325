"""csrc/gatv2.hip without a GPU: the kernel source and csrc/row_tiles.hpp, both UNMODIFIED, compiled with g++ against host stand-ins
for common.hpp and edge_args.hpp (tests/kernel_emu/) and run in lock step -- a fiber per lane, 256 per workgroup, wave shuffles and
__syncthreads as collectives that fail when a lane does not reach them, every buffer ending at a guard page -- against the float64
restatement of test_gatv2_host.py, at the bars of test_gatv2_gpu.py.

It checks what the source says (lane layout, index batches, online softmax, the long-row merge, the three gradients, bounds and
alignment of every access); it cannot check what only the card shows (the exp2 / log instructions, execution masks, timing)."""
import os
import subprocess

import numpy as np
import pytest
import torch

from kernel_emu import build_emulator
from test_gatv2_host import gatv2_reference


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return build_emulator(tmp_path_factory, "gatv2.hip", "gatv2_main.cpp")


def _graph(full):
    """full -- 24 x 30: an empty row, one entry, 64, 65, one column five times, LONG_ROW, LONG_ROW + 1 and 400 entries (columns with
    repetition), short rows, an empty last row; the last source is never referenced.  Not full -- 9 x 12: empty, one entry, LONG_ROW + 1,
    short rows, empty (the wide case, whose emulation costs most per entry)."""
    from dgll_amd import CSRGraph, ops_gatv2

    rng = np.random.RandomState(9)
    n_src = 30 if full else 12
    draw = lambda k: list(rng.randint(0, n_src - 1, k))         # noqa: E731
    if full:
        rows = [[], [7], draw(64), draw(65), [11] * 5, draw(ops_gatv2.LONG_ROW), draw(ops_gatv2.LONG_ROW + 1), draw(400)]
        rows += [draw(rng.randint(1, 9)) for _ in range(15)] + [[]]
    else:
        rows = [[], [7], draw(ops_gatv2.LONG_ROW + 1)] + [draw(rng.randint(1, 9)) for _ in range(5)] + [[]]
    rowptr = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
    return CSRGraph(rowptr, torch.tensor([int(c) for r in rows for c in r], dtype=torch.int32), None, len(rows), n_src)


def _dump(t, path):
    (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).contiguous().numpy().tofile(path)


def _read(path, dtype, shape):
    if dtype == torch.bfloat16:
        return torch.from_numpy(np.fromfile(path, dtype=np.int16)).view(torch.bfloat16).reshape(shape)
    return torch.from_numpy(np.fromfile(path, dtype=np.float32)).reshape(shape)


# lanes per head / per row: 8 x 16 fp32 = 4 / 32; 3 x 24 bf16 = 3 of 4 / 16 (idle lanes, 4 rows a wavefront); 5 x 8 fp32 = 2 / 16
# (3 idle heads); 3 x 128 fp32 = 32 / 64 in two column blocks (the second half empty); 1 x 48 bf16 = 6 of 8 / 8
@pytest.mark.parametrize("heads,D,dtype", [(8, 16, torch.float32), (3, 24, torch.bfloat16), (5, 8, torch.float32), (3, 128, torch.float32),
                                           (1, 48, torch.bfloat16)], ids=lambda v: str(v).replace("torch.", ""))
def test_kernel_source_in_lock_step(emulator, tmp_path, heads, D, dtype):
    graph = _graph(full=D < 128)
    gen = torch.Generator().manual_seed(heads * 100 + D)
    F, d = heads * D, str(tmp_path)
    xl = torch.randn(graph.n_cols, F, generator=gen).to(dtype)
    xr = torch.randn(graph.n_rows, F, generator=gen).to(dtype)
    attn = torch.randn(heads, D, generator=gen) / D ** 0.5
    g = torch.randn(graph.n_rows, F, generator=gen).to(dtype)
    gt, _ = graph.transpose()
    for name, t in (("rowptr", graph.rowptr), ("col", graph.col), ("trowptr", gt.rowptr), ("tcol", gt.col), ("xl", xl), ("xr", xr),
                    ("g", g), ("attn", attn)):
        _dump(t, os.path.join(d, name + ".bin"))
    res = subprocess.run([emulator, d, str(graph.n_rows), str(graph.n_cols), str(heads), str(D), "0" if dtype == torch.float32 else "1",
                          "0.2", "3"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "emu ok" in res.stdout, res.stdout + res.stderr
    got = [_read(os.path.join(d, "out.bin"), dtype, (graph.n_rows, F)), _read(os.path.join(d, "dxl.bin"), dtype, (graph.n_cols, F)),
           _read(os.path.join(d, "dxr.bin"), dtype, (graph.n_rows, F)), _read(os.path.join(d, "dattn.bin"), torch.float32, (heads, D))]
    xl64, xr64, a64 = (t.double().requires_grad_() for t in (xl, xr, attn))
    out, _ = gatv2_reference(graph.rowptr, graph.col, xl64.view(-1, heads, D), xr64.view(-1, heads, D), a64, 0.2)
    out = out.reshape(graph.n_rows, F)
    want = [out.detach()] + list(torch.autograd.grad(out, (xl64, xr64, a64), g.double()))
    for name, a, b in zip(("out", "dxl", "dxr", "dattn"), got, want):
        a = a.double()
        assert bool(torch.isfinite(a).all()), name
        if dtype == torch.float32:
            assert ((a - b).abs().max() / b.abs().max()).item() <= (1e-4 if name == "out" else 2e-3), name
        elif name == "out":
            assert ((a - b).abs().max() / b.abs().max()).item() <= 2e-2, name
        else:
            assert ((a - b).norm() / b.norm()).item() <= 1.5e-2, name
    assert got[0][0].abs().max().item() == 0.0 and got[0][-1].abs().max().item() == 0.0         # the empty rows
    assert got[1][-1].abs().max().item() == 0.0                                                 # the unreferenced source


# The closed-form legs of rowtile_ref.py on the source (cut-down graph: rows of 0, 1, 7 .. 9, 63 .. 65, 255 .. 257 and 400 distinct
# entries): 3 x 24 bf16 = 3 of 4 lanes a head, 12 of 16 lanes a row; 5 x 8 fp32 = 5 heads of 2 lanes in 16 (3 idle heads);
# 33 x 8 fp32 = two column blocks of 32 heads of 2 lanes, the second with one head.  One dattn partial: every tile grid-stride in one workgroup.
@pytest.mark.parametrize("leg", ["flat", "onehot"])
@pytest.mark.parametrize("heads,D,dtype", [(3, 24, torch.bfloat16), (5, 8, torch.float32), (33, 8, torch.float32)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_closed_form_legs_in_lock_step(emulator, tmp_path, heads, D, dtype, leg):
    import rowtile_ref as R

    graph = R.emu_graph()
    case = R.Case(dtype, heads, D, None)
    xl, xr, attn, g, slope = R.gatv2_operands(graph, case, leg)
    F, d = heads * D, str(tmp_path)
    gt, _ = graph.csr().transpose()
    for name, t in (("rowptr", graph.rowptr), ("col", graph.col), ("trowptr", gt.rowptr), ("tcol", gt.col), ("xl", xl), ("xr", xr),
                    ("g", g), ("attn", attn)):
        _dump(t, os.path.join(d, name + ".bin"))
    res = subprocess.run([emulator, d, str(graph.n_rows), str(graph.n_cols), str(heads), str(D), "0" if dtype == torch.float32 else "1",
                          repr(slope), "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "emu ok" in res.stdout, res.stdout + res.stderr
    got = {"out": _read(os.path.join(d, "out.bin"), dtype, (graph.n_rows, F)), "dxl": _read(os.path.join(d, "dxl.bin"), dtype, (graph.n_cols, F)),
           "dxr": _read(os.path.join(d, "dxr.bin"), dtype, (graph.n_rows, F)), "dattn": _read(os.path.join(d, "dattn.bin"), torch.float32, (1, F))}
    lse = _read(os.path.join(d, "lse.bin"), torch.float32, (graph.n_rows, heads))
    ref = R.gatv2_reference(graph, xl, xr, attn, g, heads, slope)
    empty = np.flatnonzero(graph.deg == 0)
    bad = R.check_finite("out", got["out"]) + R.check_finite("lse", lse) + R.check_zero_rows("out", got["out"], empty) \
        + R.check_zero_rows("lse", lse, empty)
    if leg == "onehot":
        win, mult, top = R.winners(graph, ref["s"])
        want, keep = R.onehot_expected(graph, xl, win, mult, heads)
        assert bool(keep.all())
        bad += R.check_equal("out", got["out"], want, keep, heads)
        bad += R.check_lse("lse", lse, *R.onehot_lse(top, mult))[0]
    else:
        bad += R.check_flat_forward("out", got["out"], ref["mean"])[0]
        bad += R.check_lse("lse", lse, ref["lse"], R.flat_lse_bar(graph, ref))[0]
        for name in ("dxl", "dxr", "dattn"):
            found, frac = R.check_units(name, got[name], ref[name])
            print("%s %dx%d %s: %.3f of the bar" % (leg, heads, D, name, frac))
            bad += found + R.check_finite(name, got[name])
        bad += R.check_zero_rows("dxr", got["dxr"], empty) + R.check_zero_rows("dxl", got["dxl"], graph.unreferenced)
    assert not bad, "\n".join(bad)
