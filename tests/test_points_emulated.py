"""csrc/fps.hip and csrc/radius.hip without a GPU: the kernel sources, UNMODIFIED, run in lock step on the host stand-ins of
tests/kernel_emu/ (test_sparse_attn_emulated.py says what that checks) against the float64 references of points_ref.py.  Integer
coordinates in [-16, 16] and D <= 32: every squared distance is an integer <= 32768, exact in fp32 and bf16, so every output must
equal the reference EXACTLY.  x may sit on a wider pitch with NaN behind the rows; outputs start as 0xCD bytes at a guard page."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import knn_ref
import points_ref
from conftest import ROOT
from kernel_emu import build_emulator

F32, BF16 = torch.float32, torch.bfloat16


def _emulator(tmp_path_factory, kernel):
    """build_emulator on directories that start with the two csrc headers the kernels include beside row_tiles.hpp"""
    def mktemp(name):
        work = tmp_path_factory.mktemp(name)
        for header in ("point_rows.hpp", "scan.hpp"):
            shutil.copy(os.path.join(ROOT, "dgll_amd", "csrc", header), work)
        return work
    return build_emulator(types.SimpleNamespace(mktemp=mktemp), kernel + ".hip", kernel + "_main.cpp")


@pytest.fixture(scope="module")
def emulators(tmp_path_factory):
    return {kernel: _emulator(tmp_path_factory, kernel) for kernel in ("fps", "radius")}


def padded(x64, D, pad, dtype):
    """x64 in the storage dtype on a pitch of D + pad, NaN behind every row"""
    xp = torch.full((x64.shape[0], D + pad), float("nan"), dtype=dtype)
    xp[:, :D] = torch.from_numpy(x64).to(dtype)
    assert torch.equal(xp[:, :D].double(), torch.from_numpy(x64))              # the storage dtype holds the lattice exactly
    return xp


def _bits(x64, D, pad, dtype):
    xp = padded(x64, D, pad, dtype)
    return (xp.view(torch.int16) if dtype == BF16 else xp).numpy()


def _emu(exe, d, files, *args):
    """the arrays of `files` into directory d, one emulator run on them, then reader(name, dtype) of its outputs"""
    for name, array in files.items():
        array.tofile(os.path.join(d, name + ".bin"))
    res = subprocess.run([exe, d] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "emu ok" in res.stdout, res.stdout + res.stderr
    return lambda name, dtype: np.fromfile(os.path.join(d, name + ".bin"), dtype=dtype)


# (D, dtype, pad, pts): pts dmin per lane in registers, 0 the scratch array; (5, F32, 0, 16) and (5, BF16, 0, 0) take the scalar loads
FPS_CASES = [(1, F32, 0, 4), (3, F32, 0, 4), (3, BF16, 1, 16), (3, F32, 1, 32), (4, F32, 0, 4), (5, F32, 0, 16), (5, BF16, 3, 4),
             (32, BF16, 0, 32), (32, F32, 0, 4), (3, F32, 0, 0), (5, BF16, 0, 0), (32, F32, 4, 0)]


@pytest.mark.parametrize("D,dtype,pad,pts", FPS_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_fps_in_lock_step_is_exact_on_the_lattice(emulators, tmp_path, D, dtype, pad, pts):
    sizes, counts, starts, x64 = points_ref.fps_case(D, pts)
    d, out_ptr = str(tmp_path), knn_ref.segment_bounds(counts)
    files = {"x": _bits(x64, D, pad, dtype), "seg": knn_ref.segment_bounds(sizes), "outptr": out_ptr, "start": np.asarray(starts, dtype=np.int64)}
    out = _emu(emulators["fps"], d, files, x64.shape[0], D, int(dtype == BF16), D + pad, len(sizes), max(sizes), int(out_ptr[-1]))
    idx, dmin = out("idx", np.int64), out("dmin", np.float32)
    want_idx, want_dmin = points_ref.fps(x64, sizes, counts, starts)
    assert np.array_equal(idx, want_idx), np.nonzero(idx != want_idx)[0][:5]
    assert np.array_equal(dmin.astype(np.float64), want_dmin)


# (K, D, dtype, pad, r2, mode): mode "square" / "square-noself" search x in itself, "bipartite" other queries in other segment sizes
RADIUS_CASES = [(1, 1, F32, 0, 0.0, "square"), (1, 3, BF16, 1, 9.0, "bipartite"), (32, 3, F32, 0, 9.0, "square-noself"),
                (32, 3, F32, 1, 1e6, "bipartite"), (32, 5, BF16, 3, 1e6, "square"), (32, 1, F32, 3, 9.0, "bipartite"),
                (64, 5, F32, 0, 9.0, "bipartite"), (64, 32, F32, 0, 1e6, "square-noself"), (64, 32, BF16, 0, 0.0, "bipartite"),
                (64, 3, BF16, 5, 1e6, "square"), (32, 32, F32, 4, 9.0, "square"), (1, 5, F32, 0, 1e6, "square-noself")]


@pytest.mark.parametrize("K,D,dtype,pad,r2,mode", RADIUS_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_radius_in_lock_step_is_exact_on_the_lattice(emulators, tmp_path, K, D, dtype, pad, r2, mode):
    square, excl = mode != "bipartite", mode == "square-noself"
    x_sizes, x64, y_sizes, y64, _ = points_ref.radius_case(K, D, not square)
    m, n = y64.shape[0], x64.shape[0]
    d, files = str(tmp_path), {"x": _bits(x64, D, pad, dtype), "xseg": knn_ref.segment_bounds(x_sizes)}
    if not square:
        files.update(y=_bits(y64, D, 0, dtype), yseg=knn_ref.segment_bounds(y_sizes))
    out = _emu(emulators["radius"], d, files, m, n, D, int(dtype == BF16), D + pad if square else D, D + pad, len(x_sizes), repr(r2), K,
               int(excl), int(square))
    rowptr, nnz, col, dist = out("rowptr", np.int64), int(out("nnz", np.int64)[0]), out("col", np.int32), out("dist", np.float32)
    want_ptr, want_col, want_dist = points_ref.radius(y64, y_sizes, x64, x_sizes, r2, K, excl)
    assert np.array_equal(rowptr, want_ptr) and nnz == want_ptr[-1]
    assert np.array_equal(col[:nnz].astype(np.int64), want_col)
    assert np.array_equal(dist[:nnz].astype(np.float64), want_dist)
    assert (col[nnz:] == np.int32(-842150451)).all()                            # 0xCDCDCDCD: nothing written behind nnz
