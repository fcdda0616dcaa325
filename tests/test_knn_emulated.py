"""csrc/knn.hip without a GPU: the kernel source, UNMODIFIED, compiled with g++ against the host stand-ins of tests/kernel_emu/ and run
in lock step (tests/kernel_emu.py; test_sparse_attn_emulated.py says what that checks and what it cannot) against the float64 brute
force of knn_ref.py.

The coordinates are integers in [-16, 16] (knn_ref.lattice_case): every squared distance is an integer below 2^24, exact in fp32 and
with bf16 inputs whatever the order of the sum, so `col` and `dist` must equal the reference EXACTLY, in every row, and the ties the
lattice forces hold the index rule.  One call covers segments of 0, 1, 2, k, k + 1, 63, 64, 65, CAND_TILE - 1, CAND_TILE,
CAND_TILE + 1 and 2 CAND_TILE + 3 rows, one that spans more than one QUERY_TILE, and one of identical points.  x may sit on a pitch
wider than D with NaN behind the row; the outputs start as 0xCD bytes and end at a guard page."""
import os
import subprocess

import numpy as np
import pytest
import torch

import knn_ref
from kernel_emu import build_emulator


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return build_emulator(tmp_path_factory, "knn.hip", "knn_main.cpp")


def _dump(t, path):
    (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).contiguous().numpy().tofile(path)


def _run(emulator, tmp_path, k, D, dtype, excl, pad):
    from dgll_amd import knn as K

    sizes, x64, (ib, ie) = knn_ref.lattice_case(k, D, K.CAND_TILE, K.QUERY_TILE)
    n, ld = x64.shape[0], D + pad
    assert max(sizes) > K.QUERY_TILE and sizes.count(0) == 2
    xp = torch.full((n, ld), float("nan"), dtype=dtype)
    xp[:, :D] = torch.from_numpy(x64).to(dtype)
    assert torch.equal(xp[:, :D].double(), torch.from_numpy(x64))              # the storage dtype holds the lattice exactly
    rowptr = knn_ref.out_rowptr(sizes, k, excl)
    nnz = int(rowptr[-1])
    d = str(tmp_path)
    _dump(xp, os.path.join(d, "x.bin"))
    knn_ref.segment_bounds(sizes).tofile(os.path.join(d, "seg.bin"))
    rowptr.tofile(os.path.join(d, "rowptr.bin"))
    res = subprocess.run([emulator, d, str(n), str(D), "1" if dtype == torch.bfloat16 else "0", str(ld), str(len(sizes)), str(k),
                          "1" if excl else "0", str(nnz)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "emu ok" in res.stdout, res.stdout + res.stderr
    col = np.fromfile(os.path.join(d, "col.bin"), dtype=np.int32)
    dist = np.fromfile(os.path.join(d, "dist.bin"), dtype=np.float32)
    col2 = np.fromfile(os.path.join(d, "col_nodist.bin"), dtype=np.int32)

    want_ptr, want_col, want_dist = knn_ref.knn(x64, sizes, k, excl)
    assert np.array_equal(want_ptr, rowptr)
    assert col.shape == want_col.shape and dist.shape == want_dist.shape
    bad = np.nonzero(col.astype(np.int64) != want_col)[0]
    assert bad.size == 0, (bad[:5], col[bad[:5]], want_col[bad[:5]])
    assert np.array_equal(dist.astype(np.float64), want_dist)                   # exact, every slot (an unwritten one holds 0xCD bytes)
    assert np.array_equal(col2, col)
    # identical points: the first deg_i indices of the segment, self skipped by index when excluded, all at distance 0
    for i in range(ib, ie):
        want = [j for j in range(ib, ie) if not (excl and j == i)][:k]
        assert list(col[rowptr[i]:rowptr[i + 1]]) == want
        assert not dist[rowptr[i]:rowptr[i + 1]].any()


# (k, D, dtype, exclude_self, pad): every k of {1, 2, 20, 64} and every D of {1, 3, 4, 5, 64, 65, 256}; 33 is the first width past one
# column chunk.  pad == 0 with D off the vector width takes the scalar loads, a pad that completes the vector the 16-byte ones.
CASES = [(1, 1, torch.float32, False, 0), (2, 3, torch.float32, True, 0), (1, 3, torch.bfloat16, True, 0), (20, 3, torch.float32, True, 1),
         (20, 4, torch.float32, False, 0), (20, 5, torch.float32, True, 3), (20, 5, torch.bfloat16, False, 3),
         (20, 33, torch.float32, True, 3), (20, 64, torch.float32, True, 0), (20, 64, torch.bfloat16, False, 8),
         (64, 65, torch.float32, False, 0), (64, 65, torch.bfloat16, True, 7), (2, 256, torch.float32, False, 0),
         (64, 256, torch.bfloat16, True, 0)]


@pytest.mark.parametrize("k,D,dtype,excl,pad", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_knn_in_lock_step_is_exact_on_the_lattice(emulator, tmp_path, k, D, dtype, excl, pad):
    _run(emulator, tmp_path, k, D, dtype, excl, pad)


def test_the_cases_cover_every_k_and_width():
    assert {c[0] for c in CASES} == {1, 2, 20, 64}
    assert {c[1] for c in CASES} >= {1, 3, 4, 5, 64, 65, 256}
    assert {c[2] for c in CASES} == {torch.float32, torch.bfloat16} and {c[3] for c in CASES} == {False, True}
