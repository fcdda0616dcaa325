"""csrc/segment_mm.hip without a GPU: the kernel source, UNMODIFIED, runs in lock step on the host stand-ins of tests/kernel_emu/
(test_sparse_attn_emulated.py says what that checks; the two MFMA instructions are wave-level collectives there) through its C entry
points, against the float64 loop of segmm_ref.py and the tile list of segmm_ref.plan_ref.  The file's ext_vector_type typedefs need
clang: this one emulator is built with the ROCm clang++ as a plain host compiler.

Integer operands in [-2, 2] only: every partial sum is exact in fp32 in any order, so every output must EQUAL the float64 result as
stored.  Every buffer has exactly the size the API reports or requires and ends at a guard page (an access behind it ends the run);
`a` and `g` carry NaN behind column K; outputs and workspaces start as 0xCD bytes, so what the kernels leave unwritten shows."""
import os
import subprocess

import numpy as np
import pytest
import torch

import dense_small_cases as sc
from kernel_emu import build_emulator, rocm_clang
from segmm_ref import grouped_refs, gw_slab, plan_ref, segment_ids

F32, BF16 = torch.float32, torch.bfloat16
EDGES = [0, 1, 0, 31, 32, 33, 0]
WG = [127, 128, 129]
SLAB = [700, 1, 1, 5]
CD16, CD32 = np.int16(-12851), np.int32(-842150451)           # 0xCDCD, 0xCDCDCDCD


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_emulator(tmp_path_factory, "segment_mm.hip", "segment_mm_main.cpp", compiler=rocm_clang())


def _bits(t, dtype):
    t = t.to(dtype).contiguous()
    return (t.view(torch.int16) if dtype == BF16 else t).numpy()


def _rows16(x64, dtype, spare):
    """(file array, pitch) of x64 [M, K] in `dtype`: rows on a 16-byte pitch (+ spare vectors), NaN behind column K, cut behind the last
    row's last vector -- exactly what the entry points require."""
    epv = 8 if dtype == BF16 else 4
    m, k = x64.shape
    kpad = sc.round_up(max(k, 1), epv)
    ld = kpad + spare * epv
    full = torch.full((m, ld), sc.NAN, dtype=dtype)
    full[:, :k] = x64.to(dtype)
    return _bits(full, dtype).reshape(-1)[:(m - 1) * ld + kpad if m else 0], ld


def _run(exe, d, files, *args):
    for name, array in files.items():
        np.ascontiguousarray(array).tofile(os.path.join(d, name + ".bin"))
    res = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "emu ok" in res.stdout, (res.returncode, res.stdout + res.stderr)
    return lambda name, dtype: np.fromfile(os.path.join(d, name + ".bin"), dtype=dtype)


def _index_files(seglen, rows, len_dtype, rows_dtype):
    files = {"seglen": np.asarray(seglen, dtype=len_dtype)}
    if rows is not None:
        files["rows"] = np.asarray(rows, dtype=rows_dtype)
    return files, np.dtype(len_dtype).itemsize, 0 if rows is None else np.dtype(rows_dtype).itemsize


def product(exe, d, x64, b, strides, n, seglen, dtype, rows=None, ranges=None, len_dtype=np.int64, rows_dtype=np.int64, wide=False,
            bdtype=None):
    """x64 [M, K] times the matrices that `strides` (r, k, n) address in the contiguous tensor b -> (c [M, n] float64, read), c on the exact
    pitch n (its end at the guard page) or, wide=True, on a wider multiple of 4 (the vector stores) whose padding must keep its 0xCD."""
    d = str(d)
    m, k = x64.shape
    R = len(seglen)
    bdtype = bdtype or dtype
    a_file, lda = _rows16(x64, dtype, spare=1)
    ldc = sc.round_up(n, 4) + 4 if wide else n
    files, len_bytes, rows_bytes = _index_files(seglen, rows, len_dtype, rows_dtype)
    files.update(a=a_file, b=_bits(b, bdtype).reshape(-1))
    ranges = [(0, R)] if ranges is None else ranges
    read = _run(exe, d, files, "fwd", d, int(dtype == BF16), m, k, n, lda, ldc, R, len_bytes, rows_bytes, int(bdtype == BF16), *strides,
                b.numel(), len(ranges), *[v for r in ranges for v in r])
    raw = read("c", np.int16 if dtype == BF16 else np.int32).reshape(m, ldc)
    assert (raw[:, n:] == (CD16 if dtype == BF16 else CD32)).all(), "written behind column N"
    c = torch.from_numpy(raw[:, :n].copy())
    return (c.view(BF16) if dtype == BF16 else c.view(F32)).double(), read


def gradw(exe, d, a64, g64, seglen, dtype, rows=None, len_dtype=np.int64, rows_dtype=np.int64):
    d = str(d)
    (m, k), n, R = a64.shape, g64.shape[1], len(seglen)
    (a_file, lda), (g_file, ldg) = _rows16(a64, dtype, spare=1), _rows16(g64, dtype, spare=0)
    files, len_bytes, rows_bytes = _index_files(seglen, rows, len_dtype, rows_dtype)
    files.update(a=a_file, g=g_file)
    read = _run(exe, d, files, "gradw", d, int(dtype == BF16), m, k, n, lda, ldg, R, len_bytes, rows_bytes)
    return torch.from_numpy(read("gw", np.float32).reshape(R, k, n)).double(), read


def same(got, ref, bf16_out):
    return torch.equal(got, sc.as_stored(ref, bf16_out).double())


def operands(m, k, n, R, seed):
    gen = torch.Generator().manual_seed(seed)
    return sc._draw(gen, (m, k), True, True), sc._draw(gen, (R, k, n), True, True), sc._draw(gen, (m, n), True, True)


def row_types(seglen, m, rows=None):
    """float64-reference type of each of the m rows: tile row t of the segments is row rows[t]; -1 where no valid entry names the row"""
    ids = segment_ids(torch.tensor([min(max(v, 0), m) for v in seglen], dtype=torch.int64))[:m]
    idx = torch.full((m,), -1, dtype=torch.int64)
    where = torch.arange(ids.numel()) if rows is None else torch.as_tensor(rows)[:ids.numel()]
    ok = (where >= 0) & (where < m)
    idx[where[ok]] = ids[ok]
    return idx


# ---- the tile list ------------------------------------------------------------------------------------------------------------------
def _lengths(R, kind, m):
    """R lengths with negatives, values above m and long runs of zeros; their clamped sum below / above / equal to m"""
    cycle = [0, 1, 33, 2, 0, 0, 5, -3, 0, 0, 0, 0, 64, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7]
    lens = [cycle[i % len(cycle)] for i in range(R)]
    if kind == "above" and R:
        lens[(2 * R) // 3] = m + 7                      # clamped to m: every later segment is empty at offset m
    if kind == "exact" and R:
        lens[-1] += m - sum(max(v, 0) for v in lens)
    return lens


def _check_plan(read, lens, m, unit):
    R = len(lens)
    segoff, tileptr, partptr = plan_ref(lens, m, unit)
    assert read("segoff", np.int64).tolist() == segoff
    assert read("tileptr", np.int32).tolist() == tileptr
    assert read("partptr", np.int32).tolist() == partptr
    if unit == 32:
        assert tileptr[R + 1] <= sc.ceil_div(m, 32) + R + 1                 # the forward's grid
    else:
        assert tileptr[R] <= sc.ceil_div(m, unit) + R                       # the weight gradient's grid
        assert unit == gw_slab(m) and partptr[R + 1] <= 2 * (m // unit) + 2      # its partial slots


@pytest.mark.parametrize("len_dtype", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("kind", ["below", "above", "exact"])
@pytest.mark.parametrize("R", [0, 1, 255, 256, 257, 700])
def test_plan_equals_the_reference(emu, tmp_path, R, kind, len_dtype):
    """segoff / tileptr / partptr of both launches (unit 32: the forward's; unit slab: the weight gradient's) against plan_ref, past the 256
    entries at which a thread of the plan kernel takes more than one segment; the grid bounds the host relies on hold."""
    m = 1700 if R else 70
    lens = _lengths(R, kind, m)
    if kind == "exact" and R == 1:
        lens = [m]
    a, b, g = operands(m, 1, 1, max(R, 1), 3)
    c, read = product(emu, tmp_path, a, b, (1, 1, 1), 1, lens, F32, len_dtype=len_dtype)
    _check_plan(read, lens, m, 32)
    idx = row_types(lens, m)
    assert same(c, grouped_refs(a, b[:R], g, idx)[0], False)              # (R = 0: all zeros, written by the pseudo segment)
    if R:
        gw, read = gradw(emu, tmp_path, a, g, lens, F32, len_dtype=len_dtype)
        _check_plan(read, lens, m, gw_slab(m))
        assert same(gw, grouped_refs(a, b[:R], g, idx)[2], False)


@pytest.mark.parametrize("m, lens", [(513 * 4, [513] * 4), (1025 + 513 + 2, [1025, 0, 513, 1, 1]), (70000, [1700, 0, 560, 561, 1120, 1121])],
                         ids=["4x513", "3slabs", "slab560"])
def test_partial_slots_near_their_bound(emu, tmp_path, m, lens):
    """Segments of slab + 1 rows fill the partial slots fastest: 8 of the 10 there are at M = 4 * 513; a segment of three slabs; the slab of
    560 rows that M = 70 000 gives, with segments of exactly one and two slabs, one row more, and four (1700: the rest is uncovered)."""
    a, b, g = operands(m, 1, 1, len(lens), 4)
    gw, read = gradw(emu, tmp_path, a, g, lens, F32)
    _check_plan(read, lens, m, gw_slab(m))
    assert same(gw, grouped_refs(a, b, g, row_types(lens, m))[2], False)


# ---- the three products ----------------------------------------------------------------------------------------------------------------
def _cases():
    out, i = [], 0
    for seglen in (EDGES, WG, SLAB):
        for k in (1, 17, 23, 40):
            for n in (1, 33, 64):
                out.append((seglen, k, n, (BF16, F32)[i % 2], (i // 2) % 2 == 1, (np.int64, np.int32)[(i // 4) % 2]))
                out.append((seglen, k, n, (F32, BF16)[i % 2], (i // 2) % 2 == 0, (np.int32, np.int64)[(i // 4) % 2]))
                i += 1
    out += [(EDGES, 17, 256, BF16, True, np.int32), (EDGES, 23, 256, F32, False, np.int64)]
    return out


CASES = _cases()
IDS = ["%dsegs-k%d-n%d-%s-%s-i%d" % (len(s), k, n, str(t)[6:], "rows" if r else "norows", np.dtype(w).itemsize * 8) for s, k, n, t, r, w in CASES]


@pytest.mark.parametrize("seglen, k, n, dtype, with_rows, width", CASES, ids=IDS)
def test_products_in_lock_step_are_exact(emu, tmp_path, seglen, k, n, dtype, with_rows, width):
    """forward, grad_a (the same kernel on the other pair of strides of b) and grad_b at ragged K (keep_first: NaN lies behind column K),
    ragged N and the wave tile's edges, with and without a row index, both index widths."""
    m, R = sum(seglen), len(seglen)
    a, b, g = operands(m, k, n, R, 100 * k + n)
    rows = torch.randperm(m, generator=torch.Generator().manual_seed(k + n)).tolist() if with_rows else None
    want = grouped_refs(a, b, g, row_types(seglen, m, rows))
    bf16 = dtype == BF16
    kw = dict(rows=rows, len_dtype=width, rows_dtype=width)
    c, _ = product(emu, tmp_path, a, b, (k * n, n, 1), n, seglen, dtype, wide=k % 2 == 1, **kw)
    assert same(c, want[0], bf16), "forward"
    ga, _ = product(emu, tmp_path, g, b, (k * n, 1, n), k, seglen, dtype, wide=k % 2 == 0, **kw)
    assert same(ga, want[1], bf16), "grad_a"
    gw, _ = gradw(emu, tmp_path, a, g, seglen, dtype, **kw)
    assert same(gw, want[2], False), "grad_b"


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("k, n", [(97, 7), (129, 7)])
def test_gradw_k_tile_edges(emu, tmp_path, k, n, dtype):
    """K = 97: wave 3 owns one column of a; K = 129: a second k block (blockIdx.y = 1) holding one column -- next to a two-slab segment"""
    a, b, g = operands(sum(SLAB), k, n, len(SLAB), k)
    gw, _ = gradw(emu, tmp_path, a, g, SLAB, dtype)
    assert same(gw, grouped_refs(a, b, g, row_types(SLAB, sum(SLAB)))[2], False)


# ---- segment ranges through the C API -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("seglen, m", [(EDGES, 97), ([1, 2, 3] * 3, 18), ([40, 0, 30, 5, 0, 2, 1], 100), ([40, 50, 70, 1, 1, 1, 1], 100)],
                         ids=["edges", "short", "sum-below", "sum-above"])
def test_segment_ranges_reuse_the_plan(emu, tmp_path, seglen, m, dtype):
    """Three launches over [0, 3), [3, 6), [6, R) with build_plan = 1, 0, 0, each on a packed buffer that holds its own range alone (and
    ends at a guard page): equal to the one-launch result and to float64.  With a seglen whose sum is not M: clamped segments, and the
    pseudo segment's rows zeroed by the first range only."""
    R, k, n = len(seglen), 23, 33
    a, b, g = operands(m, k, n, R, 9)
    want = grouped_refs(a, b, g, row_types(seglen, m))[0]
    parts, _ = product(emu, tmp_path, a, b, (k * n, n, 1), n, seglen, dtype, ranges=[(0, 3), (3, 6), (6, R)])
    whole, _ = product(emu, tmp_path, a, b, (k * n, n, 1), n, seglen, dtype, wide=True)
    assert same(parts, want, dtype == BF16) and torch.equal(parts, whole)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_no_segments_zeroes_c(emu, tmp_path, dtype):
    a, b, _ = operands(70, 8, 33, 1, 2)
    c, _ = product(emu, tmp_path, a, b, (8 * 33, 33, 1), 33, [], dtype)
    assert c.shape == (70, 33) and not c.any()


# ---- what cannot be checked without a read-back stays inside the operands ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("width", [np.int32, np.int64], ids=["i32", "i64"])
def test_rows_outside_the_operands_are_neither_read_nor_written(emu, tmp_path, dtype, width):
    """rows: a permutation with four entries replaced by -1, -3, M and M + 5.  The rows of c that no valid entry names keep their 0xCD, the
    others are right, grad_b has nothing from the four; a, g and c end at guard pages and start behind one."""
    seglen, k, n = EDGES, 17, 33
    m = sum(seglen)
    a, b, g = operands(m, k, n, len(seglen), 6)
    rows = torch.randperm(m, generator=torch.Generator().manual_seed(1)).tolist()
    for at, bad in zip((0, 40, 64, m - 1), (-1, -3, m, m + 5)):
        rows[at] = bad
    idx = row_types(seglen, m, rows)
    want = grouped_refs(a, b, g, idx)
    assert int((idx < 0).sum()) == 4
    c, read = product(emu, tmp_path, a, b, (k * n, n, 1), n, seglen, dtype, rows=rows, len_dtype=width, rows_dtype=width)
    raw = read("c", np.int16 if dtype == BF16 else np.int32).reshape(m, n)
    named = (idx >= 0).numpy()
    assert (raw[~named] == (CD16 if dtype == BF16 else CD32)).all(), "a row that no valid entry names was written"
    assert same(c[named], want[0][named], dtype == BF16)
    gw, _ = gradw(emu, tmp_path, a, g, seglen, dtype, rows=rows, len_dtype=width, rows_dtype=width)
    assert same(gw, want[2], False)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("seglen", [[40, 0, 30], [40, 50, 70], [-7, 1000, 5], [2 ** 40, 3, 3], [2 ** 62] * 3],
                         ids=["short", "long", "negative", "huge", "overflow"])
def test_wrong_seglen_stays_inside(emu, tmp_path, seglen, dtype):
    """M = 100 rows under lengths that do not sum to it: the guard pages are the check; covered rows are right, uncovered ones zeros,
    grad_b has the clamped segments' rows.  ("overflow": the lengths are clamped before they are summed -- unclamped, their int64 sum wraps.)"""
    m, k, n = 100, 40, 33
    a, b, g = operands(m, k, n, 3, 5)
    want = grouped_refs(a, b, g, row_types(seglen, m))
    c, _ = product(emu, tmp_path, a, b, (k * n, n, 1), n, seglen, dtype)
    assert same(c, want[0], dtype == BF16)
    gw, _ = gradw(emu, tmp_path, a, g, seglen, dtype)
    assert same(gw, want[2], False)


# ---- weight pack ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["to-bf16", "to-fp32"])
@pytest.mark.parametrize("bdtype", [BF16, F32], ids=["from-bf16", "from-fp32"])
@pytest.mark.parametrize("transposed", [False, True], ids=["w", "wT"])
def test_pack_is_in_fragment_order(emu, tmp_path, transposed, bdtype, dtype):
    """packed[r][k group][column tile][lane]: element e of lane (l32, half) is W_r[group * G + half * P + e][32 tile + l32], zero past K or
    N (the kernel's own comment), from either pair of strides and either source type; and the product on it is right."""
    R, k, n = 3, 23, 37
    P, G = (8, 16) if dtype == BF16 else (4, 8)
    a, b, g = operands(5, k, n, R, 8)
    store, strides = (b.transpose(1, 2).contiguous(), (k * n, 1, k)) if transposed else (b, (k * n, n, 1))
    c, read = product(emu, tmp_path, a, store, strides, n, [2, 0, 3], dtype, bdtype=bdtype)
    assert same(c, grouped_refs(a, b, g, row_types([2, 0, 3], 5))[0], dtype == BF16)
    groups, nt = sc.ceil_div(k, G), sc.ceil_div(n, 32)
    full = torch.zeros(R, groups * G, nt * 32, dtype=torch.float64)
    full[:, :k, :n] = b
    want = full.view(R, groups, 2, P, nt, 32).permute(0, 1, 4, 2, 5, 3).reshape(-1)          # r, group, tile, half, l32, e
    raw = torch.from_numpy(read("packed", np.int16 if dtype == BF16 else np.int32))
    assert torch.equal((raw.view(BF16) if dtype == BF16 else raw.view(F32)).double(), want)
