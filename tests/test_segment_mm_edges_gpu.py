"""The branches of csrc/segment_mm.hip and dgll_amd/ops_segmm.py that tests/test_segment_mm_gpu.py does not reach, at the smallest shapes
that reach them: segment ranges (_PACK_BYTES), the plan kernel past 256 entries, weight-gradient slabs above M = 65 536, keep_first at a
ragged K, the weight gradient's k-tile edges, int32 index vectors and the documented contracts.  GPU box only (-m gpu).

The legs, comparators and bars are those of test_segment_mm_gpu.py (tests/segmm_cases.py): integers in [-2, 2] must EQUAL the float64
result as stored; bf16-rounded randn at the project's bars, f32_random_ok given S = ceil(longest segment / 512) for grad_b (slabs hold
512 rows at the least).  Every forward runs into a sentinel buffer with spare rows and a wider pitch, from an `a` with NaN behind column
K; a second run must give the same bits."""
import pytest
import torch

import dense_small_cases as sc
from segmm_cases import DTYPES, EDGES, SHORT, SLAB, check, operands, problems, run
from segmm_ref import grouped_refs, segment_ids

pytestmark = pytest.mark.gpu

DT_IDS = ["bf16", "fp32"]
OPS = ["segment", "gather"]


def grouping_of(op, seglen, device, shift=0):
    """(float64-reference type of every row, the operator's grouping argument); gather: the types in a fixed random order"""
    idx = segment_ids(seglen)
    if op == "gather":
        idx = idx[torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(7))] + shift
        return idx, idx.to(device)
    return idx, torch.tensor(seglen, device=device)


def both_legs(op, seglen, k, n, dtype, device, extra=0, kinds=("forward", "grad_a", "grad_b"), random_kinds=None, tag=""):
    """Both legs of one case against float64, the sentinels, and a second run's bits -> [(buf, grad_a, grad_b)] per leg"""
    idx, grouping = grouping_of(op, seglen, device)
    m = idx.numel()
    slabs = sc.ceil_div(max(max(seglen), 1), 512)
    out = []
    for exact in (True, False):
        a, b, g = operands(seglen, k, n, extra, exact, dtype == torch.bfloat16, 11 + exact)
        buf, ga, gb = run(op, a, b, g, grouping, dtype, device)
        name = "%s%s %s k%d n%d exact=%d" % (tag, op, dtype, k, n, exact)
        for got, p, kind in zip((buf[:m, :n], ga, gb), problems(a, b, g, idx), ("forward", "grad_a", "grad_b")):
            if kind in (kinds if exact or random_kinds is None else random_kinds):
                check(name, got, p, exact, dtype, kind, slabs=slabs)
        empty = torch.bincount(idx, minlength=b.shape[0]) == 0
        assert not gb[empty.to(device)].any(), (name, "grad_b of an empty segment is not exactly zero")
        assert sc.outside_untouched(buf, m, n), (name, "written outside [M, N]")
        again = run(op, a, b, g, grouping, dtype, device)
        assert all(torch.equal(x, y) for x, y in zip((buf, ga, gb), again)), (name, "two runs differ")
        out.append((buf, ga, gb))
    return out


# ---- 1. segment ranges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("k, n", [(40, 33), (64, 300)])
@pytest.mark.parametrize("seglen", [EDGES, SHORT], ids=["edges", "short"])
def test_segment_ranges(cuda_device, monkeypatch, seglen, k, n, op, dtype):
    """_PACK_BYTES = 1: one segment per range; three packed matrices: ranges of three segments, the last one short (N = 300: the range loop
    inside the 256-column loop).  Each against float64 on both legs and bit for bit the result at the default _PACK_BYTES."""
    from dgll_amd import _lib, ops_segmm

    extra = 3 if op == "gather" else 0
    whole = both_legs(op, seglen, k, n, dtype, cuda_device, extra)
    three = 3 * int(_lib.lib.dgll_hip_segment_mm_packed_bytes(1, k, min(n, 256), ops_segmm._code(dtype)))
    for pack_bytes in (1, three):
        monkeypatch.setattr(ops_segmm, "_PACK_BYTES", pack_bytes)
        parts = both_legs(op, seglen, k, n, dtype, cuda_device, extra, tag="_PACK_BYTES=%d " % pack_bytes)
        assert all(torch.equal(x, y) for u, v in zip(whole, parts) for x, y in zip(u, v)), ("differs from the one-range result", pack_bytes)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("seglen", [[40, 0, 30], [40, 50, 70]], ids=["short", "long"])
def test_wrong_device_seglen_in_ranges(cuda_device, monkeypatch, seglen, dtype):
    """test_wrong_device_seglen_stays_inside with one segment per range and two column blocks: only the launches with seg_begin == 0 zero
    the rows that no segment covers -- in all 300 columns -- covered rows are right, nothing outside c is written."""
    from dgll_amd import ops_segmm

    monkeypatch.setattr(ops_segmm, "_PACK_BYTES", 1)
    m, k, n = 100, 40, 300
    a, b, g = operands([m, 0, 0], k, n, 0, True, True, 5)
    idx = segment_ids(seglen)[:m]
    idx = torch.cat((idx, torch.full((m - idx.numel(),), -1)))                 # uncovered rows: no type
    ref = grouped_refs(a, b, g, idx)[0]
    buf = sc.sentinel_buffer(m + 3, n + 5, dtype, cuda_device)
    ad = sc.padded(a, cuda_device, dtype, sc.bf16_pitch(k), spare_rows=2)
    ops_segmm._product_raw(ad, b.to(device=cuda_device, dtype=dtype), torch.tensor(seglen, device=cuda_device), None, False, out=buf[:m, :n])
    assert sc.exact_ok(buf[:m, :n], ref, bf16_out=dtype == torch.bfloat16)
    assert not buf[:m, :n][(idx < 0).to(cuda_device)].any()
    assert sc.outside_untouched(buf, m, n)


# ---- 2. long type lists ----------------------------------------------------------------------------------------------------------------------
def _long_lists(R):
    cycle = [0, 1, 33, 2, 0, 0, 5]
    return {"cycle": [cycle[i % 7] for i in range(R)], "last": [0] * (R - 1) + [70], "first": [70] + [0] * (R - 1)}


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("R", [255, 256, 257, 700])
def test_long_type_lists(cuda_device, R, op, dtype):
    """R + 1 plan entries around and past the 256 threads of the plan kernel (per = 1, 2, 2, 3 segments per thread, idle threads at the
    end); gather: three trailing types that never occur.  grad_b of every empty segment is exactly zero."""
    for name, seglen in _long_lists(R).items():
        both_legs(op, seglen, 8, 8, dtype, cuda_device, 3 if op == "gather" else 0, tag=name + " ")


# ---- 3. weight-gradient slabs above M = 65 536 -----------------------------------------------------------------------------------------------
BIG_M = 70000                                                    # slab = ceil(70000 / 128) = 547 rounded up to 16: 560
BIG = [1700, 0, 560, 561, 1120, 1121] + [561] * 110
BIG = BIG + [BIG_M - sum(BIG)]                                   # (3228 rows: six slabs)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("op, k, n", [("segment", 8, 8), ("gather", 8, 8), ("segment", 136, 8)])
def test_large_m_slabs(cuda_device, op, k, n, dtype):
    """Segments of exactly one and two slabs of 560 rows, of one row more, of four and six slabs, and 110 of slab + 1 rows that fill the
    partial slots; K = 136: a second k block next to them.  grad_b on both legs, forward and grad_a on the exact leg."""
    assert sum(BIG) == BIG_M and min(BIG) >= 0
    both_legs(op, BIG, k, n, dtype, cuda_device, random_kinds=("grad_b",))


# ---- 4. ragged K, k-tile edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("k", [1, 3, 13, 17, 23, 29])
def test_ragged_k(cuda_device, k, op, dtype):
    """K no multiple of 4: keep_first masks an odd count (bf16: inside a 32-bit word) of a vector whose other elements are NaN"""
    both_legs(op, EDGES, k, 33, dtype, cuda_device, 3 if op == "gather" else 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("k", [97, 129])
def test_gradw_k_tile_edges(cuda_device, k, op, dtype):
    """K = 97: wave 3 owns one column; K = 129: a second k block holding one column; next to a two-slab segment"""
    both_legs(op, SLAB, k, 7, dtype, cuda_device, 3 if op == "gather" else 0)


# ---- 5. int32 index vectors ------------------------------------------------------------------------------------------------------------------
def _op_results(op, ad, bd, gd, grouping):
    from dgll_amd import ops_segmm

    ad, bd = ad.detach().clone().requires_grad_(True), bd.detach().clone().requires_grad_(True)
    c = ops_segmm.gather_mm(ad, bd, idx_b=grouping) if op == "gather" else ops_segmm.segment_mm(ad, bd, grouping)
    c.backward(gd)
    return c.detach(), ad.grad, bd.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("op", OPS)
def test_int32_indices_equal_int64(cuda_device, op, dtype):
    """an int32 device seglen_a / idx_b through the operators, an int32 `rows` through the raw launches: the bits of the int64 run, and
    (the int64 run) float64 on the exact leg"""
    from dgll_amd import ops_segmm

    k, n = 23, 33
    idx, grouping = grouping_of(op, EDGES, cuda_device)
    a, b, g = operands(EDGES, k, n, 0, True, True, 3)
    ad, bd, gd = a.to(cuda_device, dtype), b.to(cuda_device, torch.float32), g.to(cuda_device, dtype)
    wide = _op_results(op, ad, bd, gd, grouping)
    narrow = _op_results(op, ad, bd, gd, grouping.to(torch.int32))
    for got, p, kind in zip(wide, problems(a, b, g, idx), ("forward", "grad_a", "grad_b")):
        check("int64 %s %s" % (op, dtype), got, p, True, dtype, kind)
    assert all(torch.equal(x, y) for x, y in zip(wide, narrow))
    if op == "gather":
        ids, rows = torch.sort(grouping, stable=True)
        seglen = torch.bincount(ids, minlength=len(EDGES))
        a16, g16 = ops_segmm._rows16(ad), ops_segmm._rows16(gd)
        for rows_n, seglen_n in ((rows.to(torch.int32), seglen), (rows.to(torch.int32), seglen.to(torch.int32))):
            assert torch.equal(ops_segmm._product_raw(a16, bd, seglen_n, rows_n, False), wide[0])
            assert torch.equal(ops_segmm._gradw_raw(a16, g16, seglen_n, rows_n, len(EDGES)), wide[2])


# ---- 6. documented contracts -----------------------------------------------------------------------------------------------------------------
def _interior(x, device, dtype, pitch, fill):
    """x as rows [8, 8 + M) of a larger `fill`-filled allocation on `pitch`: an access a few rows outside stays inside allocated memory"""
    store = torch.full((x.shape[0] + 16, pitch), fill, dtype=dtype, device=device)
    view = store[8:8 + x.shape[0], :x.shape[1]]
    view.copy_(x)
    return store, view


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("width", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_rows_outside_the_operands(cuda_device, width, dtype):
    """rows: a permutation with four entries replaced by -1, -3, M and M + 5.  Their rows of c keep the sentinel (as do the 8 spare rows
    on either side of c), every other row is right, grad_b has nothing from them."""
    from dgll_amd import ops_segmm

    k, n, m = 23, 33, sum(EDGES)
    a, b, g = operands(EDGES, k, n, 0, True, True, 6)
    rows = torch.randperm(m, generator=torch.Generator().manual_seed(1))
    for at, bad in zip((0, 40, 64, m - 1), (-1, -3, m, m + 5)):
        rows[at] = bad
    idx = torch.full((m,), -1, dtype=torch.int64)
    ok = (rows >= 0) & (rows < m)
    idx[rows[ok]] = segment_ids(EDGES)[ok]
    assert int((idx < 0).sum()) == 4
    want = grouped_refs(a, b, g, idx)
    _, ad = _interior(a, cuda_device, dtype, 64, sc.NAN)
    _, gd = _interior(g, cuda_device, dtype, 64, sc.NAN)
    c_store, c = _interior(torch.full((m, n), sc.SENTINEL), cuda_device, dtype, 64, sc.SENTINEL)
    seglen, rows_d = torch.tensor(EDGES, device=cuda_device, dtype=width), rows.to(cuda_device, width)
    bd = b.to(cuda_device, dtype)
    ops_segmm._product_raw(ad, bd, seglen, rows_d, False, out=c)
    named = (idx >= 0).to(cuda_device)
    assert bool((c[~named] == sc.SENTINEL).all()), "a row that no valid entry names was written"
    assert sc.exact_ok(c[named], want[0][idx >= 0], bf16_out=dtype == torch.bfloat16)
    assert bool((c_store[:8] == sc.SENTINEL).all()) and bool((c_store[8 + m:] == sc.SENTINEL).all()) and bool((c_store[:, n:] == sc.SENTINEL).all())
    assert sc.exact_ok(ops_segmm._gradw_raw(ad, gd, seglen, rows_d, len(EDGES)), want[2])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_gather_mm_clamps_types(cuda_device, dtype):
    """idx_b at -5 and R + 3: b[0] and b[R - 1], as documented"""
    from dgll_amd import ops_segmm

    k, n, R = 23, 33, len(EDGES)
    idx, _ = grouping_of("gather", EDGES, cuda_device)
    a, b, g = operands(EDGES, k, n, 0, True, True, 8)
    wild = idx.clone()
    wild[::9], wild[4::9] = -5, R + 3
    ad, bd, gd = a.to(cuda_device, dtype), b.to(cuda_device, torch.float32), g.to(cuda_device, dtype)
    for got, p, kind in zip(_op_results("gather", ad, bd, gd, wild.to(cuda_device)), problems(a, b, g, wild.clamp(0, R - 1)),
                            ("forward", "grad_a", "grad_b")):
        check("clamped types %s" % dtype, got, p, True, dtype, kind)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("layout", ["transposed", "strided"])
def test_non_contiguous_b(cuda_device, layout, op, dtype):
    """b = leaf.transpose(1, 2) of an [R, N, K] leaf, and b = leaf[:, :, ::2] of an [R, K, 2 N] one: packed from their strides, forward
    and gradients on both legs, the gradient arriving on the leaf (zeros in the columns the slice skips)."""
    from dgll_amd import ops_segmm

    k, n = 40, 33
    idx, grouping = grouping_of(op, EDGES, cuda_device)
    for exact in (True, False):
        a, b, g = operands(EDGES, k, n, 0, exact, dtype == torch.bfloat16, 21 + exact)
        if layout == "transposed":
            leaf = b.transpose(1, 2).contiguous().to(cuda_device, torch.float32).requires_grad_(True)
            bd = leaf.transpose(1, 2)
        else:
            leaf = torch.full((len(EDGES), k, 2 * n), sc.NAN)
            leaf[:, :, ::2] = b.float()
            leaf = leaf.to(cuda_device).requires_grad_(True)
            bd = leaf[:, :, ::2]
        assert not bd.is_contiguous()
        ad = a.to(cuda_device, dtype).requires_grad_(True)
        c = ops_segmm.gather_mm(ad, bd, idx_b=grouping) if op == "gather" else ops_segmm.segment_mm(ad, bd, grouping)
        c.backward(g.to(cuda_device, dtype))
        gb = leaf.grad.transpose(1, 2) if layout == "transposed" else leaf.grad[:, :, ::2]
        for got, p, kind in zip((c.detach(), ad.grad, gb), problems(a, b, g, idx), ("forward", "grad_a", "grad_b")):
            check("%s b %s %s exact=%d" % (layout, op, dtype, exact), got, p, exact, dtype, kind, slabs=1)
        if layout == "strided":
            assert not leaf.grad[:, :, 1::2].any()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("op", OPS)
def test_bf16_b_through_autograd(cuda_device, op, dtype):
    """a bf16 b with requires_grad: the forward of the fp32 parameter holding the same values, grad_b its fp32 gradient rounded to bf16"""
    k, n = 40, 33
    _, grouping = grouping_of(op, SLAB, cuda_device)
    a, b, g = operands(SLAB, k, n, 0, False, True, 31)
    ad, gd = a.to(cuda_device, dtype), g.to(cuda_device, dtype)
    c32, ga32, gb32 = _op_results(op, ad, b.to(cuda_device, torch.float32), gd, grouping)
    c16, ga16, gb16 = _op_results(op, ad, b.to(cuda_device, torch.bfloat16), gd, grouping)
    assert gb16.dtype == torch.bfloat16 and torch.equal(gb16, gb32.to(torch.bfloat16))
    assert torch.equal(c16, c32) and torch.equal(ga16, ga32)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("op", OPS)
def test_no_rows(cuda_device, op, dtype):
    """M = 0 with R = 3: an empty c, a grad_b of exact zeros"""
    from dgll_amd import ops_segmm

    ad = torch.zeros((0, 40), dtype=dtype, device=cuda_device, requires_grad=True)
    bd = torch.randn(3, 40, 33, device=cuda_device).requires_grad_(True)
    if op == "gather":
        c = ops_segmm.gather_mm(ad, bd, idx_b=torch.zeros(0, dtype=torch.int64, device=cuda_device))
    else:
        c = ops_segmm.segment_mm(ad, bd, torch.zeros(3, dtype=torch.int64, device=cuda_device))
    assert c.shape == (0, 33) and c.dtype == dtype
    c.backward(torch.zeros_like(c))
    assert bd.grad.shape == bd.shape and bool(torch.isfinite(bd.grad).all()) and not bd.grad.any()
    assert ad.grad.shape == ad.shape


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [33, 64, 300])
def test_misaligned_c(cuda_device, n, dtype):
    """out = buf[:m, 1:1 + n] on a pitch that is a multiple of 4: the base is not 8 / 16-byte aligned while the pitch is, so every store is
    scalar.  The bits of the aligned run; column 0, the columns behind and the spare rows keep the sentinel."""
    from dgll_amd import ops_segmm

    k, m = 40, sum(EDGES)
    a, b, g = operands(EDGES, k, n, 0, False, dtype == torch.bfloat16, 41)
    ad = sc.padded(a, cuda_device, dtype, sc.bf16_pitch(k), spare_rows=2)
    bd, seglen = b.to(cuda_device, torch.float32), torch.tensor(EDGES, device=cuda_device)
    aligned = ops_segmm._product_raw(ad, bd, seglen, None, False)
    check("aligned %s n%d exact=0" % (dtype, n), aligned, problems(a, b, g, segment_ids(EDGES))[0], False, dtype, "forward")
    buf = sc.sentinel_buffer(m + 3, sc.round_up(n + 1, 4) + 4, dtype, cuda_device)
    ops_segmm._product_raw(ad, bd, seglen, None, False, out=buf[:m, 1:1 + n])
    assert torch.equal(buf[:m, 1:1 + n], aligned)
    assert bool((buf[m:] == sc.SENTINEL).all()) and bool((buf[:, 0] == sc.SENTINEL).all()) and bool((buf[:, 1 + n:] == sc.SENTINEL).all())
