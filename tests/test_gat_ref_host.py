"""What test_gat_geometry_gpu.py stands on, checked without a GPU: the float64 reference (gat_ref.gat_reference) against the two
oracles that are pinned to the reference's fixtures, the sweep graph's degree lists, and -- through dgll_hip_debug_gat_choice, as
test_gat_choice_host.py does -- that the table of cases reaches every (lanes per row, heads per wavefront) geometry of gat2_kernel
for both dtypes, the in-row form, both finalize kernels and 8, 7 and 1 rows per wavefront.  Every expected value is a literal."""
import numpy as np
import pytest
import torch

import gat_ref
from gat_ref import ALL_PAIRS, BASE_CASES, BF16, CASES, EXTRA_CASES, F32, N_COLS, N_ROWS, case_id, gat_reference, gat_reference_grads
from test_gat_choice_host import COLS, FWD, GROUP, ROWS, WAVE, choose, form, geom, packed

NNZ = 6375                  # of the sweep graph
PASSES = ((FWD, 0), (ROWS, 3), (ROWS, 0), (COLS, 0))       # forward, rows pass with exact dd, with stored dd, transposed pass


# ------------------------------------------------------------------------------------------------ the reference against the oracles
def _small_graph(n=60, seed=3):
    gen = torch.Generator().manual_seed(seed)
    adj = (torch.rand(n, n, generator=gen) < 0.12) | torch.eye(n, dtype=torch.bool)
    adj[4, :40] = True                                   # one heavy row
    r, c = adj.nonzero(as_tuple=True)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    torch.cumsum(torch.bincount(r, minlength=n), 0, out=rowptr[1:])
    return rowptr, c.to(torch.int32), gen


def _block_diagonal(a, heads, fo):
    """A [heads * fo, 2 * heads] from spgat_conv's a [heads, 1, 2 fo], differentiably."""
    A = torch.zeros(heads * fo, 2 * heads, dtype=a.dtype)
    for k in range(heads):
        A[k * fo:(k + 1) * fo, k] = a[k, 0, :fo]
        A[k * fo:(k + 1) * fo, heads + k] = a[k, 0, fo:]
    return A


@pytest.mark.parametrize("heads,fo", [(1, 5), (3, 8)])
@pytest.mark.parametrize("concat", [True, False])
def test_reference_equals_torch_ref_spgat_conv_forward_and_gradients(heads, fo, concat):
    from oracle import torch_ref

    rowptr, col, gen = _small_graph()
    n, fin = rowptr.numel() - 1, 7
    x = torch.randn(n, fin, generator=gen)
    W = torch.randn(heads, fin, fo, generator=gen) * 0.4
    a = torch.randn(heads, 1, 2 * fo, generator=gen) * 0.4
    gout = torch.randn(n, heads * fo, generator=gen)

    def ours(dtype):
        xs, Ws, as_ = (v.to(dtype).requires_grad_() for v in (x, W, a))
        h = torch.cat([xs @ Ws[k] for k in range(heads)], 1)
        out = gat_reference(rowptr, col, h, None, None, heads, 0.2, concat, A=_block_diagonal(as_, heads, fo))
        return (out.detach(),) + torch.autograd.grad(out, (xs, Ws, as_), gout.to(dtype))

    def oracle(dtype):
        xs, Ws, as_ = (v.to(dtype).requires_grad_() for v in (x, W, a))
        out = torch_ref.spgat_conv(rowptr, col, xs, Ws, as_, 0.2, concat=concat)
        return (out.detach(),) + torch.autograd.grad(out, (xs, Ws, as_), gout.to(dtype))

    mine = ours(torch.float64)
    for got, want in zip(mine, oracle(torch.float64)):          # the same formula in the same precision
        torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-12)
    for got, want in zip(mine, oracle(torch.float32)):          # the oracle as its goldens pin it: to fp32 rounding
        torch.testing.assert_close(got.float(), want, rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("heads,fo", [(1, 5), (3, 8)])
@pytest.mark.parametrize("apply_elu", [True, False])
def test_reference_equals_the_c_oracle_forward(heads, fo, apply_elu):
    from oracle import cref

    rowptr, col, gen = _small_graph(seed=4)
    n = rowptr.numel() - 1
    h = torch.randn(n, heads * fo, generator=gen) * 0.5
    s, t = torch.randn(n, heads, generator=gen) * 0.5, torch.randn(n, heads, generator=gen) * 0.5
    want = cref.gat_fwd(rowptr.numpy(), col.numpy(), h.numpy(), s.numpy(), t.numpy(), heads, 0.2, apply_elu=apply_elu, mode=0)
    got = gat_reference(rowptr, col, h.double(), s.double(), t.double(), heads, 0.2, apply_elu)
    np.testing.assert_allclose(got.float().numpy(), want, rtol=2e-5, atol=2e-6)


# ------------------------------------------------------------------------------------------------ the sweep graph
def test_sweep_graph_degree_lists():
    rowptr, col = gat_ref.sweep_graph()
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and rowptr.numel() == N_ROWS + 1 == 532 and N_COLS == 760
    assert int(rowptr[-1]) == col.numel() == NNZ
    deg = (rowptr[1:] - rowptr[:-1]).tolist()
    assert {r: deg[r] for r in (0, 5, 6, 7, 40, 41, 42, 80, 81, 82, 120, 121, 122, 530)} == {
        0: 700, 5: 1, 6: 2, 7: 3, 40: 63, 41: 64, 42: 65, 80: 127, 81: 128, 82: 129, 120: 255, 121: 256, 122: 257, 530: 513}
    ordinary = [d for r, d in enumerate(deg) if r not in gat_ref.SPECIAL_ROWS]
    assert len(ordinary) == 517 and min(ordinary) == 3 and max(ordinary) == 12        # self-loop, column 5, [6], [7], 1 .. 8 random
    assert sum(d > 256 for d in deg) == 3                                             # the plan's long rows: 257, 513, 700
    colv = col.long()
    for r in range(N_ROWS):
        mine = colv[rowptr[r]:rowptr[r + 1]]
        assert bool((mine[1:] > mine[:-1]).all()) and r in mine and 5 in mine         # sorted, distinct, self-loop, the hub column
    indeg = torch.bincount(colv, minlength=N_COLS)
    assert (int(indeg[5]), int(indeg[6]), int(indeg[7])) == (531, 257, 256)
    assert sum(int(d) > 256 for d in indeg) == 2                                      # long rows of the transpose: columns 5 and 6
    assert int(indeg[750:].sum()) == 0 and int((indeg[:750] == 0).sum()) == 0         # ten columns >= 531 that no row references
    assert gat_ref.sweep_graph()[1] is col                                            # one builder, built once
    # not symmetric: the rows are the first 531 columns, and row 5 holds column 5 only while column 5 sits in every row
    assert int(rowptr[6] - rowptr[5]) == 1 and int(colv[rowptr[5]]) == 5


# ------------------------------------------------------------------------------------------------ what the table reaches
def test_the_table_is_the_one_written_down():
    assert len(BASE_CASES) == 38 and len(EXTRA_CASES) == 11 and len(set(c[:3] for c in CASES)) == 49
    assert [c[1:3] for c in BASE_CASES[:19]] == [(1, 4), (2, 4), (4, 4), (1, 20), (2, 12), (4, 8), (8, 4), (1, 36), (2, 20), (4, 12), (8, 8),
                                                 (1, 68), (2, 36), (4, 20), (8, 12), (1, 132), (2, 68), (4, 36), (8, 20)]
    assert all(c[0] == F32 for c in BASE_CASES[:19]) and all(c[0] == BF16 for c in BASE_CASES[19:])
    assert [(c[1], c[2]) for c in BASE_CASES[19:]] == [(c[1], 2 * c[2]) for c in BASE_CASES[:19]]
    assert [c[3:] for c in BASE_CASES[19:]] == [c[3:] for c in BASE_CASES[:19]]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_pass_of_a_case_gets_the_geometry_in_the_table(case):
    dtype, heads, fo, lpr, nh, grid_y = case
    for pass_, phase in PASSES:
        c = choose(pass_, dtype, heads, fo, phase=phase)
        assert c.generation == 2 and geom(c) == (lpr, nh, grid_y), (pass_, phase, c.generation, geom(c))
        assert c.kind == {(FWD, 0): 0, (ROWS, 3): 3, (ROWS, 0): 1, (COLS, 0): 2}[(pass_, phase)]
    # the forms the GPU test runs besides the compact one keep it: t_j from the gathered row; {s_i, dd_i} side by side for the
    # transposed pass, with and without the score-gradient epilogue; scores in the padding of 16-byte pitched rows
    pitch = (heads * fo * (2 if dtype == BF16 else 4) + 8 * heads + 15) // 16 * 4          # floats per padded row
    for c in (choose(FWD, dtype, heads, fo, rowscore=True), choose(ROWS, dtype, heads, fo, phase=3, rowscore=True, sd_out=True),
              choose(ROWS, dtype, heads, fo, phase=3, sd_out=True), choose(COLS, dtype, heads, fo, t_stride=2 * heads),
              choose(COLS, dtype, heads, fo, t_stride=2 * heads, epilogue=True),
              choose(FWD, dtype, heads, fo, t_stride=pitch, **packed(8 * heads)),
              choose(COLS, dtype, heads, fo, t_stride=pitch, epilogue=True, **packed(8 * heads))):
        assert c.generation == 2 and geom(c) == (lpr, nh, grid_y), geom(c)


def test_the_table_reaches_all_19_geometries_of_each_dtype():
    assert len(ALL_PAIRS) == 19
    for dtype in (F32, BF16):
        for cases in (BASE_CASES, CASES):
            for pass_, phase in PASSES:
                reached = sorted({geom(choose(pass_, dtype, heads, fo, phase=phase))[:2] for d, heads, fo, *_ in cases if d == dtype})
                assert reached == ALL_PAIRS, (dtype, pass_, phase, reached)
    # a base case leaves lanes of a head idle (the head's last vectors are masked) unless its heads are one or two vectors wide --
    # four such cases per dtype; none of the three "no idle lane" extras does
    full = [c[:3] for c in BASE_CASES if c[2] // (8 if c[0] == BF16 else 4) == c[3] // c[4]]
    assert full == [(F32, 4, 4), (F32, 4, 8), (F32, 8, 4), (F32, 8, 8), (BF16, 4, 8), (BF16, 4, 16), (BF16, 8, 8), (BF16, 8, 16)]
    for dtype, heads, fo, lpr, nh, _ in EXTRA_CASES[6:9]:
        assert fo // (8 if dtype == BF16 else 4) == lpr // nh


def test_one_head_in_the_row_padding_is_the_in_row_form():
    one_head = [c for c in BASE_CASES if c[1] == 1]
    assert len(one_head) == 10
    for dtype, heads, fo, *_ in one_head:
        for pass_, phase, kind in ((FWD, 0, 0), (ROWS, 3, 3), (ROWS, 0, 1), (COLS, 0, 2)):
            assert form(choose(pass_, dtype, 1, fo, phase=phase, **packed(8))) == (2, kind, 0, 0, 1)
    for pass_, phase, kind in ((FWD, 0, 0), (ROWS, 3, 3), (ROWS, 0, 1), (COLS, 0, 2)):
        assert form(choose(pass_, BF16, 1, 64, phase=phase, **packed(8))) == (2, kind, 0, 0, 0)      # packed, but no idle lane: not in-row
    for dtype, heads, fo, *_ in CASES:
        if heads > 1:
            assert choose(FWD, dtype, heads, fo, **packed(8 * heads)).inrow == 0


def test_finalize_kernel_and_rows_per_wavefront_on_the_sweep_graph():
    # (n_rows, n_chunks, n_long) of the plans: A has long rows of 700, 257 and 513 entries (3 + 2 + 3 chunks), its transpose of 531 and 257
    plans = {FWD: (531, 8, 3), ROWS: (531, 8, 3), COLS: (760, 5, 2)}
    rpw = {}
    for dtype, heads, fo, *_ in CASES:
        for pass_, phase in PASSES:
            n_rows, n_chunks, n_long = plans[pass_]
            c = choose(pass_, dtype, heads, fo, phase=phase, plan=True, n_rows=n_rows, nnz=NNZ, n_chunks=n_chunks, n_long=n_long)
            assert c.finalize == (GROUP if heads == 72 else WAVE), (dtype, heads, fo, pass_)
            assert c.chunk_blocks == 2                                   # 8 and 5 chunk items, four per block
            rpw[(dtype, heads, fo, pass_, phase)] = c.rows_per_wave
    assert sum(c[1] == 72 for c in CASES) == 1
    # 98304 bytes over (6375 / 531 = 12.006 entries) x (the row's bytes): 640 B -> 12 -> 8; 1152 B -> 7; 5120 B -> 1; 2048 B -> 3
    for pass_, phase in PASSES[:3]:
        assert rpw[(F32, 8, 20, pass_, phase)] == 8
        assert rpw[(F32, 72, 4, pass_, phase)] == 7
        assert rpw[(F32, 5, 256, pass_, phase)] == 1
        assert rpw[(F32, 2, 256, pass_, phase)] == 3
    # the transposed pass: 6375 / 760 = 8.388 entries: 1152 B -> 10 -> 8; 5120 B -> 2; 2048 B -> 5
    assert (rpw[(F32, 72, 4, COLS, 0)], rpw[(F32, 5, 256, COLS, 0)], rpw[(F32, 2, 256, COLS, 0)]) == (8, 2, 5)
    assert {1, 7, 8} <= set(rpw.values())


# ------------------------------------------------------------------------------------------------ the bars
@pytest.mark.parametrize("case", [c for c in CASES if c[0] == BF16], ids=case_id)
def test_bf16_rounding_of_the_reference_is_inside_the_forward_bound(case):
    """The derived bf16 bound of the compact-score forward, |got - ref| <= 2^-8 |ref| + 1e-4 max|ref|, holds for the float64 reference
    stored with round-to-nearest-even: the reference alone stays inside it, with the whole second term to spare."""
    for apply_elu in (True, False):
        ref = gat_ref.case_reference(case, apply_elu, False)["out"]
        rounded = ref.to(torch.bfloat16)
        assert gat_ref.check("out", rounded, ref, torch.bfloat16, form_a=True) == []
        assert bool(((rounded.double() - ref).abs() <= 2.0 ** -8 * ref.abs()).all())


def test_the_fp32_bars_see_one_dropped_edge():
    """The last entry of the 257-entry row dropped for ONE head of a four-head case: the fp32 forward and grad_h bars reject the
    perturbed reference held against the true one (and pass the true one against itself)."""
    case = (F32, 4, 8, 8, 4, 1)
    assert case in CASES
    rowptr, col = gat_ref.sweep_graph()
    x = gat_ref.case_inputs(case)
    true = gat_ref.case_reference(case, True, False)
    row, head, fo = 122, 2, 8
    assert int(rowptr[row + 1] - rowptr[row]) == 257
    cut = int(rowptr[row + 1]) - 1
    rowptr2 = rowptr.clone()
    rowptr2[row + 1:] -= 1
    col2 = torch.cat([col[:cut], col[cut + 1:]])
    without = gat_reference_grads(rowptr2, col2, x["h"], x["s"], x["t"], 4, 0.2, True, x["gout"])
    wrong = {k: v.clone() for k, v in true.items()}
    cols = slice(head * fo, (head + 1) * fo)
    wrong["out"][:, cols] = without["out"][:, cols]
    wrong["grad_h"][:, cols] = without["grad_h"][:, cols]
    assert int((wrong["out"] != true["out"]).any(1).sum()) == 1                      # one output row, one head of it
    for name in ("out", "grad_h"):
        assert gat_ref.check(name, true[name].float(), true[name], torch.float32) == []
        assert gat_ref.check(name, wrong[name].float(), true[name], torch.float32) != [], name
