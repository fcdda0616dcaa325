"""rowtile_ref.py without a GPU: the sweep graph and its transpose have the rows the module text names; the literal table is what
make_head_geometry gives (the Python restatement and the C++ itself, compiled from the unmodified csrc/row_tiles.hpp) and reaches all
22 (lph, lpr) pairs per dtype with every idle-lane condition; the closed-form legs' premises hold on the data in float64; the
edge-by-edge references agree with autograd; and the comparators reject, on the reference arrays alone, the faults they exist for."""
import subprocess

import numpy as np
import pytest
import torch

import rowtile_ref as R
from attn_ref import sparse_attention_reference
from kernel_emu import build_emulator
from rowtile_ref import BF16, CASES, F32, LONG_ROW
from test_gatv2_host import gatv2_reference

BY_ID = {R.case_id(c): c for c in CASES}
SMALL = [BY_ID["fp32-8x8"], BY_ID["bf16-3x16"], BY_ID["fp32-2x12"]]          # two vectors a head and more than one head; idle lanes


# ---- the graph ---------------------------------------------------------------------------------------------------------------------
def test_sweep_graph_has_the_rows_it_names():
    g = R.sweep_graph()
    assert (g.n_rows, g.n_cols) == (307, 760) and g.n_rows % 4 != 0
    assert g.deg[0] == 0 and g.deg[-1] == 0
    for n in R.SPECIAL:
        row = g.rows[g.special[n]]
        assert len(row) == n and len(set(row)) == n, n
    for groups in (4, 8, 16, 32):
        assert R.tile_has_pattern(g, groups), groups
        assert g.n_rows % groups != 0
    long_rows = [r for r in range(g.n_rows) if g.deg[r] > LONG_ROW]
    assert sorted(g.deg[long_rows]) == [257, 511, 512, 513, 700]
    assert any(a // 32 == b // 32 for a in long_rows for b in long_rows if a < b)           # two long rows in one tile at lpr = 8
    assert not any(a // 4 == b // 4 for a in long_rows for b in long_rows if a < b)
    # every row but the one with a repeated column has distinct columns
    repeated = [r for r in range(g.n_rows) if len(set(g.rows[r])) != len(g.rows[r])]
    assert repeated == [g.dup_row] and g.rows[g.dup_row].count(g.dup_col) == 5
    assert len(set(g.rows[g.dup_row])) == len(g.rows[g.dup_row]) - 4
    for n in R.WINNER_LAST:
        assert g.rows[g.special[n]][-1] == max(g.rows[g.special[n]])
    for n in R.WINNER_FIRST:
        assert g.rows[g.special[n]][0] == max(g.rows[g.special[n]])
    assert all(0 <= c < g.n_cols for r in g.rows for c in r)


def test_transposed_sweep_graph_meets_long_rows_and_the_threshold():
    g = R.sweep_graph()
    t = g.transposed_rows()
    indeg = np.array([len(r) for r in t])
    assert np.array_equal(indeg, g.indeg) and indeg.sum() == g.nnz
    assert int((indeg > LONG_ROW).sum()) >= 2 and int((indeg == LONG_ROW).sum()) == 1
    assert indeg[R.HUBS[1]] == LONG_ROW + 1 and indeg[R.HUBS[2]] == LONG_ROW
    assert sorted(np.flatnonzero(indeg == 0)) == sorted(R.UNREFERENCED) and len(R.UNREFERENCED) == 10
    assert g.n_cols % 32 != 0 and g.n_cols % 16 != 0                        # 760 = 32 * 23 + 24: a ragged last tile at 16 and 32 rows
    # the library's transpose is this one
    gt, _ = g.csr().transpose()
    assert gt.n_rows == g.n_cols and np.array_equal((gt.rowptr[1:] - gt.rowptr[:-1]).numpy(), indeg)
    assert [int(c) for c in gt.col] == [i for r in t for i in r]


def test_emulator_graph():
    g = R.emu_graph()
    assert sorted(g.deg) == sorted((0, 0) + R.EMU_SPECIAL) and g.deg[0] == 0 and g.deg[-1] == 0
    assert all(len(set(r)) == len(r) for r in g.rows)
    assert sorted(np.flatnonzero(g.indeg == 0)) == sorted(g.unreferenced)
    for n in (9, 65, 257):
        assert g.rows[g.special[n]][-1] == max(g.rows[g.special[n]])
    assert g.rows[g.special[255]][0] == max(g.rows[g.special[255]])


# ---- the table ---------------------------------------------------------------------------------------------------------------------
PAIRS = [(lph, lpr) for lph in (1, 2, 4, 8, 16, 32, 64) for lpr in (8, 16, 32, 64) if lpr >= lph]


def test_table_is_what_the_restated_geometry_gives():
    assert len(PAIRS) == 22 and len(CASES) == 50
    for c in CASES:
        geo, tiles = R.head_geometry(c.heads, c.D, R.epv(c.dtype), R.N_ROWS)
        assert geo == c.geo, (R.case_id(c), geo)
        assert c.D == c.geo.vph * R.epv(c.dtype) and tiles == -(-R.N_ROWS // (256 // c.geo.lpr))
    assert len(set(BY_ID)) == 50


def test_table_is_what_row_tiles_hpp_gives(tmp_path_factory):
    exe = build_emulator(tmp_path_factory, "row_tiles.hpp", "geometry_main.cpp")
    args = [str(v) for c in CASES for n in (R.N_ROWS, R.N_COLS) for v in (c.heads, c.D, R.epv(c.dtype), n)]
    res = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    lines = [tuple(int(v) for v in ln.split()) for ln in res.stdout.splitlines()]
    assert len(lines) == 2 * len(CASES)
    for k, c in enumerate(CASES):
        for n, line in ((R.N_ROWS, lines[2 * k]), (R.N_COLS, lines[2 * k + 1])):
            tiles = -(-n // (256 // c.geo.lpr))
            assert line == tuple(c.geo) + (tiles, tiles), (R.case_id(c), n, line)


def test_flat_geometry_is_the_formula(tmp_path_factory):
    """make_flat_geometry (the passes whose rows are F columns without heads: typed SpMM, PNA, edge features) against its formula
    restated: vpr below, at and above the lane-width steps and the 64-lane cap, with no rows, one row and a ragged last tile."""
    exe = build_emulator(tmp_path_factory, "row_tiles.hpp", "geometry_main.cpp")
    cases = [(vpr, n_rows) for vpr in (1, 6, 8, 9, 33, 64, 65, 130) for n_rows in (0, 1, 33)]
    res = subprocess.run([exe, "flat"] + [str(v) for c in cases for v in c], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    lines = [tuple(int(v) for v in ln.split()) for ln in res.stdout.splitlines()]
    assert len(lines) == len(cases)
    for (vpr, n_rows), line in zip(cases, lines):
        lpr = 8
        while lpr < min(vpr, 64):
            lpr *= 2
        groups = 4 * 64 // lpr
        tiles = -(-n_rows // groups)
        assert line == (lpr, -(-vpr // lpr), tiles, min(tiles, 2 ** 22)), (vpr, n_rows, line)


def test_table_reaches_every_pair_and_condition():
    for dt in (F32, BF16):
        cases = [c for c in CASES if c.dtype == dt]
        base = cases[:22]
        assert [(c.geo.lph, c.geo.lpr) for c in base] == PAIRS and all(c.geo.col_blocks == 1 for c in base)
        assert {(c.geo.lph, c.geo.lpr) for c in cases} == set(PAIRS)
        assert any(c.geo.vph < c.geo.lph for c in cases)                                    # idle lanes inside a head
        assert any(c.geo.hpb * c.geo.lph < c.geo.lpr for c in cases)                        # idle lanes after the last head
        assert any(c.heads % c.geo.hpb != 0 for c in cases)                                 # a ragged last column block
        assert {c.geo.col_blocks for c in cases} == {1, 2, 3}
        # (c) of the mutation checks: heads < 64 / lph with lanes idling after the last head
        assert any(c.heads < 64 // c.geo.lph and c.geo.hpb * c.geo.lph < c.geo.lpr for c in cases)
        partials = -(-R.N_ROWS // 16)                                                       # workgroups of the GATv2 rows pass
        tiles = {-(-R.N_ROWS // (256 // c.geo.lpr)) for c in cases}
        assert min(tiles) < partials < max(tiles) and tiles == {10, 20, 39, 77}
        assert max(c.heads * c.D * (4 if dt == F32 else 2) for c in cases) == 3072


def test_several_column_blocks_mean_full_lane_rows():
    """Over every shape the passes accept: a launch with more than one column block has hpb = 64 / lph whole heads in each (hpb is
    the smaller of 64 / lph and heads, and heads > hpb), and a launch with lanes idling after the last head has one column block.
    So `blockIdx.y * hpb` and `blockIdx.y * (64 / lph)` address the same head in every launch make_head_geometry can produce: the
    head decode cannot be told from that variant by any test (CHANGELOG: mutation (c))."""
    for vph in range(1, 65):
        for heads in range(1, 140):
            geo, _ = R.head_geometry(heads, vph * 4, 4, R.N_ROWS)
            if geo.col_blocks > 1:
                assert geo.hpb == 64 // geo.lph and geo.hpb * geo.lph == geo.lpr == 64
            else:
                assert geo.hpb == heads


# ---- the legs' premises ------------------------------------------------------------------------------------------------------------
def _exact_in(t, dtype):
    return torch.equal(t.double(), t.double().to(dtype).double())


@pytest.mark.parametrize("case", [BY_ID["fp32-8x8"], BY_ID["bf16-3x16"], BY_ID["bf16-3x512"], BY_ID["fp32-1x132"], BY_ID["bf16-64x8"]],
                         ids=R.case_id)
def test_flat_leg_premises(case):
    g = R.sweep_graph()
    q, k, v, gr, scale = R.attn_operands(g, case, "flat")
    ref = R.attn_reference(g, q, k, v, gr, case.heads, scale)
    s, alpha = ref["s"], ref["alpha"]
    n = g.n_rows
    lo = torch.full((n, case.heads), float("inf"), dtype=torch.float64).scatter_reduce(0, g.row.unsqueeze(1).expand_as(s), s, "amin")
    hi = torch.full((n, case.heads), -float("inf"), dtype=torch.float64).scatter_reduce(0, g.row.unsqueeze(1).expand_as(s), s, "amax")
    live = torch.from_numpy(g.deg > 0)
    assert torch.equal(lo[live], hi[live]) and hi[live].abs().max().item() <= 8 and hi[live].abs().min().item() > 0
    assert torch.equal(s, s.float().double()) and scale == 0.125                            # exactly representable, a power of two
    assert torch.equal(alpha, (1.0 / torch.from_numpy(g.deg).double())[g.row].unsqueeze(1).expand_as(alpha))
    q3 = q.double().view(n, case.heads, case.D)
    assert torch.equal(q3, q3[:, :, :1].expand_as(q3)) and bool((q3 != 0).all())
    assert len(torch.unique(q3[:, :, 0])) >= 4                                              # c_ih differs by row and head
    ksum = k.double().view(-1, case.heads, case.D).sum(-1)
    assert torch.equal(ksum, ksum[:1].expand_as(ksum)) and bool((ksum != 0).all())
    assert bool((v != 0).all()) and bool((gr != 0).all()) and v.double().abs().max().item() <= 4
    for t in (q, k, v, gr):
        assert _exact_in(t, BF16) and torch.equal(t.double(), t.double().round())
    # the degenerate form: q = 0, same k
    q0, k0, _, _, _ = R.attn_operands(g, case, "zero")
    assert q0.abs().max().item() == 0.0 and k0.double().view(-1, case.heads, case.D).sum(-1).min().item() > 0
    # GATv2: flat in both regimes of the leaky ReLU
    xl, xr, attn, gg, slope = R.gatv2_operands(g, case, "flat")
    r2 = R.gatv2_reference(g, xl, xr, attn, gg, case.heads, slope)
    s2 = r2["s"]
    lo = torch.full((n, case.heads), float("inf"), dtype=torch.float64).scatter_reduce(0, g.row.unsqueeze(1).expand_as(s2), s2, "amin")
    hi = torch.full((n, case.heads), -float("inf"), dtype=torch.float64).scatter_reduce(0, g.row.unsqueeze(1).expand_as(s2), s2, "amax")
    assert torch.equal(lo[live], hi[live]) and hi[live].abs().max().item() <= 8 and slope == 0.25
    assert torch.equal(s2, s2.float().double())
    z = xl.double()[g.col.long()] + xr.double()[g.row]
    even = (g.row % 2 == 0)
    assert bool((z[even] > 0).all()) and bool((z[~even] < 0).all())
    assert bool((xl.double() >= 0).all()) and xr.double()[1::2].max().item() <= -(xl.double().max().item() + 1)
    a = attn.double()
    assert torch.equal(a, a[:, :1].expand_as(a)) and torch.equal(torch.log2(a), torch.log2(a).round())
    for t in (xl, xr, gg):
        assert _exact_in(t, BF16) and torch.equal(t.double(), t.double().round())
    assert R.gatv2_operands(g, case, "zero")[2].abs().max().item() == 0.0


@pytest.mark.parametrize("case", [BY_ID["fp32-8x8"], BY_ID["bf16-3x16"], BY_ID["bf16-64x8"], BY_ID["fp32-5x4"], BY_ID["bf16-33x16"]], ids=R.case_id)
def test_onehot_leg_premises(case):
    g = R.sweep_graph()
    for h in range(case.heads):
        assert sorted(R.permutation(g.n_cols, h)) == list(range(g.n_cols))
    assert np.array_equal(R.permutation(g.n_cols, 0), np.arange(g.n_cols))
    excluded = []
    for op in ("attn", "gatv2"):
        if op == "attn":
            q, k, v, gr, scale = R.attn_operands(g, case, "onehot")
            ref = R.attn_reference(g, q, k, v, gr, case.heads, scale)
            assert scale == 1.0 and bool((q == 128).all()) and _exact_in(k, BF16)
            key, value = k, v
        else:
            xl, xr, attn, gg, slope = R.gatv2_operands(g, case, "onehot")
            ref = R.gatv2_reference(g, xl, xr, attn, gg, case.heads, slope)
            assert xr.abs().max().item() == 0.0 and bool((attn == 128).all()) and _exact_in(xl, BF16)
            key, value = xl, xl
        # the score of a source is 128 pi_h(j): distinct sources are at least 128 apart
        score = key.double().view(-1, case.heads, case.D).sum(-1) * 128
        for h in range(case.heads):
            assert np.array_equal(score[:, h].numpy(), 128.0 * R.permutation(g.n_cols, h))
        assert torch.equal(ref["s"], score[g.col.long()])
        win, mult, top = R.winners(g, ref["s"])
        want, keep = R.onehot_expected(g, value, win, mult, case.heads)
        assert torch.equal(win[:, 0], torch.tensor([max(r) if r else -1 for r in g.rows]))
        assert case.heads == 1 or bool((win[:, 0] != win[:, 1])[torch.from_numpy(g.deg > 3)].any())   # the winner differs by head
        dropped = (~keep).any(1).nonzero().flatten().tolist()
        assert dropped in ([], [g.dup_row])
        excluded += dropped
        assert bool(((mult == 1) | ~keep | (mult == 0))[torch.arange(g.n_rows) != g.dup_row].all())
        # the float64 softmax agrees: alpha is 1 on the winner's entries / multiplicity, and the output is the winner's value
        assert (ref["out"].ref - want.double())[keep.repeat_interleave(case.D, 1)].abs().max().item() <= 1e-12
    assert len(set(excluded)) <= 1


@pytest.mark.parametrize("case", [BY_ID["fp32-8x8"], BY_ID["bf16-3x512"], BY_ID["bf16-64x8"]], ids=R.case_id)
def test_mp_leg_is_exact_in_fp32(case):
    g = R.sweep_graph()
    x, y, w = R.mp_operands(g, case)
    fwd, bwd, dots, cap = R.mp_reference(g, x, y, w, case.heads)
    assert cap < 2 ** 24 and x.double().abs().max().item() == 4 and w.abs().max().item() == 2.0
    assert torch.equal(w * 4, (w * 4).round()) and torch.equal(x.double(), x.double().round())
    for t in (fwd, bwd, dots):
        assert torch.equal(t, t.float().double())


# ---- the references against autograd -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leg", ["random", "flat"])
@pytest.mark.parametrize("case", SMALL, ids=R.case_id)
def test_references_agree_with_autograd(case, leg):
    g = R.sweep_graph()
    H, D = case.heads, case.D
    q, k, v, gr, scale = R.attn_operands(g, case, leg)
    ref = R.attn_reference(g, q, k, v, gr, H, scale)
    q64, k64, v64 = (t.double().requires_grad_() for t in (q, k, v))
    out, s = sparse_attention_reference(g.rowptr, g.col, q64.view(-1, H, D), k64.view(-1, H, D), v64.view(-1, H, D), scale)
    out = out.reshape(g.n_rows, H * D)
    want = dict(zip(("out", "dq", "dk", "dv"), (out.detach(),) + torch.autograd.grad(out, (q64, k64, v64), gr.double())))
    for name, b in want.items():
        assert (ref[name].ref - b).abs().max().item() <= 1e-12 * b.abs().max().item(), name
        assert bool((ref[name].scale >= ref[name].ref.abs() * (1 - 1e-12)).all()), name
    assert torch.equal(ref["s"], s.detach())
    xl, xr, attn, gg, slope = R.gatv2_operands(g, case, leg)
    ref = R.gatv2_reference(g, xl, xr, attn, gg, H, slope)
    xl64, xr64, a64 = (t.double().requires_grad_() for t in (xl, xr, attn))
    out, e = gatv2_reference(g.rowptr, g.col, xl64.view(-1, H, D), xr64.view(-1, H, D), a64, slope)
    out = out.reshape(g.n_rows, H * D)
    want = dict(zip(("out", "dxl", "dxr", "dattn"), (out.detach(),) + torch.autograd.grad(out, (xl64, xr64, a64), gg.double())))
    for name, b in want.items():
        # the flat leg's dxr is identically 0 (attn and the slope are constant over a row, and sum_j alpha (d - delta) = 0): both sides
        # hold rounding noise alone, which the scale measures and max|ref| does not
        yard = ref[name].scale.max().item() if leg == "flat" and name == "dxr" else b.abs().max().item()
        assert (ref[name].ref - b.reshape(ref[name].ref.shape)).abs().max().item() <= 1e-12 * yard, name
        assert bool((ref[name].scale >= ref[name].ref.abs() * (1 - 1e-12)).all()), name
    assert torch.equal(ref["s"], e.detach())


# ---- the comparators reject what they exist for ------------------------------------------------------------------------------------
def _splice(ref, mutated, head, D, rows=None):
    """ref with the columns of `head` (of the given rows) taken from mutated"""
    out = ref.clone()
    cols = slice(head * D, (head + 1) * D)
    if rows is None:
        out[:, cols] = mutated[:, cols]
    else:
        out[rows, cols] = mutated[rows, cols]
    return out


@pytest.mark.parametrize("case", SMALL[:2], ids=R.case_id)
def test_one_dropped_or_doubled_edge_fails_the_flat_and_exact_bars(case):
    g = R.sweep_graph()
    row, head, H, D = g.special[257], 1, case.heads, case.D
    q, k, v, gr, scale = R.attn_operands(g, case, "flat")
    ref = R.attn_reference(g, q, k, v, gr, H, scale)
    x, y, w = R.mp_operands(g, case)
    fwd, bwd, dots, _ = R.mp_reference(g, x, y, w, H)
    store = lambda t: t.to(case.dtype)                                      # noqa: E731
    assert not R.check_flat_forward("out", store(ref["mean"]), ref["mean"])[0]
    assert not R.check_units("dv", store(ref["dv"].ref), ref["dv"])[0]
    assert not R.check_equal("mp", store(fwd), fwd)
    for mutate in (g.without_last_entry, g.with_last_entry_twice):
        m = mutate(row)
        bad = R.attn_reference(m, q, k, v, gr, H, scale)
        got = store(_splice(ref["mean"], bad["mean"], head, D, rows=[row]))
        assert R.check_flat_forward("out", got, ref["mean"])[0]
        got = store(_splice(ref["dv"].ref, bad["dv"].ref, head, D))
        assert R.check_units("dv", got, ref["dv"])[0]
        e = int(g.rowptr[row + 1]) - 1                                      # the row's last entry
        wm = torch.cat([w[:e + 1], w[e:]]) if m.nnz > g.nnz else torch.cat([w[:e], w[e + 1:]])
        fwd_m = R.mp_reference(m, x, y, wm, H)[0]
        assert R.check_equal("mp", store(_splice(fwd, fwd_m, head, D, rows=[row])), fwd)
    # the bar this sweep replaces does not see the dropped edge in bf16: 2e-2 of the largest output
    if case.dtype == BF16:
        bad = R.attn_reference(g.without_last_entry(row), q, k, v, gr, H, scale)
        got = store(_splice(ref["mean"], bad["mean"], head, D, rows=[row]))
        err = (got.double() - ref["mean"]).abs().max().item()
        assert 0 < err <= 2e-2 * ref["mean"].abs().max().item()
        assert R.check_flat_forward("out", got, ref["mean"])[0]


@pytest.mark.parametrize("case", SMALL[:2], ids=R.case_id)
def test_onehot_equality_sees_a_dropped_winner_and_exchanged_heads(case):
    g = R.sweep_graph()
    row, H, D = g.special[257], case.heads, case.D
    q, k, v, gr, scale = R.attn_operands(g, case, "onehot")
    ref = R.attn_reference(g, q, k, v, gr, H, scale)
    win, mult, _ = R.winners(g, ref["s"])
    want, keep = R.onehot_expected(g, v, win, mult, H)
    assert not R.check_equal("out", want.clone(), want, keep, H)
    assert win[row, 0] == g.rows[row][-1]                                   # the last entry is head 0's winner
    m = g.without_last_entry(row)
    wm, mm, _ = R.winners(m, R.attn_reference(m, q, k, v, gr, H, scale)["s"])
    assert R.check_equal("out", R.onehot_expected(m, v, wm, mm, H)[0], want, keep, H)
    k3 = k.view(-1, H, D).clone()
    k3[:, [0, 1]] = k3[:, [1, 0]]                                           # two heads' scores exchanged
    ws, ms, _ = R.winners(g, R.attn_reference(g, q, k3.view(-1, H * D), v, gr, H, scale)["s"])
    assert R.check_equal("out", R.onehot_expected(g, v, ws, ms, H)[0], want, keep, H)


@pytest.mark.parametrize("case", SMALL[:2], ids=R.case_id)
def test_two_exchanged_vectors_fail_every_leg(case):
    g = R.sweep_graph()
    H, D, vec = case.heads, case.D, R.epv(case.dtype)
    store = lambda t: t.to(case.dtype)                                      # noqa: E731
    swap = lambda t: R.swap_vectors(t, 1, D, vec)                           # noqa: E731
    q, k, v, gr, scale = R.attn_operands(g, case, "flat")
    ref = R.attn_reference(g, q, k, v, gr, H, scale)
    assert R.check_flat_forward("out", swap(store(ref["mean"])), ref["mean"])[0]
    for name in ("dq", "dk", "dv"):
        assert not R.check_units(name, store(ref[name].ref), ref[name])[0], name
        # (q is constant over a head's columns in this leg, so dk is too: its exchanged vectors are the random leg's to catch)
        assert name == "dk" or R.check_units(name, swap(store(ref[name].ref)), ref[name])[0], name
    q, k, v, gr, scale = R.attn_operands(g, case, "onehot")
    ref = R.attn_reference(g, q, k, v, gr, H, scale)
    win, mult, _ = R.winners(g, ref["s"])
    want, keep = R.onehot_expected(g, v, win, mult, H)
    assert R.check_equal("out", swap(want), want, keep, H)
    q, k, v, gr, scale = R.attn_operands(g, case, "random")
    ref = R.attn_reference(g, q, k, v, gr, H, scale)
    for name in ("out", "dq", "dk", "dv"):
        assert not R.check_project(name, case.dtype, store(ref[name].ref), ref[name].ref, name == "out"), name
        assert R.check_project(name, case.dtype, swap(store(ref[name].ref)), ref[name].ref, name == "out"), name
    x, y, w = R.mp_operands(g, case)
    fwd, bwd, dots, _ = R.mp_reference(g, x, y, w, H)
    assert R.check_equal("mp", swap(store(fwd)), fwd) and R.check_equal("mp", swap(store(bwd)), bwd)
    xl, xr, attn, gg, slope = R.gatv2_operands(g, case, "flat")
    ref = R.gatv2_reference(g, xl, xr, attn, gg, H, slope)
    assert R.check_flat_forward("out", swap(store(ref["mean"])), ref["mean"])[0]
    for name in ("dxl", "dxr"):
        assert not R.check_units(name, store(ref[name].ref), ref[name])[0], name
        # (dxr is identically 0 in this leg: see test_references_agree_with_autograd)
        assert name == "dxr" or R.check_units(name, swap(store(ref[name].ref)), ref[name])[0], name
    assert not R.check_units("dattn", ref["dattn"].ref.float(), ref["dattn"])[0]
