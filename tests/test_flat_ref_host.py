"""flat_ref.py without a GPU: the literal width table is what make_flat_geometry gives (its restatement and the C++ itself, compiled
from the unmodified csrc/row_tiles.hpp) and reaches every lane width full and with idle lanes and one, two and three column blocks;
every long-row threshold of the flat files is the one the sweep graph is built for; the float64 reference rounded once to the storage
dtype stays inside the per-row comparator; the comparator rejects, on reference arrays alone, a dropped and a doubled entry; the exact
legs' premises hold in float64; and the pinned GMM seeds are conditioned as their test asks."""
import subprocess

import numpy as np
import pytest
import torch

import flat_ref as FR
import rowtile_ref as R
from flat_ref import DTYPES, OPERATORS, TABLE, dname
from kernel_emu import build_emulator
from rowtile_ref import BF16, F32

CLASSES = (1, 9, 17, 33, 129)           # a width per lane width, and the three-block one
_ids = lambda v: v.name if hasattr(v, "name") else str(v).replace("torch.", "")      # noqa: E731


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
def test_table_is_what_make_flat_geometry_gives(tmp_path_factory):
    exe = build_emulator(tmp_path_factory, "row_tiles.hpp", "geometry_main.cpp")
    cases = [(vpr, n) for vpr, _, _ in TABLE for n in (R.N_ROWS, R.N_COLS)]
    res = subprocess.run([exe, "flat"] + [str(v) for c in cases for v in c], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    lines = [tuple(int(v) for v in ln.split()) for ln in res.stdout.splitlines()]
    assert len(lines) == len(cases)
    k = 0
    for vpr, lpr, blocks in TABLE:
        for n in (R.N_ROWS, R.N_COLS):
            tiles = -(-n // (256 // lpr))
            assert lines[k] == (lpr, blocks, tiles, tiles), (vpr, n, lines[k])
            assert FR.flat_geometry(vpr, n) == (lpr, blocks, tiles)
            assert n != R.N_ROWS or n % (256 // lpr) != 0      # the rows end in a ragged tile at every lane width
            k += 1


def test_table_reaches_every_lane_width_full_and_idle_and_three_column_blocks():
    one_block = {(lpr, vpr == lpr) for vpr, lpr, blocks in TABLE if blocks == 1}
    assert one_block == {(lpr, full) for lpr in (8, 16, 32, 64) for full in (False, True)}
    assert {blocks for _, _, blocks in TABLE} == {1, 2, 3}
    assert (65, 64, 2) in TABLE and (128, 64, 2) in TABLE and (129, 64, 3) in TABLE
    assert {FR.flat_geometry(v, 1)[0] for v in FR.LPR_WIDTHS} == {8, 16, 32, 64}
    assert set(FR.LPR_WIDTHS) <= set(FR.VPRS) and FR.NAN_VPR in FR.VPRS and FR.FAULT_VPR in FR.VPRS
    assert all(FR.width(v, F32) == 4 * v and FR.width(v, BF16) == 8 * v for v in FR.VPRS)
    # more than one tile at every lane width, and per-edge operands that stay small
    assert all(FR.flat_geometry(v, R.N_ROWS)[2] >= 10 for v in FR.VPRS)
    assert R.sweep_graph().nnz < 6000


def test_every_long_row_threshold_is_the_one_the_graph_is_built_for():
    from dgll_amd import _lib

    names = [n for n in dir(_lib) if n.endswith("_LONG_ROW")]
    assert len(names) == 11 and all(getattr(_lib, n) == R.LONG_ROW for n in names), names
    for n in ("EF", "EFP", "GATED", "RES_GATED", "SOFT_AGG", "GMM", "MAGG", "TYPED"):       # the eight flat files
        assert getattr(_lib, n + "_LONG_ROW") == R.LONG_ROW == 256


def test_fault_drops_and_doubles_one_entry():
    g = R.sweep_graph()
    for label, side, row, pos in FR.planted_faults(g):
        last = pos == -1
        fg, keep = FR.fault(g, row, pos, "drop")
        assert fg.nnz == g.nnz - 1 and torch.equal(fg.col, g.col[keep])
        if last:
            assert fg.rows == g.without_last_entry(row).rows
        fg, keep = FR.fault(g, row, pos, "twice")
        assert fg.nnz == g.nnz + 1 and torch.equal(fg.col, g.col[keep])
        if last:
            assert fg.rows == g.with_last_entry_twice(row).rows
        if side == "col":
            assert g.rows[row][pos] == FR.HUB and g.indeg[FR.HUB] == R.LONG_ROW + 1
    assert [len(g.rows[g.special[n]]) for n in FR.FAULT_ROWS] == list(FR.FAULT_ROWS)


# ---- the reference alone stays inside the comparator -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("op", OPERATORS, ids=_ids)
def test_reference_rounded_once_passes(op, dtype):
    g = R.sweep_graph()
    empty = np.flatnonzero(g.deg == 0)
    for vpr in CLASSES:
        config = op.CONFIGS[0]
        ins, ref = FR.case(op, vpr, dtype, config, keep=vpr == FR.FAULT_VPR)
        for name, q in ref.items():
            got = FR.stored(q, name, dtype)
            found, frac, _ = FR.judge(op, dtype, name, got, q)
            assert not found, (op.name, vpr, name, found)
            if q.side != "whole":                           # one rounding: half an ulp of the row's largest element at the most
                assert frac <= (2.0 ** -8 if got.dtype == BF16 else 2.0 ** -23), (op.name, vpr, name, frac)
            if q.side == "row":
                assert got[empty].abs().max().item() == 0.0
            if q.side == "col":
                assert got[list(g.unreferenced)].abs().max().item() == 0.0


# ---- planted faults are rejected ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("op", OPERATORS, ids=_ids)
def test_planted_faults_are_rejected(op, dtype):
    """What a kernel would give that dropped or doubled one entry -- the reference of the faulted graph -- judged against the true
    graph's reference: every quantity that sums over entries must fail, in fp32 and on the tight form in bf16 (a condition on the
    pinned seeds); a bf16 quantity on the fallback form misses exactly what flat_ref.FALLBACK_MISSES lists."""
    g = R.sweep_graph()
    config = op.CONFIGS[0]
    ins, ref = FR.case(op, FR.FAULT_VPR, dtype, config, keep=True)
    missed = []
    for label, side, row, pos in FR.planted_faults(g):
        for how in ("drop", "twice"):
            _, _, bad = FR.faulted_reference(op, g, ins, config, row, pos, how)
            judged = 0
            for name, q in ref.items():
                if q.side not in ("row", "col"):
                    continue
                judged += 1
                found = FR.judge(op, dtype, name, FR.stored(bad[name], name, dtype), q)[0]
                if not found:
                    missed.append((name, label, how))
            assert judged >= 2
    fallback = dtype == BF16 and any(o == op.name for o, _ in FR.FALLBACK)
    assert sorted(missed) == (sorted(m[1:] for m in FR.FALLBACK_MISSES if m[0] == op.name) if fallback else []), (op.name, dname(dtype), missed)


def test_a_whole_tensor_bar_would_miss_what_the_per_row_bar_rejects():
    """The reason for the comparator: a dropped entry of the 513-entry row of a bf16 mean sits under 2e-2 max |ref| of the whole
    tensor, the bar of the operator's own test, and over the per-row bar."""
    g = R.sweep_graph()
    op, config = FR.ResGated, "mean"
    ins, ref = FR.case(op, FR.FAULT_VPR, BF16, config, keep=True)
    _, _, bad = FR.faulted_reference(op, g, ins, config, g.special[513], -1, "drop")
    got, q = FR.stored(bad["out"], "out", BF16), ref["out"]
    assert ((got.double() - q.ref).abs().max() / q.ref.abs().max()).item() <= 2e-2
    assert FR.judge(op, BF16, "out", got, q)[0]


# ---- the exact legs' premises ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_exact_leg_premises(dtype):
    """every partial sum is a multiple of the unit below 2^24 units: exactly representable in fp32 in any order"""
    g = R.sweep_graph()
    for vpr in (1, 129):
        for config in FR.EdgeFeat.CONFIGS:
            ins = FR.EdgeFeat.inputs(g, vpr, dtype, config, "exact")
            assert all(bool((ins[k].double() == ins[k].double().round()).all()) and ins[k].abs().max().item() <= 4 for k in "xeg")
            assert ins["scale"] is None or set(ins["scale"].tolist()) <= {0.0, 0.25, 0.5, 1.0}
            assert FR.EdgeFeat.magnitude(g, ins, config) < 2 ** 24
        for config in FR.EdgeProj.DYADIC:
            ins = FR.EdgeProj.inputs(g, vpr, dtype, config, "exact")
            assert FR._is_dyadic(ins) and max(v.abs().max().item() for v in ins.values() if v is not None) <= 2
            assert FR.EdgeProj.magnitude(g, ins, config) < 2 ** 24
        ins = FR.Gmm.inputs(g, vpr, dtype, "sum", "exact")
        assert FR._is_dyadic({k: ins[k] for k in ("x", "g")})
        assert FR.Gmm.magnitude(g, ins) < 2 ** 24
    assert {c[0] for c in FR.EdgeProj.DYADIC} == set(FR.efp_ref.OPS)
    assert {(c[0], 4 if c[2] <= 4 else 8 if c[2] <= 8 else 16) for c in FR.EdgeProj.DYADIC} == {(o, d) for o in FR.efp_ref.OPS for d in (4, 8, 16)}


# ---- the pinned seeds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_gmm_seeds_are_well_conditioned(dtype):
    from test_gmm_emulated import MAX_CONDITIONING

    g = R.sweep_graph()
    for vpr in FR.VPRS:
        for config in FR.Gmm.CONFIGS:
            ins = FR.Gmm.inputs(g, vpr, dtype, config, "random")
            _, terms = FR.Gmm.reference(g, ins, config, terms=True)
            for t in terms:
                assert FR.gmm_ref.conditioning(t) <= MAX_CONDITIONING, (vpr, config)


def test_edge_proj_add_relu_seeds_leave_the_gate_margin_empty():
    """efp_ref.near_gate counts no element for every pinned seed (the precondition of comparing add_relu on random inputs), the pinned n
    is the first that does, and the widths without a seed are the ones the module text names."""
    g = R.sweep_graph()
    have = {dt: sorted(v for v, d in FR.EFP_SEEDS if d == dname(dt)) for dt in DTYPES}
    assert have[F32] == [v for v in FR.VPRS if v != 129] and have[BF16] == [1, 8, 9, 16, 17, 32]
    assert {FR.flat_geometry(v, 1)[:2] for v in have[F32]} >= {(8, 1), (16, 1), (32, 1), (64, 1), (64, 2)}
    assert {FR.flat_geometry(v, 1)[0] for v in have[BF16]} == {8, 16, 32}
    config = FR.EdgeProj.RELU
    for dtype in DTYPES:
        for vpr in have[dtype]:
            n = FR.EFP_SEEDS[(vpr, dname(dtype))]
            ins = FR.EdgeProj.inputs(g, vpr, dtype, config, "random")
            x, a, W, b = (ins[k].double() for k in ("x", "a", "W", "b"))
            assert FR.efp_ref.near_gate(g.col, x, a, W, b) == 0, (vpr, dname(dtype))
            if 0 < n <= 2:                                  # the first such n (checked where that is cheap)
                for m in range(n):
                    seed = FR.seed_of(vpr, dtype, 23) + FR.EFP_SEED_STEP * m
                    x, a, _, W, b = FR.efp_ref.inputs(g, FR.width(vpr, dtype), 3, dtype, seed, False, True)
                    assert FR.efp_ref.near_gate(g.col, x.double(), a.double(), W.double(), b.double()) > 0
    with pytest.raises(KeyError):
        FR.EdgeProj.inputs(g, 129, F32, config, "random")


def test_gated_mask_without_a_gradient_through_ehat_leaves_only_one_entry_rows_out():
    g = R.sweep_graph()
    assert all(FR.Gated.judged(g, True, n) is None for n in ("out", "ehat", "grad_a", "grad_b", "grad_c", "grad_v"))
    assert all(FR.Gated.judged(g, False, n) is None for n in ("out", "ehat", "grad_v"))
    rows, edges, cols = (FR.Gated.judged(g, False, n) for n in ("grad_a", "grad_c", "grad_b"))
    single = int((g.deg == 1).sum())
    assert single > 0 and int((~rows).sum()) == single and int((~edges).sum()) == single
    assert rows[g.special[9]] and rows[g.special[513]] and rows[0] and not rows[g.special[1]]
    left_out = [c for c in range(g.n_cols) if not cols[c]]
    assert len(left_out) <= single and all(all(g.deg[r] == 1 for r in t) and t for c, t in enumerate(g.transposed_rows()) if c in left_out)
    assert cols[FR.HUB] and all(cols[c] for c in g.unreferenced)
