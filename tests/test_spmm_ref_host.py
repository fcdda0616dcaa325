"""What test_spmm_geometry_gpu.py stands on, checked without a GPU: that the table of cases (spmm_ref.CASES) reaches every one of the
208 row kernels spmm_launch can instantiate -- asked of dgll_hip_debug_spmm_choice under the case's knobs, as test_spmm_choice_host.py
does --, the sweep graphs' row lengths, that the operands keep every sum exact in fp32, and the float64 reference against a dense
A @ X.  Every expected value is a literal."""
import collections

import numpy as np
import pytest
import torch

import spmm_ref
from spmm_ref import BF16, CASES, EXTRA_FORMS, F32, FORMS, KNOB_SETS, RUNS, check, expected_kernel, form_reference, operands, reference
from test_spmm_choice_host import choose, fragment, knobs

ACC = {"P1": 0, "P2": 0, "P3": 0, "E1": 1, "E2": 0, "E3": 2}        # SpmmLaunchDesc::accumulate of a form
GATE = {"P1": False, "P2": False, "P3": False, "E1": False, "E2": True, "E3": True}


def choice_of(case):
    """What spmm_choose() gives the case's launch on its graph -- under the knobs that are live."""
    g = spmm_ref.GRAPHS[case.graph]()
    flat_edges = {int(k[1:]): v for k, v in KNOB_SETS[case.knobs].plan_knobs.items()}.get(14, 256)
    return choose(case.x_dtype, case.width, g.n_rows, g.nnz, case.weighted, ACC[case.form], GATE[case.form], aligned=case.aligned,
                  y_dtype=case.y_dtype, n_chunks=g.n_chunks, n_flat=spmm_ref.n_flat(g, flat_edges))


def shown(c):
    return (c.kernel, c.lpr, c.spr, c.unroll, c.prefetch, c.epv, c.grid_y)


# ------------------------------------------------------------------------------------------------ what the table reaches
@pytest.fixture(scope="module")
def instantiations():
    """{instantiation: [cases]} with every case's choice held against the table on the way."""
    reached = collections.defaultdict(list)
    for name, ks in KNOB_SETS.items():
        with knobs(**ks.knobs):
            for case in CASES:
                if case.knobs != name:
                    continue
                c = choice_of(case)
                assert shown(c) == expected_kernel(case), (case, shown(c))
                reached[fragment(c, case.x_dtype, case.weighted, case.form in EXTRA_FORMS, y_dtype=case.y_dtype)].append(case)
    return reached


def test_the_table_is_the_one_written_down():
    assert list(KNOB_SETS) == ["default", "rowslot", "wave", "rowgroup2", "rowgroup4", "flat", "flat-nogroup", "unroll2", "unroll8",
                               "prefetch", "rpw1", "rpw3", "xcd", "flat64", "block"]
    assert list(FORMS) == ["P1", "P2", "P3", "E1", "E2", "E3"] and spmm_ref.UNALIGNED_FORMS == ("P1", "E1")
    per_set = collections.Counter(run[0] for run in RUNS)
    assert per_set == {"default": 28, "rowslot": 24, "wave": 28, "rowgroup2": 8, "rowgroup4": 4, "flat": 12, "flat-nogroup": 4,
                       "unroll2": 10, "unroll8": 10, "prefetch": 2, "rpw1": 6, "rpw3": 6, "xcd": 6, "flat64": 6, "block": 11}
    assert len(RUNS) == 165 and len(set(RUNS)) == 165
    assert len(CASES) == 165 * 12 + 28 * 4 and len(set(CASES)) == len(CASES)
    assert sorted(spmm_ref.LANES[BF16]) == [7, 32, 33, 64, 100, 128, 203, 256, 523]
    assert sorted(spmm_ref.LANES[F32]) == [3, 16, 29, 32, 47, 64, 100, 128, 131, 300]
    # a "default" run of every width and dtype pair: all six forms and the two unaligned ones, weighted and not
    assert sum(c.knobs == "default" and not c.aligned for c in CASES) == 28 * 4


def test_the_table_reaches_all_208_instantiations(instantiations):
    assert len(instantiations) == 208
    family = collections.Counter()
    for name in instantiations:
        one_per_lane = name.startswith("spmm_csr_kernel<") and name.split(", ")[2] == "1"
        family["one-element-per-lane" if one_per_lane else name.split("<")[0]] += 1
    assert family == {"spmm_csr_kernel": 112, "spmm_rowslot_kernel": 48, "spmm_csr_flat_kernel": 24, "spmm_rowgroup_kernel": 12,
                      "one-element-per-lane": 12}


def _template_args(name):
    """(family, HAS_VAL, EXTRA or None, the name without HAS_VAL) of an instantiation's name."""
    family, args = name[:name.index("<")], name[name.index("<") + 1:-1].split(", ")
    hv, ex = {"spmm_csr_kernel": (4, 6), "spmm_rowslot_kernel": (4, 5), "spmm_csr_flat_kernel": (4, 6), "spmm_rowgroup_kernel": (5, None)}[family]
    return family, args[hv] == "true", None if ex is None else args[ex] == "true", (family,) + tuple(v for i, v in enumerate(args) if i != hv)


def test_every_instantiation_runs_its_forms_weighted_and_not(instantiations):
    twins = collections.defaultdict(set)
    n_extra = 0
    for name, cases in instantiations.items():
        family, has_val, extra, rest = _template_args(name)
        assert {c.weighted for c in cases} == {has_val}, name
        twins[rest].add(has_val)
        forms = {c.form for c in cases}
        if extra:                    # the accumulate / gate epilogue: all three forms (the unaligned kernel: E1)
            n_extra += 1
            assert forms == (set(EXTRA_FORMS) if cases[0].aligned else {"E1"}), (name, forms)
        else:
            assert forms == ({"P1", "P2", "P3"} if cases[0].aligned else {"P1"}), (name, forms)
    # HAS_VAL is a template argument: every kernel is reached weighted and unweighted
    assert len(twins) == 104 and all(v == {True, False} for v in twins.values())
    assert n_extra == (208 - 12) // 2                      # EXTRA doubles every family but row-group


def test_schedules_on_top_of_the_instantiations():
    g = spmm_ref.sweep_graph()

    def ask(name, dtype, width, **kw):
        with knobs(**KNOB_SETS[name].knobs):
            return choose(dtype, width, g.n_rows, g.nnz, n_chunks=g.n_chunks, n_flat=spmm_ref.n_flat(g), **kw)

    assert ask("rpw1", BF16, 256).rows_per_wave == 1 and ask("rpw3", BF16, 256).rows_per_wave == 3
    assert ask("default", BF16, 256).rows_per_wave not in (1, 3)
    assert ask("rpw1", BF16, 64).rows_per_wave == 4 and ask("rpw3", BF16, 64).rows_per_wave == 4        # row-group: four rows at a time
    c = ask("xcd", F32, 300)
    assert (c.kernel, c.rows_per_wave, c.row_blocks, c.chunk_blocks, c.grid_y) == (0, 1, 276, 16, 2)  # 276 % 8 != 0: the remap's tail
    # 33 chunk items are 9 blocks of four, rounded up to 16: seven chunk blocks idle but for one wavefront
    assert ask("default", F32, 100).chunk_blocks == 16
    # the flattened schedule at 64 edges per share: four times the shares
    assert spmm_ref.n_flat(g) == -(-(g.nnz + 4 * 1103) // 256) and spmm_ref.n_flat(g, 64) == -(-(g.nnz + 4 * 1103) // 64)
    with knobs(**KNOB_SETS["flat64"].knobs):
        c = choose(F32, 100, g.n_rows, g.nnz, n_chunks=g.n_chunks, n_flat=spmm_ref.n_flat(g, 64))
    assert c.kernel == 3 and c.row_blocks == -(-spmm_ref.n_flat(g, 64) // 4)
    # the host-only plan: no chunk items, no flattened schedule
    b = spmm_ref.block_graph()
    assert (b.n_chunks, b.n_long, spmm_ref.n_flat(b)) == (0, 0, 0)
    c = choose(F32, 100, b.n_rows, b.nnz, n_chunks=0, n_flat=0)
    assert (c.kernel, c.chunk_blocks) == (0, 0)


# ------------------------------------------------------------------------------------------------ the graphs
def test_sweep_graph_row_lengths():
    g = spmm_ref.sweep_graph()
    assert (g.n_rows, g.n_cols) == (1103, 4200) and g.rowptr.dtype == np.int64 and g.col.dtype == np.int32 and g.val.dtype == np.float32
    assert g.nnz == int(g.rowptr[-1]) == g.col.shape[0] == g.val.shape[0] and np.array_equal(np.diff(g.rowptr), g.deg)
    lengths = set(g.deg.tolist())
    assert lengths >= {0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 513, 2049, 4097}
    assert g.deg[0] == 0 and g.deg[1102] == 0
    assert g.deg[4:8].tolist() == [5, 0, 2049, 3]                  # one lane-group set: short, empty, LONG, short
    assert sorted(g.deg[g.deg > 256].tolist()) == [257, 512, 513, 2049, 4097]
    assert (g.n_long, g.n_chunks) == (5, 33)                       # 2 + 2 + 3 + 9 + 17
    ordinary = np.array([d for r, d in enumerate(g.deg.tolist()) if r not in spmm_ref.SPECIAL_ROWS])
    assert len(ordinary) == 1073 and 10 <= ordinary.min() and ordinary.max() <= 60 and 29.0 < ordinary.mean() < 31.0
    assert 24.0 < g.nnz / g.n_rows <= 64.0                         # inside the row-group band of 16-lane rows, above the row-per-slot band
    for r in range(g.n_rows):
        mine = g.col[g.rowptr[r]:g.rowptr[r + 1]]
        assert bool((mine[1:] > mine[:-1]).all())                  # sorted, distinct
    used = np.bincount(g.col, minlength=g.n_cols) > 0
    assert not used[0] and not used[4190:].any() and g.col.min() >= 1 and g.col.max() == 4189       # the row of 4 097 edges reaches far
    assert spmm_ref.sweep_graph() is g


def test_block_graph_is_the_short_rows():
    g, b = spmm_ref.sweep_graph(), spmm_ref.block_graph()
    assert b.max_degree == 128 and int(b.deg.max()) == 128 and b.n_cols == 4200
    assert b.deg.tolist() == [d for d in g.deg.tolist() if d <= 128] and b.n_rows == 1103 - 8
    assert 24.0 < b.nnz / b.n_rows <= 64.0
    used = np.bincount(b.col, minlength=b.n_cols) > 0
    assert not used[0] and not used[4190:].any()


# ------------------------------------------------------------------------------------------------ the operands
def test_every_sum_of_the_sweep_is_exact_in_fp32():
    """max over rows of sum |a_ij|, times max |x|, in quarter units, stays below 2^24 -- with the epilogue's additions (|Y_old| and
    |bias| <= 8 each) inside the same cap; and every operand survives the trip to bf16."""
    for graph in ("sweep", "block"):
        g = spmm_ref.GRAPHS[graph]()
        for weighted in (False, True):
            mag = np.abs(g.val.astype(np.float64)) if weighted else np.ones(g.nnz)
            row_abs = np.array([mag[g.rowptr[r]:g.rowptr[r + 1]].sum() for r in range(g.n_rows)])
            for dtype, widths in spmm_ref.LANES.items():
                for width in widths:
                    op = operands(graph, width, dtype)
                    assert float(row_abs.max()) * float(np.abs(op["x"]).max()) * 4 < 2 ** 24
                    assert (float(row_abs.max()) * float(np.abs(op["x"]).max()) + 16) * 4 < 2 ** 24
    g = spmm_ref.sweep_graph()
    assert set(np.unique(g.val * 4).tolist()) == set(range(-8, 9))                 # multiples of 1/4 in [-2, 2]
    op = operands("sweep", 203, BF16)
    assert set(np.unique(op["x"]).tolist()) == set(range(-4, 5)) and set(np.unique(op["bias"]).tolist()) <= set(range(-8, 9))
    assert set(np.unique(op["row_scale"]).tolist()) == {0.25, 0.5, 1.0, 2.0} and set(np.unique(op["y_old"]).tolist()) == set(range(-8, 9))
    assert set(np.unique(op["gate"]).tolist()) == {-1.0, 0.0, 1.0} and bool(np.signbit(op["gate"][op["gate"] == 0]).any())
    assert not bool(np.signbit(op["gate"][op["gate"] == 0]).all())
    for a in op.values():
        assert spmm_ref.storage(a, BF16).dtype == torch.bfloat16                   # storage() asserts the round trip
    assert operands("sweep", 203, BF16) is op and not np.array_equal(operands("sweep", 203, BF16)["x"][:, :100], operands("sweep", 100, BF16)["x"])


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("weighted", [False, True])
def test_reference_equals_dense_numpy_for_every_form(weighted):
    """reference() (reduceat over the edge list) against a dense float64 A @ X with the epilogues written out again, on the sweep
    graph: equal to the last bit -- both are exact."""
    g = spmm_ref.sweep_graph()
    width, dtype = 47, F32
    op = operands("sweep", width, dtype)
    A = np.zeros((g.n_rows, g.n_cols))
    rows = np.repeat(np.arange(g.n_rows), g.deg)
    A[rows, g.col] = g.val if weighted else 1.0
    S = A @ op["x"]
    x, b, sc, y0, gt = op["x"], op["bias"], op["row_scale"][:, None], op["y_old"], op["gate"] > 0
    has = (g.deg > 0)[:, None]
    dense = {
        "P1": S,
        "P2": np.maximum(S / np.maximum(g.deg, 1)[:, None] + b, 0),
        "P3": S * sc + b,
        "E1": np.maximum((S + y0) * sc + b, 0),
        "E2": S * gt,
        "E3": y0 + has * (S * sc * gt),
    }
    assert set(dense) == set(FORMS)
    for form, want in dense.items():
        ref, bound = form_reference("sweep", width, dtype, weighted, form)
        assert (bound is not None) == (form == "P2")
        assert np.array_equal(ref, want), form
    assert np.array_equal(reference(g, x, weighted), S)


def test_the_bars_see_one_wrong_edge():
    """One edge of the 4 097-edge row dropped, one doubled, two weights swapped: each moves elements of that row by at least 1/4
    and check() names the row; the reference itself passes, for fp32 and bf16 outputs and for the mean form."""
    g = spmm_ref.sweep_graph()
    width, dtype, row = 100, BF16, 901
    x = operands("sweep", width, dtype)["x"]
    b, e = int(g.rowptr[row]), int(g.rowptr[row + 1])
    assert e - b == 4097
    for form in ("P1", "P2", "E1"):
        ref, bound = form_reference("sweep", width, dtype, True, form)
        for yd, t in ((F32, torch.float32), (BF16, torch.bfloat16)):
            assert check(form, torch.from_numpy(ref).to(torch.float32).to(t), ref, bound, yd, g.deg) == []
    ref, _ = form_reference("sweep", width, dtype, True, "P1")
    k = b + 4000
    j = next(i for i in range(b, e) if g.val[i] != g.val[k])
    edge = lambda i: float(g.val[i]) * x[g.col[i]]              # noqa: E731
    for delta in (-edge(k), edge(k), (float(g.val[j]) - float(g.val[k])) * (x[g.col[k]] - x[g.col[j]])):
        assert float(np.abs(delta).max()) >= 0.25
        wrong = ref.copy()
        wrong[row] += delta
        found = check("P1", torch.from_numpy(wrong).to(torch.float32), ref, None, F32, g.deg)
        assert len(found) == 1 and "row 901 (4097 edges)" in found[0], found
    # a NaN that leaked in, and a value that is not the rounding of the reference
    wrong = torch.from_numpy(ref).to(torch.float32)
    wrong[7, 3] = float("nan")
    assert "not finite at row 7 (3 edges) column 3" in check("P1", wrong, ref, None, F32, g.deg)[0]
    assert check("P1", wrong, ref, None, F32, g.deg, rows=np.arange(g.n_rows) != 7) == []
    # the mean bar has no floor: a reference of 0 must come out as 0
    ref, bound = form_reference("sweep", width, dtype, False, "P2")
    zero = np.argwhere(bound == 0)                   # S = 0 (an empty row among them) under a bias of 0
    assert len(zero) > 0 and bool((ref[bound == 0] == 0).all()) and 0 in zero[:, 0]
    wrong = torch.from_numpy(ref).to(torch.float32)
    wrong[zero[0][0], zero[0][1]] = 1e-30
    assert len(check("P2", wrong, ref, bound, F32, g.deg)) == 1
