"""The float64 reference of the SpMM launches (csrc/spmm.hip), the graphs they are swept on, operands whose sums are exact in fp32,
and the table of cases: shared by test_spmm_ref_host.py (which pins all of it without a GPU) and test_spmm_geometry_gpu.py.

Why the comparison needs no tolerance.  X holds integers in [-4, 4], the edge weights multiples of 1/4 in [-2, 2] (unweighted: 1), so
every product is a multiple of 1/4 of magnitude <= 8 and any partial sum of the longest row (4 097 edges), in any order, is a
multiple of 1/4 below 32 776 = 131 104 quarter units < 2^24: exact in fp32, in registers, in the chunk partials and in their sum.
Bias and the previous Y are integers in [-8, 8], row_scale is a power of two in [1/4, 2], the gate is one of {-1, -0.0, 0.0, +1}:
all exact in bf16, and every epilogue with reduce = "sum" or a row_scale stays exact (an fma instead of a multiply and an add makes
no difference).  The float64 reference is then THE answer: an fp32 output equals it bit for bit, a bf16 output equals its
round-to-nearest-even.  reduce = "mean" without row_scale has one inexact step, 1.0f / len: see check().

Nothing here touches a device or any part of dgll_amd."""
import collections
import functools

import numpy as np
import torch

F32, BF16 = 0, 1            # DGLL_F32, DGLL_BF16 (include/dgll_hip.h)
THRESHOLD = 256             # the plan's long-row threshold and chunk length (spmm.hip: dgll_hip_csr_plan_create)

# ------------------------------------------------------------------------------------------------ the graphs
N_ROWS, N_COLS = 1103, 4200         # 1103 is prime: a multiple of no rows-per-wave value
FIRST_COL, END_COL = 1, 4190        # column 0 and columns 4190 .. 4199 are referenced by no row
# row -> its exact number of edges; every other row draws Poisson(30).  A round of a kernel is SLOTS x U = 2 .. 64 edges, an index
# batch 64, a row-group round 8 or 16: lengths on both sides of each.  256 is exactly the threshold (runs inline); 257 leaves a
# chunk of one edge, 512 is two full chunks, 2 049 = nine chunks (the finalize kernel's second trip: one live partial, seven clamped),
# 4 097 = seventeen (a third trip).  Rows 4 .. 7 are one lane-group set of a wavefront that takes four rows at a time: short, empty,
# LONG, short.  The first and the last row are empty.
SPECIAL_ROWS = {0: 0, 4: 5, 5: 0, 6: 2049, 7: 3, 40: 1, 41: 2, 42: 4, 43: 7, 100: 8, 101: 9, 102: 15, 103: 16, 200: 17, 201: 31,
                202: 32, 203: 33, 300: 63, 301: 64, 302: 65, 400: 127, 401: 128, 402: 129, 500: 255, 501: 256, 502: 257, 640: 512,
                777: 513, 901: 4097, 1102: 0}

Graph = collections.namedtuple("Graph", "name rowptr col val deg n_rows n_cols nnz n_long n_chunks max_degree")


def _graph(name, deg, rng, max_degree):
    rowptr = np.zeros(len(deg) + 1, np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = np.concatenate([np.sort(rng.choice(np.arange(FIRST_COL, END_COL), d, replace=False)) for d in deg]).astype(np.int32)
    val = (rng.integers(-8, 9, col.shape[0]) / 4.0).astype(np.float32)           # multiples of 1/4 in [-2, 2]
    long_rows = deg[deg > THRESHOLD] if max_degree is None else deg[:0]
    return Graph(name, rowptr, col, val, deg.astype(np.int64), len(deg), N_COLS, int(rowptr[-1]), len(long_rows),
                 int(sum(-(-int(d) // THRESHOLD) for d in long_rows)), max_degree)


def _sweep_degrees():
    deg = np.random.default_rng(20241019).poisson(30, N_ROWS)
    for r, d in SPECIAL_ROWS.items():
        deg[r] = d
    return deg


@functools.lru_cache(maxsize=None)
def sweep_graph():
    """The 1103 x 4200 sweep adjacency: Graph(name, rowptr int64, col int32, val fp32, deg, n_rows, n_cols, nnz, n_long, n_chunks,
    max_degree) in numpy.  Columns sorted and distinct within a row; n_long / n_chunks are what a plan at threshold 256 holds."""
    return _graph("sweep", _sweep_degrees(), np.random.default_rng(7), None)


@functools.lru_cache(maxsize=None)
def block_graph():
    """The rows of sweep_graph() with at most 128 edges, in their order, as a second graph with max_degree = 128: CSRGraph gives
    it the host-only plan (threshold 0, no flattened schedule, every row gathered inline)."""
    deg = _sweep_degrees()
    return _graph("block", deg[deg <= 128], np.random.default_rng(8), 128)


GRAPHS = {"sweep": sweep_graph, "block": block_graph}


def n_flat(g, flat_edges=256):
    """Shares of the plan's flattened schedule (spmm.hip: kFlatRowCost = 4 per row); 0 for the host-only plan."""
    return 0 if g.max_degree is not None else -(-(g.nnz + 4 * g.n_rows) // flat_edges)


# ------------------------------------------------------------------------------------------------ the operands
@functools.lru_cache(maxsize=None)
def operands(graph, width, dtype):
    """{"x" [n_cols, width], "bias" [width], "row_scale" [n_rows], "y_old" [n_rows, width], "gate" [n_rows, width]} as float64 numpy
    arrays from a generator seeded by (graph, width, dtype); every value is exact in bf16."""
    g = GRAPHS[graph]()
    rng = np.random.default_rng([len(graph), width, dtype])
    return dict(x=rng.integers(-4, 5, (g.n_cols, width)).astype(np.float64),
                bias=rng.integers(-8, 9, width).astype(np.float64),
                row_scale=rng.choice(np.array([0.25, 0.5, 1.0, 2.0]), g.n_rows),
                y_old=rng.integers(-8, 9, (g.n_rows, width)).astype(np.float64),
                gate=rng.choice(np.array([-1.0, -0.0, 0.0, 1.0]), (g.n_rows, width)))


def storage(a, dtype):
    """A float64 array of the operands as a CPU torch tensor in the storage dtype (exact: the values are representable)."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16 if dtype == BF16 else torch.float32)
    assert bool((t.double() == torch.from_numpy(np.ascontiguousarray(a))).all())
    return t


# ------------------------------------------------------------------------------------------------ the reference
def row_sums(g, x, weighted):
    """A . X in float64: the products of every edge, summed per row with np.add.reduceat over the rows that have edges."""
    prod = x[g.col.astype(np.int64)]
    if weighted:
        prod = prod * g.val.astype(np.float64)[:, None]
    out = np.zeros((g.n_rows, x.shape[1]))
    live = g.deg > 0
    if prod.shape[0]:
        out[live] = np.add.reduceat(prod, g.rowptr[:-1][live], axis=0)
    return out


def reference(g, x, weighted=False, reduce="sum", row_scale=None, bias=None, relu=False, accumulate=0, y_old=None, gate=None, s=None):
    """Y of one launch in float64, in the order of SpmmArgs::accumulate's comment and finish_row (spmm.hip):
    accumulate 0: Y = gate(relu(scale . A.X + bias));  1: Y = gate(relu(scale . (A.X + Y_old) + bias));
    2: Y = Y_old + gate(scale . A.X), rows without edges untouched.  scale is row_scale, else 1 / len for "mean" (len > 0), else 1;
    the gate zeroes where !(gate > 0), so -0.0 and 0.0 both zero.  s: A.X if the caller has it already."""
    s = row_sums(g, x, weighted) if s is None else s
    v = s + y_old if accumulate == 1 else s
    if row_scale is not None:
        v = v * row_scale[:, None]
    elif reduce == "mean":
        v = v / np.maximum(g.deg, 1)[:, None]            # one division: the correctly rounded quotient
    if bias is not None:
        v = v + bias
    if relu:
        v = np.maximum(v, 0.0)
    if gate is not None:
        v = np.where(gate > 0, v, 0.0)
    if accumulate == 2:
        v = np.where((g.deg > 0)[:, None], y_old + v, y_old)
    return v


# ------------------------------------------------------------------------------------------------ the forms
# what a form passes to ops.spmm_raw besides the graph and X (True: the operand of that name from operands())
FORMS = {
    "P1": dict(reduce="sum"),
    "P2": dict(reduce="mean", bias=True, relu=True),
    "P3": dict(reduce="sum", row_scale=True, bias=True),           # written into a slice of a larger buffer: ldy != ldx
    "E1": dict(reduce="sum", accumulate=1, row_scale=True, bias=True, relu=True),
    "E2": dict(reduce="sum", gate=True),
    "E3": dict(reduce="sum", accumulate=2, gate=True, row_scale=True),
}
EXTRA_FORMS = ("E1", "E2", "E3")


@functools.lru_cache(maxsize=64)
def _sums(graph, width, dtype, weighted):
    return row_sums(GRAPHS[graph](), operands(graph, width, dtype)["x"], weighted)


def form_reference(graph, width, dtype, weighted, form):
    """(ref, bound): the float64 result of the form on the operands of (graph, width, dtype); bound is None for the exact forms
    and, for "mean" without row_scale, the elementwise fp32 bound 2^-21 (|S| / len + |bias|): HIP allows 2.5 ulp for 1.0f / len, the
    product adds 0.5 and the bias add 0.5 -- under 4 ulp = 2^-21 of the two terms' magnitudes.  No floor: a reference of 0 (S = 0 and
    no bias, or an empty row) must come out as 0."""
    g, op, f = GRAPHS[graph](), operands(graph, width, dtype), FORMS[form]
    s = _sums(graph, width, dtype, weighted)
    pick = lambda name: op[name] if f.get(name) else None           # noqa: E731
    ref = reference(g, op["x"], weighted, f["reduce"], pick("row_scale"), pick("bias"), bool(f.get("relu")), f.get("accumulate", 0),
                    op["y_old"] if f.get("accumulate") else None, pick("gate"), s=s)
    bound = None
    if f["reduce"] == "mean" and not f.get("row_scale"):
        bound = 2.0 ** -21 * (np.abs(s) / np.maximum(g.deg, 1)[:, None] + (np.abs(op["bias"]) if f.get("bias") else 0.0))
    return ref, bound


# ------------------------------------------------------------------------------------------------ the bars
def check(name, got, ref, bound, y_dtype, deg, rows=None):
    """Hold `got` (a torch tensor, any device) against the float64 `ref`; returns the violations as a list of strings (empty: inside).
    bound None -- an exact form: fp32 output torch.equal to ref cast to fp32, bf16 output torch.equal to ref cast to bf16 (the stored
    value is ONE round-to-nearest-even of an exactly known number; ref is exact in fp32, so the cast rounds once).
    bound given -- "mean": |got - ref| <= bound elementwise for fp32, bound + 2^-8 |ref| (half a bf16 step) for bf16.  No atol.
    rows: boolean mask of the rows to compare (the others are the caller's business).  The worst element is named by row, the row's
    length and column."""
    got = got.detach().cpu()
    assert tuple(got.shape) == ref.shape, (name, tuple(got.shape), ref.shape)
    want = torch.from_numpy(np.ascontiguousarray(ref))
    keep = torch.ones(ref.shape[0], dtype=torch.bool) if rows is None else torch.from_numpy(np.ascontiguousarray(rows))
    g64 = got.double()
    if not bool(torch.isfinite(g64[keep]).all()):
        r, c = [int(v[0]) for v in torch.nonzero(~torch.isfinite(g64) & keep[:, None], as_tuple=True)]
        return ["%s: not finite at row %d (%d edges) column %d" % (name, r, int(deg[r]), c)]
    if bound is None:
        cast = want.to(torch.float32) if y_dtype == F32 else want.to(torch.float32).to(torch.bfloat16)
        assert got.dtype == cast.dtype, (name, got.dtype)
        bad = (got != cast) & keep[:, None]              # elementwise torch.equal: values, so -0.0 equals 0.0 and a NaN nothing
        over = torch.where(bad, (g64 - want).abs(), torch.zeros_like(want))
        bar = "exact"
    else:
        tol = torch.from_numpy(np.ascontiguousarray(bound)) + (2.0 ** -8 * want.abs() if y_dtype == BF16 else 0.0)
        err = (g64 - want).abs()
        bad = (err > tol) & keep[:, None]
        over = torch.where(bad, err, torch.zeros_like(want))
        bar = "2^-21 (|S| / len + |bias|)" + (" + 2^-8 |ref|" if y_dtype == BF16 else "")
    n_bad = int(bad.sum())
    if n_bad == 0:
        return []
    flat = int(over.argmax()) if float(over.max()) > 0 else int(torch.nonzero(bad.flatten())[0])
    r, c = divmod(flat, ref.shape[1])
    return ["%s: %d elements in %d rows outside the bar (%s); worst at row %d (%d edges) column %d: got %r, reference %r" % (
        name, n_bad, int(bad.any(1).sum()), bar, r, int(deg[r]), c, float(g64[r, c]), float(want[r, c]))]


# ------------------------------------------------------------------------------------------------ the cases
PAIRS = ((F32, F32), (BF16, BF16), (BF16, F32))             # (x dtype, y dtype) the kernels are instantiated for
# width -> lanes per row (4-element fp32 / 8-element bf16 vectors, the next power of two from 4 to 64).  Per class one width that
# fills the row's vectors and one with a ragged last vector AND idle lanes; the widest also with a second block column (grid_y = 2).
LANES = {F32: {3: 4, 16: 4, 29: 8, 32: 8, 47: 16, 64: 16, 100: 32, 128: 32, 131: 64, 300: 64},
         BF16: {7: 4, 32: 4, 33: 8, 64: 8, 100: 16, 128: 16, 203: 32, 256: 32, 523: 64}}
GRID_Y = {(F32, 300): 2, (BF16, 523): 2}

# The kernel of a launch as test_spmm_choice_host.what() shows it, without the lanes: (kernel, slots per row, unroll, prefetch)
KERNELS = {"W": (0, 0, 4, 0), "W2": (0, 0, 2, 0), "W8": (0, 0, 8, 0), "WP": (0, 0, 4, 1), "S": (1, 1, 4, 0), "G2": (2, 2, 4, 0),
           "G4": (2, 4, 4, 0), "F": (3, 0, 4, 0)}
_BAND = {(BF16, 8): ("G2", "W"), (BF16, 16): ("G2", "W")}          # 24 < edges per row <= 64: the row-group band, plain forms only
_FLAT32 = {(F32, 16): ("F", "F"), (F32, 32): ("F", "F")}
_WIDE = lambda k: {(d, lanes): (k, k) for d in (F32, BF16) for lanes in (32, 64)}           # noqa: E731

KnobSet = collections.namedtuple("KnobSet", "knobs plan_knobs graph kernels widths")
# name -> (dgll_hip_debug_tune keys for the launch, keys read when the plan is created, graph, {(x dtype, lanes): (kernel of the plain
# forms, of the accumulate / gate forms)} -- "W", "W" where not listed --, {x dtype: widths}).  None: every width of LANES.
KNOB_SETS = {
    "default": KnobSet({}, {}, "sweep", {**_BAND, **_FLAT32}, None),
    "rowslot": KnobSet(dict(k5=2), {}, "sweep", {(d, lanes): ("S", "S") for d in (F32, BF16) for lanes in (4, 8, 16, 32)},
                       {F32: (3, 16, 29, 32, 47, 64, 100, 128), BF16: (7, 32, 33, 64, 100, 128, 203, 256)}),
    "wave": KnobSet(dict(k5=1, k13=1, k15=1), {}, "sweep", {}, None),
    "rowgroup2": KnobSet(dict(k15=2), {}, "sweep", _BAND, {BF16: (33, 64, 100, 128)}),
    "rowgroup4": KnobSet(dict(k15=4), {}, "sweep", {(BF16, 8): ("G4", "W")}, {BF16: (33, 64)}),
    "flat": KnobSet(dict(k13=2), {}, "sweep", {**_FLAT32, (BF16, 32): ("F", "F"), (BF16, 16): ("G2", "F")},
                    {F32: (47, 64, 100, 128), BF16: (100, 128, 203, 256)}),
    "flat-nogroup": KnobSet(dict(k13=2, k15=1), {}, "sweep", {(BF16, 16): ("F", "F")}, {BF16: (100, 128)}),
    "unroll2": KnobSet(dict(k0=2, k5=1), {}, "sweep", _WIDE("W2"), {F32: (100, 128, 131, 300), BF16: (203, 256, 523)}),
    "unroll8": KnobSet(dict(k0=8, k5=1), {}, "sweep", _WIDE("W8"), {F32: (100, 128, 131, 300), BF16: (203, 256, 523)}),
    "prefetch": KnobSet(dict(k2=4, k5=1), {}, "sweep", {(BF16, 32): ("WP", "WP")}, {BF16: (203, 256)}),
    # the same instantiations on another schedule
    "rpw1": KnobSet(dict(k1=1), {}, "sweep", {**_BAND, **_FLAT32}, {F32: (29, 131), BF16: (64, 256)}),
    "rpw3": KnobSet(dict(k1=3), {}, "sweep", {**_BAND, **_FLAT32}, {F32: (29, 131), BF16: (64, 256)}),
    "xcd": KnobSet(dict(k2=1, k1=1), {}, "sweep", {}, {F32: (29, 300), BF16: (33, 256)}),      # 276 row blocks: the remap's tail
    "flat64": KnobSet(dict(k13=2, k15=1), dict(k14=64), "sweep", {**_FLAT32, (BF16, 16): ("F", "F"), (BF16, 32): ("F", "F")},
                      {F32: (47, 100), BF16: (128, 256)}),
    "block": KnobSet({}, {}, "block", _BAND, {F32: (16, 100, 300), BF16: (33, 128, 256, 523)}),
}
UNALIGNED_FORMS = ("P1", "E1")      # X one element off 16-byte alignment: one element per lane, 64 lanes per row; "default" only


def _runs():
    for name, ks in KNOB_SETS.items():
        for xd, yd in PAIRS:
            if name == "prefetch" and yd != BF16:                   # the prefetch variant exists for bf16 / bf16 only
                continue
            for width in (LANES[xd] if ks.widths is None else ks.widths.get(xd, ())):
                yield name, xd, yd, width


RUNS = list(_runs())                 # one GPU test each
Case = collections.namedtuple("Case", "knobs x_dtype y_dtype width weighted form aligned graph")


def run_cases(name, xd, yd, width):
    """The launches of one run: weighted x every form, and for "default" the unaligned forms on top."""
    graph = KNOB_SETS[name].graph
    out = [Case(name, xd, yd, width, weighted, form, True, graph) for weighted in (False, True) for form in FORMS]
    if name == "default":
        out += [Case(name, xd, yd, width, weighted, form, False, graph) for weighted in (False, True) for form in UNALIGNED_FORMS]
    return out


CASES = [case for run in RUNS for case in run_cases(*run)]


def expected_kernel(case):
    """(kernel, lanes per row, slots per row, unroll, prefetch, elements per lane, grid_y) of the case, from the tables above."""
    if not case.aligned:
        return (0, 64, 0, 4, 0, 1, -(-case.width // 64))
    lanes = LANES[case.x_dtype][case.width]
    plain, extra = KNOB_SETS[case.knobs].kernels.get((case.x_dtype, lanes), ("W", "W"))
    kernel = KERNELS[extra if case.form in EXTRA_FORMS else plain]
    return (kernel[0], lanes) + kernel[1:] + (8 if case.x_dtype == BF16 else 4, 1 if kernel[0] == 2 else GRID_Y.get((case.x_dtype, case.width), 1))


def run_id(run):
    name, xd, yd, width = run
    return "%s-%s-%d" % (name, {(F32, F32): "fp32", (BF16, BF16): "bf16", (BF16, F32): "bf16to32"}[(xd, yd)], width)
