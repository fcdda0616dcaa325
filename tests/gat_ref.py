"""The float64 reference of the second-generation GAT passes (csrc/gat_kernel.hpp), the graph they are swept on and the table of
cases: shared by test_gat_ref_host.py (which pins all three without a GPU) and test_gat_geometry_gpu.py.

`gat_reference` is sparseGatConv's formula (gatconv.py:111-148) per edge in plain torch on the CPU; the gradients are
torch.autograd's.  Nothing here touches a device or any part of dgll_amd."""
import functools

import numpy as np
import torch

F32, BF16 = 0, 1            # DGLL_F32, DGLL_BF16 (include/dgll_hip.h)
ALPHA = 0.2


# ------------------------------------------------------------------------------------------------ the reference
def gat_reference(rowptr, col, h, s, t, heads, alpha, apply_elu, A=None):
    """out [n_rows, heads * fo] of sparseGatConv's aggregation over the CSR (rowptr, col): per edge (i, j) and head
    w = exp(-leaky_relu(s_i + t_j)), out_i = act(sum_j w h_j / sum_j w).  h: [n_cols, heads * fo]; s: [n_rows, heads]; t: [n_cols, heads].
    A [heads * fo, 2 * heads] given: the scores are formed as h @ A instead (s, t ignored): its rows [:n_rows] and columns [:heads]
    are s, all rows and columns [heads:] are t.  Everything in the dtype of h (float64 in the tests); differentiable."""
    n_rows = rowptr.numel() - 1
    row = torch.repeat_interleave(torch.arange(n_rows), rowptr[1:] - rowptr[:-1])
    colv = col.long()
    if A is not None:
        st = h @ A
        s, t = st[:n_rows, :heads], st[:, heads:]
    fo = h.shape[1] // heads
    outs = []
    for k in range(heads):          # one head at a time: the per-edge tensors are [nnz, fo]
        w = torch.exp(-torch.nn.functional.leaky_relu(s[row, k] + t[colv, k], alpha))
        den = torch.zeros(n_rows, dtype=h.dtype).index_add_(0, row, w)
        num = torch.zeros(n_rows, fo, dtype=h.dtype).index_add_(0, row, w[:, None] * h[colv, k * fo:(k + 1) * fo])
        hp = num / den[:, None]
        outs.append(torch.nn.functional.elu(hp) if apply_elu else hp)
    return torch.cat(outs, 1)


def gat_reference_grads(rowptr, col, h, s, t, heads, alpha, apply_elu, gout, A=None):
    """{"out", "grad_h", "grad_s", "grad_t"} (explicit scores) or {"out", "grad_h", "grad_A"} (A given) in float64, detached."""
    h = h.detach().double().requires_grad_()
    if A is None:
        s, t = s.detach().double().requires_grad_(), t.detach().double().requires_grad_()
        leaves, names = (h, s, t), ("grad_h", "grad_s", "grad_t")
    else:
        A = A.detach().double().requires_grad_()
        leaves, names = (h, A), ("grad_h", "grad_A")
    out = gat_reference(rowptr, col, h, s, t, heads, alpha, apply_elu, A=A)
    res = dict(zip(names, torch.autograd.grad(out, leaves, gout.double())))
    res["out"] = out.detach()
    return res


# ------------------------------------------------------------------------------------------------ the sweep graph
N_ROWS, N_COLS = 531, 760
USED_COLS = 750             # columns 750 .. 759 are referenced by no row
# row -> its exact number of entries.  The plan's long-row threshold is 256 and chunks are cut every 256 entries: 257 and 513 both
# leave a one-entry chunk.  Rows 5, 6, 7 hold {5}, {5, 6}, {5, 6, 7}: self-loop, the column every row has, and nothing random.
SPECIAL_ROWS = {0: 700, 5: 1, 6: 2, 7: 3, 40: 63, 41: 64, 42: 65, 80: 127, 81: 128, 82: 129, 120: 255, 121: 256, 122: 257, 530: 513}
HUB, COL_257, COL_256 = 5, 6, 7      # columns with in-degree 531 (every row), exactly 257 and exactly 256


@functools.lru_cache(maxsize=None)
def sweep_graph():
    """(rowptr int64 [532], col int32 [nnz]) of the 531 x 760 sweep adjacency, whose rows are its first 531 columns; columns sorted
    and distinct within a row.  Every row holds its self-loop and column 5; column 6 sits in 257 rows, column 7 in 256; the rows of
    SPECIAL_ROWS have exactly those lengths, every other row has 1 to 8 random columns on top of its fixed ones."""
    rng = np.random.RandomState(20240531)
    others = np.array([r for r in range(N_ROWS) if r not in (5, 6, 7)])
    in_257 = {6, 7} | set(rng.permutation(others)[:255].tolist())
    in_256 = {7} | set(rng.permutation(others)[:255].tolist())
    pool = np.array([c for c in range(USED_COLS) if c not in (HUB, COL_257, COL_256)])
    rows = []
    for r in range(N_ROWS):
        fixed = {r, HUB} | ({COL_257} if r in in_257 else set()) | ({COL_256} if r in in_256 else set())
        extra = SPECIAL_ROWS[r] - len(fixed) if r in SPECIAL_ROWS else int(rng.randint(1, 9))
        assert extra >= 0
        free = pool[~np.isin(pool, list(fixed))]
        rows.append(sorted(fixed | set(rng.permutation(free)[:extra].tolist())))
    rowptr = torch.tensor([0] + list(np.cumsum([len(r) for r in rows])), dtype=torch.int64)
    col = torch.tensor([c for r in rows for c in r], dtype=torch.int32)
    return rowptr, col


# ------------------------------------------------------------------------------------------------ the cases
# (dtype, heads, fo, lpr, nh, grid_y): what gat_choose() gives every pass of the case with compact, 16-byte aligned scores.  The base
# cases reach each of the 19 (lpr, nh) pairs once per dtype, with grid_y = 1 and idle lanes inside a head.
_F32_BASE = [(1, 4, 4, 1), (2, 4, 4, 2), (4, 4, 4, 4),
             (1, 20, 8, 1), (2, 12, 8, 2), (4, 8, 8, 4), (8, 4, 8, 8),
             (1, 36, 16, 1), (2, 20, 16, 2), (4, 12, 16, 4), (8, 8, 16, 8),
             (1, 68, 32, 1), (2, 36, 32, 2), (4, 20, 32, 4), (8, 12, 32, 8),
             (1, 132, 64, 1), (2, 68, 64, 2), (4, 36, 64, 4), (8, 20, 64, 8)]
BASE_CASES = ([(F32, heads, fo, lpr, nh, 1) for heads, fo, lpr, nh in _F32_BASE] +
              [(BF16, heads, 2 * fo, lpr, nh, 1) for heads, fo, lpr, nh in _F32_BASE])
EXTRA_CASES = [
    (BF16, 3, 24, 8, 2, 2), (F32, 5, 8, 4, 2, 3), (BF16, 7, 8, 4, 2, 4),            # a ragged last head block
    (F32, 12, 8, 8, 4, 3), (BF16, 16, 16, 16, 8, 2), (F32, 16, 4, 8, 8, 2),          # several column blocks
    (BF16, 8, 32, 32, 8, 1), (BF16, 1, 64, 8, 1, 1), (F32, 2, 256, 64, 1, 2),        # no idle lane in a head
    (F32, 72, 4, 8, 8, 9),                                                           # more than 64 heads: the workgroup finalize kernel
    (F32, 5, 256, 64, 1, 5),                                                         # one row per wavefront
]
CASES = BASE_CASES + EXTRA_CASES
ALL_PAIRS = sorted([(lpr, nh) for lpr in (4, 8, 16, 32, 64) for nh in (1, 2, 4)] + [(lpr, 8) for lpr in (8, 16, 32, 64)])


def case_id(case):
    return "%s-%dx%d" % ("bf16" if case[0] == BF16 else "fp32", case[1], case[2])


def torch_dtype(case):
    return torch.bfloat16 if case[0] == BF16 else torch.float32


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """{"h", "s", "t", "A", "gout"} as fp32 CPU tensors from a generator seeded by the case; for a bf16 case h, A and gout hold
    bf16-representable values (s and t of the explicit-score form stay fp32 values).  A is block-diagonal: column k holds a1 of head
    k in rows k fo .. (k + 1) fo, column heads + k its a2."""
    dtype, heads, fo = case[:3]
    gen = torch.Generator().manual_seed(1000003 * dtype + 1009 * heads + fo)
    rnd = lambda *shape: torch.randn(*shape, generator=gen)        # noqa: E731
    h = 0.5 * rnd(N_COLS, heads * fo)
    s, t = 0.5 * rnd(N_ROWS, heads), 0.5 * rnd(N_COLS, heads)
    A = torch.zeros(heads * fo, 2 * heads)
    for k in range(heads):
        A[k * fo:(k + 1) * fo, k] = 0.3 * rnd(fo)
        A[k * fo:(k + 1) * fo, heads + k] = 0.3 * rnd(fo)
    gout = rnd(N_ROWS, heads * fo)
    if dtype == BF16:
        h, A, gout = (v.to(torch.bfloat16).float() for v in (h, A, gout))
    return dict(h=h, s=s, t=t, A=A, gout=gout)


@functools.lru_cache(maxsize=None)
def case_reference(case, apply_elu, with_A):
    """gat_reference_grads of the case on the sweep graph, computed once per (case, apply_elu, form of the scores)."""
    rowptr, col = sweep_graph()
    x = case_inputs(case)
    return gat_reference_grads(rowptr, col, x["h"], x["s"], x["t"], case[1], ALPHA, apply_elu, x["gout"], A=x["A"] if with_A else None)


# ------------------------------------------------------------------------------------------------ the bars
def check(name, got, want, dtype, form_a=False):
    """Hold `got` against the float64 `want` at the bar of its quantity; returns the violations as a list of strings (empty: inside)
    after printing the measured error.
    fp32: forward elementwise rtol 1e-4, atol 1e-5; every gradient elementwise rtol 2e-3, atol 2e-4 (test_ops_gpu.py).
    bf16 forward of the compact-score aggregation (form_a): |got - want| <= 2^-8 |want| + 1e-4 max|want| -- fp32 accumulation, one
    round-to-nearest-even store (half a bf16 step is at most 2^-8 of the value), and the fp32 forward bar for the order of the sums
    and the ELU's exp - 1.  bf16 otherwise: forward max|err| <= 2e-2 max|want|, every gradient relative L2 <= 1.5e-2."""
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if not bool(torch.isfinite(got).all()):
        return ["%s: not finite" % name]
    err = (got - want).abs()
    top = float(want.abs().max())
    err_max = float(err.max()) / top
    err_l2 = float((got - want).norm() / want.norm())
    forward = name.endswith("out")
    if dtype == torch.float32:
        rtol, atol = (1e-4, 1e-5) if forward else (2e-3, 2e-4)
        worst = float((err / (atol + rtol * want.abs())).max())
        bar, ok = "elementwise rtol %.0e atol %.0e" % (rtol, atol), worst <= 1.0
    elif forward and form_a:
        worst = float((err / (2.0 ** -8 * want.abs() + 1e-4 * top)).max())
        bar, ok = "elementwise 2^-8 |ref| + 1e-4 max|ref|", worst <= 1.0
    elif forward:
        worst, bar = err_max / 2e-2, "max|err| <= 2e-2 max|ref|"
        ok = worst <= 1.0
    else:
        worst, bar = err_l2 / 1.5e-2, "relative L2 <= 1.5e-2"
        ok = worst <= 1.0
    print("%-28s max/max %.3e  rel-l2 %.3e  of the bar %.3f  (%s)" % (name, err_max, err_l2, worst, bar))
    return [] if ok else ["%s: %.3f of the bar (%s); max/max %.3e, rel-l2 %.3e" % (name, worst, bar, err_max, err_l2)]
