"""The sweep of the passes on csrc/row_tiles.hpp that carry heads: the graph, the table of lane geometries, operands whose attention
weights are known in closed form, float64 references with per-edge tensors, and the comparators.  test_rowtile_ref_host.py pins all
of it without a GPU, test_rowtile_geometry_gpu.py runs it on the card, the two emulated files run the closed-form legs on the source.

GEOMETRY.  make_head_geometry(heads, D, epv, n_rows) gives a launch (lph, lpr): lph = lanes of a head (the power of two at or above
vph = D / epv), hpb = min(64 / lph, heads) whole heads in a row's lanes, lpr = the power of two at or above max(hpb * lph, 8),
col_blocks = ceil(heads / hpb), tiles of 4 * 64 / lpr rows.  lph in 1 .. 64 and lpr in 8 .. 64 with lpr >= lph: 22 pairs.  TABLE
holds one base case per pair (the same (heads, vph) for fp32 and bf16, D = vph * epv), alternately one that fills its lanes and one
that leaves lanes idle (vph < lph, hpb * lph < lpr), and three extras with 2, 2 and 3 column blocks, two of them ragged.

GRAPH.  sweep_graph(): 307 x 760 (307 = 4 * 76 + 3: a ragged last tile at 4, 8, 16 and 32 rows a tile).  Rows 0 and 306 are empty;
rows of 1, 2, 3, 7 .. 9, 15 .. 17, 31 .. 33, 63 .. 65, 255 .. 257 (LONG_ROW = 256 is still swept inline), 511 .. 513 and 700 entries
have distinct columns -- which is why there are 760 columns and not about 400: 700 distinct ones and ten nobody references need 710;
rows 4 .. 7 are a short, an empty, a long (257) and a short row, a pattern every tile size keeps in one tile; rows 6 and 20 are two
long rows of one 32-row tile; Poisson(6) rows with distinct columns elsewhere, row 290 with one column five times.  Column 1 is in
every non-empty row, column 2 in exactly 257 rows, column 3 in exactly 256: the transposed passes meet two long rows and the
threshold.  Column 0 and columns 751 .. 759 are referenced by nobody.  emu_graph() is the cut-down 13 x 420 form for the emulator.

LEGS (sparse attention; the GATv2 form in brackets).
 * flat: alpha_ij = 1 / deg_i.  scale = 1/8; q[i, h, :] = c_ih in every column, a non-zero integer in [-4, 4] that differs by row
   and head; k[j, h, :] is a per-source permutation of one integer vector per head, so its sum over the head is the same kappa_h in
   1 .. 4 for every j; v and g are non-zero integers in [-4, 4].  Every score of a row is the same exactly representable number
   (|s| <= 2): the running maximum never moves after the first entry, every weight is exp2(0), l = deg and acc = sum v exactly.
   (GATv2: attn[h, :] a power of two <= 1 / D, slope 1/4, xl a permutation per source of one vector of integers in 0 .. 3 per head;
   even rows xr in 1 .. 2, so every z > 0; odd rows xr in -6 .. -4, so every z < 0 and lrelu(z) = z / 4 exactly.)  `zero`: the same
   with q = 0 (attn = 0), for which dk (dxr and the score part of dxl) must be exactly 0.
 * onehot: alpha_ij in {0, 1}, forward only.  scale = 1, q = 128 everywhere, k[j, h, :] holds pi_h(j) = 16 a + b (b < 16) as 16 a in
   column j mod D and b in column (j + 1) mod D, with pi_h an affine permutation of the source ids that differs by head (pi_0 is the
   identity); v is randn rounded to the dtype.  Scores of distinct sources differ by at least 128 nats = 184 in the kernel's log2
   units: every weight but the winner's is exp2 of less than -150, 0 in fp32 with or without denormals, every rescale is by 0 or 1,
   and out[i, h] must EQUAL v[winner_ih, h] in any sweep order.  The rows of 9, 17, 33, 65, 257 and 513 entries end with the largest
   column (head 0's winner: a one-entry tail batch), those of 255 and 511 begin with it.  A (row, head) whose winner is the column
   row 290 holds five times is excluded (l = 5, and 5 * (1 / 5) is not 1).  (GATv2: xr = 0, attn = 128, xl carries pi and is the
   value.)
 * random: randn rounded to the dtype, as in test_sparse_attn_gpu.py and test_gatv2_gpu.py.
 * mp (U_MUL_E_SUM over A and A^T, U_DOT_V): x, y integers in [-4, 4], weights multiples of 1/4 in [-2, 2]; every sum is exact in
   fp32 (max_row sum |w| * max |x| * 4 < 2^24, asserted): the outputs must EQUAL the float64 result.

REFERENCES.  attn_reference() and gatv2_reference() write the forward and every gradient out edge by edge in float64 (held to
autograd of attn_ref.sparse_attention_reference and test_gatv2_host.gatv2_reference by the host test).  Next to each result they
return its scale -- per entry, the sum of the absolute values of the per-edge terms the entry sums, with |d_ij| + sum_j alpha |d_ij|
standing for |d_ij - delta_i| -- and the bar of the flat backward in units of 2^-23.

BARS.
 * onehot forward: torch.equal; lse within 2^-22 |s| of the winning score (log2e and ln2 rounded once each, two rounded products).
 * flat forward: |out - S / deg| <= 2^-21 |S| / deg (1.0f / l within 2.5 ulp, the product and the store half an ulp each: the mean
   bar of the SpMM sweep), plus 2^-8 |S / deg| for a bf16 output; lse within 2^-21 (|s| + ln deg).  No atol.
 * flat backward: |err| <= 2^-23 sum_t K_t |term_t| over the per-edge terms t of the entry, plus 2^-8 |ref| for a bf16 output, with
   K_t = n + n_delta(t) + 2 E_t + 4 (dv, and delta itself: K_t = n + E_t + 2).  Derivation, in units of 2^-23 = one fp32 ulp of 1:
     - n, the entry's term count: an fmaf chain of n terms (and the adds of the long-row merge) rounds n times by half an ulp of a
       partial sum that never exceeds the scale: n / 2, counted as n;
     - E_t = 3 |s| log2e + log2 deg + 2 bounds the relative error eps of alpha_t = exp2(fma(p, sl2, -lse log2e)) against 1 / deg:
       the forward's m = fl(p sl2) (the rounded constant sl2 cancels: the backward's fma forms the same product exactly) and the
       round trip lse = (m + log2 l) ln2, then lse log2e -- two rounded constants, two rounded products -- move the exponent by at
       most 2.5 |s| log2e ulp, times ln 2 to reach alpha: 1.8 |s| log2e <= 3 |s| log2e; the log2 deg and 2 stand for the errors of
       log2 l, of the sum and of the exp2 itself.  (Every step at its worst case at once would make the middle term 2.8 log2 deg;
       the bar keeps the smaller figure, so a fraction above 1 asks for a look at the kernel and at this line, not for a larger K.)
     - alpha_t enters a term through two products (alpha d, then that times the operand): + 1, counted as 2;
     - the bilinear results (dq, dk, dxr, dxl, dattn) use delta_i, itself a sum of n_delta(t) = deg_i terms with the same alpha
       errors, against |d_ij| + sum_j alpha |d_ij| of the scale: + n_delta(t) + E_t + 2.
 * random: the project's bars unchanged (fp32 1e-4 / 2e-3 of max|ref|, bf16 2e-2 of max|ref| / 1.5e-2 relative L2); the largest
   |err| / scale per quantity is recorded for a later tightening.
 * every leg: rows of unreferenced sources and empty rows exactly 0 (lse = 0), a second launch bit-identical, every output finite.
"""
import math
from collections import namedtuple

import numpy as np
import torch

F32, BF16 = torch.float32, torch.bfloat16
LONG_ROW = 256
LOG2E = 1.4426950408889634
N_ROWS, N_COLS = 307, 760
HUBS = (1, 2, 3)                                        # in every non-empty row, in exactly 257 rows, in exactly 256 rows
UNREFERENCED = (0,) + tuple(range(751, 760))
SPECIAL = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 700)
WINNER_LAST, WINNER_FIRST = (9, 17, 33, 65, 257, 513), (255, 511)
DUP_ROW = 290
EMU_SPECIAL = (1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 400)


def epv(dtype):
    return 4 if dtype == F32 else 8


# ---- the table ---------------------------------------------------------------------------------------------------------------------
Geometry = namedtuple("Geometry", "vph lph hpb lpr col_blocks")
Case = namedtuple("Case", "dtype heads D geo")

# (heads, D fp32, D bf16, (vph, lph, hpb, lpr, col_blocks)): the 22 (lph, lpr) pairs in lph-major order, then the extras
TABLE = [
    (5, 4, 8, (1, 1, 5, 8, 1)), (16, 4, 8, (1, 1, 16, 16, 1)), (17, 4, 8, (1, 1, 17, 32, 1)), (64, 4, 8, (1, 1, 64, 64, 1)),
    (3, 8, 16, (2, 2, 3, 8, 1)), (8, 8, 16, (2, 2, 8, 16, 1)), (9, 8, 16, (2, 2, 9, 32, 1)), (32, 8, 16, (2, 2, 32, 64, 1)),
    (2, 12, 24, (3, 4, 2, 8, 1)), (3, 16, 32, (4, 4, 3, 16, 1)), (8, 12, 24, (3, 4, 8, 32, 1)), (9, 16, 32, (4, 4, 9, 64, 1)),
    (1, 20, 40, (5, 8, 1, 8, 1)), (2, 32, 64, (8, 8, 2, 16, 1)), (3, 28, 56, (7, 8, 3, 32, 1)), (8, 32, 64, (8, 8, 8, 64, 1)),
    (1, 36, 72, (9, 16, 1, 16, 1)), (2, 64, 128, (16, 16, 2, 32, 1)), (3, 52, 104, (13, 16, 3, 64, 1)),
    (1, 68, 136, (17, 32, 1, 32, 1)), (2, 128, 256, (32, 32, 2, 64, 1)),
    (1, 132, 264, (33, 64, 1, 64, 1)),
    (33, 8, 16, (2, 2, 32, 64, 2)),                     # two column blocks, the second with one head of 32
    (5, 64, 128, (16, 16, 4, 64, 2)),                   # hpb = 4, the second block with one of four heads
    (3, 256, 512, (64, 64, 1, 64, 3)),                  # three column blocks of one full-width head
]
CASES = [Case(dt, h, (d32 if dt == F32 else d16), Geometry(*geo)) for dt in (F32, BF16) for h, d32, d16, geo in TABLE]


def case_id(case):
    return "%s-%dx%d" % ("fp32" if case.dtype == F32 else "bf16", case.heads, case.D)


def head_geometry(heads, D, epv_, n_rows):
    """make_head_geometry of csrc/row_tiles.hpp, restated: (Geometry, tiles)."""
    def pow2_at_least(n, start):
        while start < n:
            start <<= 1
        return start
    vph = D // epv_
    lph = pow2_at_least(vph, 1)
    hpb = min(64 // lph, heads)
    lpr = pow2_at_least(hpb * lph, 8)
    groups = 4 * (64 // lpr)
    return Geometry(vph, lph, hpb, lpr, -(-heads // hpb)), -(-n_rows // groups)


# ---- the graphs --------------------------------------------------------------------------------------------------------------------
class Graph:
    """rows: the column lists as the CSR keeps them (duplicates are separate entries); special: entry count -> row."""

    def __init__(self, rows, n_cols, special, dup_row, dup_col, unreferenced):
        self.rows, self.n_rows, self.n_cols = rows, len(rows), n_cols
        self.special, self.dup_row, self.dup_col, self.unreferenced = special, dup_row, dup_col, unreferenced
        self.deg = np.array([len(r) for r in rows], dtype=np.int64)
        self.rowptr = torch.tensor([0] + list(np.cumsum(self.deg)), dtype=torch.int64)
        self.col = torch.tensor([int(c) for r in rows for c in r], dtype=torch.int32)
        self.nnz = int(self.col.numel())
        self.row = torch.repeat_interleave(torch.arange(self.n_rows), torch.from_numpy(self.deg))
        self.indeg = np.bincount(self.col.numpy(), minlength=n_cols).astype(np.int64)

    def transposed_rows(self):
        out = [[] for _ in range(self.n_cols)]
        for i, r in enumerate(self.rows):
            for c in r:
                out[c].append(i)
        return out

    def csr(self, device="cpu"):
        from dgll_amd import CSRGraph

        return CSRGraph(self.rowptr, self.col, None, self.n_rows, self.n_cols).to(device)

    def without_last_entry(self, row):
        rows = [list(r) for r in self.rows]
        rows[row].pop()
        return Graph(rows, self.n_cols, self.special, self.dup_row, self.dup_col, self.unreferenced)

    def with_last_entry_twice(self, row):
        rows = [list(r) for r in self.rows]
        rows[row].append(rows[row][-1])
        return Graph(rows, self.n_cols, self.special, self.dup_row, self.dup_col, self.unreferenced)


def _build(n_rows, n_cols, placed, hubs, quotas, unreferenced, dup_row, seed):
    rng = np.random.RandomState(seed)
    pool = np.array([c for c in range(n_cols) if c not in hubs and c not in unreferenced])
    left = list(quotas)
    rows, dup_col = [], None
    for r in range(n_rows):
        if r in placed:
            n = placed[r]
        elif r == 0 or r == n_rows - 1:
            n = 0
        elif r == dup_row:
            n = 5
        else:
            n = int(rng.poisson(6))
        cols = []
        for k, hub in enumerate(hubs):                  # hub k goes to the first quota_k rows of more than k entries
            if n > k and (left[k] is None or left[k] > 0):
                cols.append(hub)
                left[k] = None if left[k] is None else left[k] - 1
        cols += [int(c) for c in rng.choice(pool, n - len(cols), replace=False)]
        cols = [cols[p] for p in rng.permutation(len(cols))]
        if r in placed and (n in WINNER_LAST or n in WINNER_FIRST):      # the largest column (head 0's winner) goes last / first
            top = max(cols)
            cols.remove(top)
            cols = cols + [top] if n in WINNER_LAST else [top] + cols
        rows.append(cols)
    if dup_row is not None:
        dup_col = next(c for c in rows[dup_row] if c not in hubs)
        rows[dup_row] = rows[dup_row] + [dup_col] * 4
    assert all(q in (None, 0) for q in left), left
    return rows, dup_col


_cache = {}


def sweep_graph():
    if "sweep" not in _cache:
        placed = {4: 3, 5: 0, 6: 257, 7: 2, 20: 511}
        rest = [n for n in SPECIAL if n not in (3, 257, 2, 511)]
        placed.update({30 + 14 * k: n for k, n in enumerate(rest)})
        rows, dup_col = _build(N_ROWS, N_COLS, placed, HUBS, (None, LONG_ROW + 1, LONG_ROW), UNREFERENCED, DUP_ROW, 307)
        _cache["sweep"] = Graph(rows, N_COLS, {n: r for r, n in placed.items()}, DUP_ROW, dup_col, UNREFERENCED)
    return _cache["sweep"]


def emu_graph():
    """13 x 420: an empty row, rows of 1, 7 .. 9, 63 .. 65, 255 .. 257 and 400 entries (distinct columns), an empty row; sources 0 and
    411 .. 419 are referenced by nobody."""
    if "emu" not in _cache:
        placed = {k + 1: n for k, n in enumerate(EMU_SPECIAL)}
        unref = (0,) + tuple(range(411, 420))
        rows, _ = _build(len(EMU_SPECIAL) + 2, 420, placed, (), (), unref, None, 12)
        _cache["emu"] = Graph(rows, 420, {n: r for r, n in placed.items()}, None, None, unref)
    return _cache["emu"]


def tile_has_pattern(graph, groups):
    """Some tile of `groups` rows holds a short, an empty, a long and a short row, adjacent and in that order."""
    d = graph.deg
    for r in range(graph.n_rows - 3):
        if r // groups == (r + 3) // groups and 0 < d[r] <= LONG_ROW and d[r + 1] == 0 and d[r + 2] > LONG_ROW and 0 < d[r + 3] <= LONG_ROW:
            return True
    return False


# ---- operands ----------------------------------------------------------------------------------------------------------------------
def _ints(gen, shape, lo, hi, nonzero=False):
    x = torch.randint(lo, hi + 1, shape, generator=gen).double()
    if nonzero:
        x = torch.where(x == 0, torch.full_like(x, float(hi)), x)
    return x


def _permuted(gen, base, n):
    """[n, heads, D]: row j holds, per head, its own permutation of base [heads, D]."""
    heads, D = base.shape
    order = torch.rand((n, heads, D), generator=gen).argsort(-1)
    return base.unsqueeze(0).expand(n, heads, D).gather(-1, order)


def permutation(n, head):
    """pi_head(j) = (m j + c) mod n with the head-th multiplier coprime to n (head 0: the identity), as an int64 array."""
    m, seen = 0, -1
    while seen < head:
        m += 1
        seen += math.gcd(m, n) == 1
    return (m * np.arange(n, dtype=np.int64) + 37 * head) % n


def _onehot_keys(n, heads, D):
    k = torch.zeros((n, heads, D), dtype=torch.float64)
    j = torch.arange(n)
    for h in range(heads):
        pi = torch.from_numpy(permutation(n, h))
        k[j, h, j % D] = (pi // 16 * 16).double()
        k[j, h, (j + 1) % D] = (pi % 16).double()
    return k


def _seed(case, leg):
    return case.heads * 1000 + case.D + {"flat": 1, "zero": 2, "onehot": 3, "random": 4, "mp": 5}[leg] * 100003


def attn_operands(graph, case, leg, shared=False):
    """q, k, v, g as [n, heads * D] CPU tensors of case.dtype, and the scale; shared: v is k."""
    dt, heads, D = case.dtype, case.heads, case.D
    gen = torch.Generator().manual_seed(_seed(case, leg))
    nd, ns = graph.n_rows, graph.n_cols
    if leg in ("flat", "zero"):
        scale = 0.125
        c = _ints(gen, (nd, heads), 1, 4) * (1 - 2 * _ints(gen, (nd, heads), 0, 1))
        q = c.unsqueeze(-1).expand(nd, heads, D).clone() * (0.0 if leg == "zero" else 1.0)
        base = _ints(gen, (heads, D), -2, 2)
        kappa = (torch.arange(heads) % 4 + 1).double()
        base[:, 0] += kappa - base.sum(-1)              # the first column fixes the head's sum; |it| stays far below 256 (asserted by the host test)
        k = _permuted(gen, base, ns)
        v = _ints(gen, (ns, heads, D), -4, 4, nonzero=True)
        g = _ints(gen, (nd, heads, D), -4, 4, nonzero=True)
    elif leg == "onehot":
        scale = 1.0
        q = torch.full((nd, heads, D), 128.0, dtype=torch.float64)
        k = _onehot_keys(ns, heads, D)
        v = torch.randn((ns, heads, D), generator=gen).double()
        g = torch.randn((nd, heads, D), generator=gen).double()
    else:
        scale = D ** -0.5
        q, k, v, g = (torch.randn((n, heads, D), generator=gen).double() for n in (nd, ns, ns, nd))
    q, k, v, g = (t.reshape(t.shape[0], heads * D).to(dt) for t in (q, k, v, g))
    return q, k, (k if shared else v), g, scale


def gatv2_operands(graph, case, leg):
    """xl, xr, g as [n, heads * D] CPU tensors of case.dtype, attn fp32 [heads, D], and the slope."""
    dt, heads, D = case.dtype, case.heads, case.D
    gen = torch.Generator().manual_seed(_seed(case, leg) + 7)
    nd, ns = graph.n_rows, graph.n_cols
    if leg in ("flat", "zero"):
        slope = 0.25
        a = 2.0 ** -math.ceil(math.log2(D)) * torch.where(torch.arange(heads) % 2 == 0, 1.0, 0.5).double()
        attn = a.unsqueeze(1).expand(heads, D).clone() * (0.0 if leg == "zero" else 1.0)
        xl = _permuted(gen, _ints(gen, (heads, D), 0, 3), ns)
        pos, neg = _ints(gen, (nd, heads, D), 1, 2), _ints(gen, (nd, heads, D), -6, -4)
        xr = torch.where((torch.arange(nd) % 2 == 0).view(nd, 1, 1), pos, neg)
        g = _ints(gen, (nd, heads, D), -4, 4, nonzero=True)
    elif leg == "onehot":
        slope = 0.2
        attn = torch.full((heads, D), 128.0, dtype=torch.float64)
        xl = _onehot_keys(ns, heads, D)
        xr = torch.zeros((nd, heads, D), dtype=torch.float64)
        g = torch.randn((nd, heads, D), generator=gen).double()
    else:
        slope = 0.2
        xl, xr = (torch.randn((n, heads, D), generator=gen).double() for n in (ns, nd))
        attn = torch.randn((heads, D), generator=gen).double() / D ** 0.5
        g = torch.randn((nd, heads, D), generator=gen).double()
    xl, xr, g = (t.reshape(t.shape[0], heads * D).to(dt) for t in (xl, xr, g))
    return xl, xr, attn.float(), g, slope


def mp_operands(graph, case):
    """x [n_src, F], y [n_dst, F] integers in [-4, 4] of case.dtype; w [nnz, heads] fp32 multiples of 1/4 in [-2, 2]."""
    gen = torch.Generator().manual_seed(_seed(case, "mp"))
    F = case.heads * case.D
    x, y = _ints(gen, (graph.n_cols, F), -4, 4).to(case.dtype), _ints(gen, (graph.n_rows, F), -4, 4).to(case.dtype)
    return x, y, (_ints(gen, (graph.nnz, case.heads), -8, 8) / 4).float()


def padded(t, fill=float("nan"), nan_rows=()):
    """t inside a buffer one 16-byte vector wider, `fill` behind its columns and in the rows `nan_rows`: (view, buffer)."""
    vec = 16 // t.element_size()
    buf = torch.full((t.shape[0], -(-t.shape[1] // vec) * vec + vec), fill, dtype=t.dtype, device=t.device)
    view = buf[:, :t.shape[1]]
    view.copy_(t)
    if len(nan_rows):
        buf[list(nan_rows)] = fill
    return view, buf


# ---- references --------------------------------------------------------------------------------------------------------------------
Q = namedtuple("Q", "ref scale units")      # [n, F] float64 each; units: the flat backward's bar in units of 2^-23 (None: no such bar)


def _softmax(graph, s):
    n = graph.n_rows
    idx = graph.row.unsqueeze(1).expand_as(s)
    top = torch.full((n, s.shape[1]), -float("inf"), dtype=torch.float64).scatter_reduce(0, idx, s, "amax")
    w = torch.exp(s - top[graph.row])
    den = torch.zeros((n, s.shape[1]), dtype=torch.float64).index_add_(0, graph.row, w)
    lse = torch.where(den > 0, top + torch.log(den), torch.zeros_like(den))
    return w / den[graph.row], lse


def _sum(idx, n, count, term, term_abs, c):
    """The entries index_add(idx, term) of n rows: Q(ref, sum |term|, count * sum |term| + sum c |term|); c per (edge, head)."""
    shape = (n,) + tuple(term.shape[1:])
    add = lambda t: torch.zeros(shape, dtype=torch.float64).index_add_(0, idx, t)      # noqa: E731
    while c.dim() < term.dim():
        c = c.unsqueeze(-1)
    scale = add(term_abs)
    units = torch.from_numpy(count).double().view((n,) + (1,) * (term.dim() - 1)) * scale + add(c * term_abs)
    return Q(add(term).reshape(n, -1), scale.reshape(n, -1), units.reshape(n, -1))


def _mean(graph, gathered):
    """S / deg [n_rows, F] with S the plain sum of the row's gathered values (exact for the flat leg's integers): its closed form"""
    S = torch.zeros((graph.n_rows,) + tuple(gathered.shape[1:]), dtype=torch.float64).index_add_(0, graph.row, gathered)
    return (S / torch.from_numpy(np.maximum(graph.deg, 1)).double().view(-1, 1, 1)).reshape(graph.n_rows, -1)


def _alpha_error(graph, s):
    """E_t of the module text, per (edge, head)."""
    deg = torch.from_numpy(graph.deg).double()[graph.row].unsqueeze(1)
    return 3 * s.abs() * LOG2E + torch.log2(deg) + 2


def attn_reference(graph, q, k, v, g, heads, scale):
    """out, dq, dk, dv, delta as Q; mean (see _mean); lse [n_dst, heads], s and alpha [nnz, heads]."""
    D = q.shape[1] // heads
    q3, k3, v3, g3 = (t.double().view(-1, heads, D) for t in (q, k, v, g))
    row, col, nd, ns = graph.row, graph.col.long(), graph.n_rows, graph.n_cols
    s = (q3[row] * k3[col]).sum(-1) * scale
    alpha, lse = _softmax(graph, s)
    E = _alpha_error(graph, s)
    degr = torch.from_numpy(graph.deg).double()[row].unsqueeze(1)
    a = alpha.unsqueeze(-1)
    res = {"lse": lse, "s": s, "alpha": alpha}
    res["out"] = _sum(row, nd, graph.deg, a * v3[col], a * v3[col].abs(), E + 2)
    res["mean"] = _mean(graph, v3[col])
    d = (g3[row] * v3[col]).sum(-1)
    res["delta"] = _sum(row, nd, graph.deg, alpha * d, alpha * d.abs(), E + 2)
    dd = d - res["delta"].ref[row]
    dd_abs = d.abs() + res["delta"].scale[row]
    K = degr + 2 * E + 4
    res["dq"] = _sum(row, nd, graph.deg, scale * (alpha * dd).unsqueeze(-1) * k3[col], abs(scale) * (alpha * dd_abs).unsqueeze(-1) * k3[col].abs(), K)
    res["dk"] = _sum(col, ns, graph.indeg, scale * (alpha * dd).unsqueeze(-1) * q3[row], abs(scale) * (alpha * dd_abs).unsqueeze(-1) * q3[row].abs(), K)
    res["dv"] = _sum(col, ns, graph.indeg, a * g3[row], a * g3[row].abs(), E + 2)
    return res


def gatv2_reference(graph, xl, xr, attn, g, heads, slope):
    """out, dxl, dxr, dattn ([1, F]), delta as Q; mean (see _mean); lse [n_dst, heads], s (the logits) and alpha [nnz, heads]."""
    D = attn.shape[1]
    xl3, xr3, g3 = (t.double().view(-1, heads, D) for t in (xl, xr, g))
    at = attn.double().unsqueeze(0)
    row, col, nd, ns = graph.row, graph.col.long(), graph.n_rows, graph.n_cols
    z = xl3[col] + xr3[row]
    sl = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    L = z * sl
    s = (at * L).sum(-1)
    alpha, lse = _softmax(graph, s)
    E = _alpha_error(graph, s)
    degr = torch.from_numpy(graph.deg).double()[row].unsqueeze(1)
    a = alpha.unsqueeze(-1)
    res = {"lse": lse, "s": s, "alpha": alpha}
    res["out"] = _sum(row, nd, graph.deg, a * xl3[col], a * xl3[col].abs(), E + 2)
    res["mean"] = _mean(graph, xl3[col])
    d = (g3[row] * xl3[col]).sum(-1)
    res["delta"] = _sum(row, nd, graph.deg, alpha * d, alpha * d.abs(), E + 2)
    dd = (alpha * (d - res["delta"].ref[row])).unsqueeze(-1)
    dd_abs = (alpha * (d.abs() + res["delta"].scale[row])).unsqueeze(-1)
    K = degr + 2 * E + 4
    res["dxr"] = _sum(row, nd, graph.deg, dd * at * sl, dd_abs * at.abs() * sl, K)
    res["dxl"] = _sum(col, ns, graph.indeg, a * g3[row] + dd * at * sl, a * g3[row].abs() + dd_abs * at.abs() * sl, K)
    res["dattn"] = _sum(torch.zeros_like(row), 1, np.array([graph.nnz]), dd * L, dd_abs * L.abs(), K)
    return res


def winners(graph, s):
    """For one-hot scores s [nnz, heads]: (winner column [n_rows, heads], -1 for an empty row; its multiplicity; the winning score)."""
    n, heads = graph.n_rows, s.shape[1]
    idx = graph.row.unsqueeze(1).expand_as(s)
    top = torch.full((n, heads), -float("inf"), dtype=torch.float64).scatter_reduce(0, idx, s, "amax")
    hit = s == top[graph.row]
    mult = torch.zeros((n, heads), dtype=torch.int64).index_add_(0, graph.row, hit.long())
    win = torch.full((n, heads), -1, dtype=torch.int64)
    e, h = hit.nonzero(as_tuple=True)
    win[graph.row[e], h] = graph.col.long()[e]
    return win, mult, torch.where(mult > 0, top, torch.zeros_like(top))


def onehot_expected(graph, value, win, mult, heads):
    """(out [n_rows, F] of value's dtype: value[winner] per head, 0 for an empty row; keep [n_rows, heads]: False where the winner's
    multiplicity is no power of two)."""
    D = value.shape[1] // heads
    v3 = value.view(-1, heads, D)
    out = torch.zeros((graph.n_rows, heads, D), dtype=value.dtype)
    i, h = (win >= 0).nonzero(as_tuple=True)
    out[i, h] = v3[win[i, h], h]
    keep = (mult & (mult - 1)) == 0
    return out.reshape(graph.n_rows, heads * D), keep


def mp_reference(graph, x, y, w, heads):
    """U_MUL_E_SUM over A (x gathered) and over A^T (y gathered), U_DOT_V, in float64; and max_row sum |w| * max |x| * 4."""
    D = x.shape[1] // heads
    x3, y3, w64 = x.double().view(-1, heads, D), y.double().view(-1, heads, D), w.double()
    row, col = graph.row, graph.col.long()
    fwd = torch.zeros((graph.n_rows, heads, D), dtype=torch.float64).index_add_(0, row, w64.unsqueeze(-1) * x3[col])
    bwd = torch.zeros((graph.n_cols, heads, D), dtype=torch.float64).index_add_(0, col, w64.unsqueeze(-1) * y3[row])
    dots = (x3[col] * y3[row]).sum(-1)
    wsum = max(torch.zeros((graph.n_rows, heads), dtype=torch.float64).index_add_(0, row, w64.abs()).max().item(),
               torch.zeros((graph.n_cols, heads), dtype=torch.float64).index_add_(0, col, w64.abs()).max().item())
    cap = wsum * max(x.double().abs().max().item(), y.double().abs().max().item()) * 4
    return fwd.reshape(graph.n_rows, -1), bwd.reshape(graph.n_cols, -1), dots, cap


# ---- comparators: each returns a list of findings (empty: passed) ---------------------------------------------------------------------
def _bf16_part(got, ref):
    return 2.0 ** -8 * ref.abs() if got.dtype == BF16 else 0.0


def _worst(label, err, bar):
    """findings for err <= bar elementwise (no atol: bar 0 demands err 0), and the largest err / bar"""
    frac = torch.where(bar > 0, err / torch.where(bar > 0, bar, torch.ones_like(bar)), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = frac.max().item() if frac.numel() else 0.0
    if not worst <= 1.0:
        at = np.unravel_index(int(frac.argmax()), frac.shape)
        return ["%s: |err| %.3e is %.2f of the bar at %s" % (label, err[at].item(), worst, tuple(int(i) for i in at))], worst
    return [], worst


def check_finite(label, got):
    return [] if bool(torch.isfinite(got.float()).all()) else ["%s: not finite" % label]


def check_equal(label, got, want, keep=None, heads=None):
    """got EQUALS want cast to got's dtype (one rounding of an exactly known number); keep [n, heads]: the (row, head) pairs compared."""
    want = want.to(got.dtype)
    same = (got == want) | (torch.isnan(got) & torch.isnan(want))
    if keep is not None:
        same = same.view(got.shape[0], heads, -1) | ~keep.unsqueeze(-1)
    bad = int((~same).sum())
    return ["%s: %d entries differ from the exact result" % (label, bad)] if bad else []


def check_flat_forward(label, got, ref):
    """|out - S / deg| <= 2^-21 |S| / deg, plus 2^-8 |S / deg| for a bf16 output: (findings, largest fraction of the bar); ref: the
    references' "mean", S / deg with S summed exactly (S = 0 demands 0)"""
    return _worst(label, (got.double() - ref).abs(), 2.0 ** -21 * ref.abs() + _bf16_part(got, ref))


def check_lse(label, lse, ref_lse, bar):
    """|lse - ref| <= bar elementwise (an empty row: bar 0, lse exactly 0): (findings, largest fraction of the bar)"""
    return _worst(label, (lse.double() - ref_lse).abs(), bar)


def flat_lse_bar(graph, ref):
    """2^-21 (|s| + ln deg) per (row, head) of a flat leg's reference, 0 for an empty row"""
    lndeg = torch.log(torch.from_numpy(np.maximum(graph.deg, 1)).double()).unsqueeze(1)
    return 2.0 ** -21 * ((ref["lse"] - lndeg).abs() + lndeg) * torch.from_numpy(graph.deg > 0).double().unsqueeze(1)


def onehot_lse(top, mult):
    """(the one-hot leg's lse: the winning score, plus ln of the winner's multiplicity in the row with a repeated column; its bar
    2^-22 (|s| + ln multiplicity))"""
    lnm = torch.log(mult.clamp(min=1).double())
    return top + lnm, 2.0 ** -22 * (top.abs() + lnm)


def check_units(label, got, q):
    """the flat backward's bar: |err| <= 2^-23 q.units, plus 2^-8 |ref| for a bf16 output: (findings, largest fraction of the bar)"""
    return _worst(label, (got.double() - q.ref).abs(), 2.0 ** -23 * q.units + _bf16_part(got, q.ref))


def check_project(label, dtype, got, ref, forward):
    """the bars of test_sparse_attn_gpu.py / test_gatv2_gpu.py by the OPERANDS' dtype (grad_attn is stored in fp32 either way): fp32
    max|err| <= 1e-4 (forward) / 2e-3 max|ref|, bf16 2e-2 max|ref| (forward) / relative L2 1.5e-2."""
    a = got.double()
    err_max = ((a - ref).abs().max() / ref.abs().max()).item()
    err_l2 = ((a - ref).norm() / ref.norm()).item()
    if dtype == F32:
        bar, err = (1e-4 if forward else 2e-3), err_max
    else:
        bar, err = (2e-2, err_max) if forward else (1.5e-2, err_l2)
    return [] if err <= bar else ["%s: %.3e over the bar %.1e" % (label, err, bar)]


def err_over_scale(got, q):
    """largest |err| / scale over the entries with a scale"""
    err = (got.double() - q.ref).abs()
    live = q.scale > 0
    return (err[live] / q.scale[live]).max().item() if bool(live.any()) else 0.0


def check_zero_rows(label, got, rows):
    rows = list(rows)
    return [] if not rows or got[rows].abs().max().item() == 0.0 else ["%s: a row that sums nothing is not exactly 0" % label]


def swap_vectors(t, head, D, vec):
    """t with the first two 16-byte vectors of `head` exchanged in every row"""
    out = t.clone()
    b = head * D
    out[:, b:b + vec], out[:, b + vec:b + 2 * vec] = t[:, b + vec:b + 2 * vec], t[:, b:b + vec]
    return out
