"""spgemm on the GPU against a dense float64 product on the CPU: the exact structure, values within the bound of a sequential fp32 sum,
the same bits twice; the gradients of both operands; khop_graph, coarsen and `@`."""
import functools

import pytest
import torch

from dgll_amd import CSRGraph, ops_spgemm

pytestmark = pytest.mark.gpu
W, L = ops_spgemm.WAVE_MAX, ops_spgemm.LDS_MAX
U = 2.0 ** -23


def _rows(lists, n_cols, weighted, seed):
    """CPU CSRGraph whose row r holds the (increasing) columns lists[r]; random normal values or none"""
    row = torch.cat([torch.full((len(c),), r, dtype=torch.int64) for r, c in enumerate(lists)] + [torch.zeros(0, dtype=torch.int64)])
    col = torch.cat([torch.as_tensor(c, dtype=torch.int64) for c in lists] + [torch.zeros(0, dtype=torch.int64)])
    val = torch.randn(col.numel(), generator=torch.Generator().manual_seed(seed)) if weighted else None
    return CSRGraph.from_coo(row, col, val, (len(lists), n_cols))


# B of the class matrix: row k has B_DEG[k] entries; the rows of A below add them up to the product counts under test
N_ALL = L + 3
B_ALL = [[], [7], list(range(3, 8 * (W - 1), 8)), list(range(0, 8 * W, 8)), list(range(2, L + 1)), list(range(L)), [L + 2], [5, L + 1],
         list(range(50, 52 + L - 2 * W)), [7], [7], [7], [7]]
A_ALL = {"none": [[], [0]],                                    # an empty row; an entry that points at an empty row of B
         "wave": [[1], [2], [3], [1, 9, 10, 11, 12]],          # 1, W - 1, W (all distinct: a full table), 5 products on one column
         "block": [[1, 3], [4], [5]],                          # W + 1, L - 1, L (all distinct: a full table)
         "long": [[5, 6], [2, 3, 4, 5, 8]]}                    # L + 1, about 3 L
assert [sum(len(B_ALL[k]) for k in r) for r in sum(A_ALL.values(), [])] == [0, 0, 1, W - 1, W, 5, W + 1, L - 1, L, L + 1, 3 * L]


def _class_case(which, wa, wb):
    lists = sum(A_ALL.values(), []) if which == "all" else A_ALL[which]
    return _rows(lists, len(B_ALL), wa, 1), _rows(B_ALL, N_ALL, wb, 2)


CASES = {
    **{"all-%d%d" % (wa, wb): functools.partial(_class_case, "all", wa, wb) for wa in (0, 1) for wb in (0, 1)},
    **{which: functools.partial(_class_case, which, 1, 1) for which in ("wave", "block", "long")},
    # every key of a row in one bucket: columns congruent modulo the table (64 slots for 9 products, 2048 for 600)
    "one-bucket": lambda: (_rows([[0], [1], [0, 1]], 2, True, 3), _rows([[5 + W * t for t in range(9)], [5 + L * t for t in range(600)]], 600 * L, True, 4)),
    # keys above 2^16 in the wave class, a bitmap of 2^20 + 3 bits in the long class
    "wide": lambda: (_rows([[0, 1], [1], []], 2, True, 5), _rows([list(range(70000, 70000 + 200 * (L + 4), 200)), [65537, (1 << 20) + 2]], (1 << 20) + 3, True, 6)),
    "cancel": lambda: (CSRGraph.from_coo(torch.tensor([0, 0]), torch.tensor([0, 1]), torch.tensor([1.0, -1.0]), (1, 2)),
                       CSRGraph.from_coo(torch.tensor([0, 1]), torch.tensor([2, 2]), torch.tensor([3.0, 3.0]), (2, 4))),
    "empty-a": lambda: (_rows([[], [], []], 2, True, 7), _rows([[0, 3], [1]], 5, True, 8)),
    "empty-b": lambda: (_rows([[0, 1], [1]], 2, True, 9), _rows([[], []], 5, True, 10)),
    "no-rows": lambda: (_rows([], 2, True, 11), _rows([[0, 3], [1]], 5, True, 12)),
}


def _dense(g, cols=None):
    """(pattern, values) of g in float64 on the columns `cols` (sorted ids; None: all)"""
    at = g.col.long() if cols is None else torch.searchsorted(cols, g.col.long())
    pat = torch.zeros(g.n_rows, g.n_cols if cols is None else cols.numel(), dtype=torch.float64)
    val = pat.clone()
    pat[g.row_index(), at] = 1.0
    val[g.row_index(), at] = 1.0 if g.val is None else g.val.double()
    return pat, val


@functools.lru_cache(maxsize=None)
def _case(name):
    """the operands on the CPU and the float64 reference over the columns B uses: computed once, shared, never changed"""
    a, b = CASES[name]()
    cols = torch.unique(b.col.long())
    (pa, va), (pb, vb) = _dense(a), _dense(b, cols)
    terms = pa @ pb
    at = (terms > 0).nonzero()
    ref = dict(cols=cols, pa=pa, va=va, pb=pb, vb=vb, at=at, rowptr=torch.cat([torch.zeros(1, dtype=torch.int64), (terms > 0).sum(1).cumsum(0)]),
               col=cols[at[:, 1]].to(torch.int32), n=terms[at[:, 0], at[:, 1]], val=(va @ vb)[at[:, 0], at[:, 1]],
               scale=(va.abs() @ vb.abs())[at[:, 0], at[:, 1]])
    return a, b, ref


def _check_structure(c, a, b, ref):
    assert c.shape == (a.n_rows, b.n_cols) and c.rowptr.dtype == torch.int64 and c.col.dtype == torch.int32
    assert torch.equal(c.rowptr.cpu(), ref["rowptr"]) and torch.equal(c.col.cpu(), ref["col"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_matches_float64_and_repeats_bit_for_bit(name):
    a, b, ref = _case(name)
    ad, bd = a.to("cuda"), b.to("cuda")
    slots = 1 if name == "long" else None                      # one slot: the second long row waits for the first inside the launch
    c = ops_spgemm.spgemm(ad, bd, long_slots=slots)
    _check_structure(c, a, b, ref)
    assert c.val.dtype == torch.float32
    err = (c.val.cpu().double() - ref["val"]).abs()
    print(name, "nnz", c.nnz, "worst error / bound", float((err / ((ref["n"] + 1) * U * ref["scale"])).max()) if c.nnz else 0.0)
    assert bool((err <= (ref["n"] + 1) * U * ref["scale"]).all())
    if name == "cancel":
        assert c.val.tolist() == [0.0]                         # the entry stays
    again = ops_spgemm.spgemm(ad, bd, long_slots=slots)
    assert torch.equal(again.col, c.col) and torch.equal(again.val.view(torch.int32), c.val.view(torch.int32))
    pattern = ops_spgemm.spgemm(ad, bd, values=False, long_slots=slots)
    _check_structure(pattern, a, b, ref)
    assert pattern.val is None


@pytest.mark.parametrize("wa,wb", [(1, 0), (0, 1), (1, 1)])
def test_backward_matches_float64_autograd(wa, wb):
    a, b, ref = _case("all-%d%d" % (wa, wb))
    ad, bd = a.to("cuda"), b.to("cuda")
    for g, on in ((ad, wa), (bd, wb)):
        if on:
            g.val.requires_grad_(True)
    weight = torch.randn(ref["col"].numel(), generator=torch.Generator().manual_seed(13))
    (ops_spgemm.spgemm(ad, bd).val * weight.cuda()).sum().backward()
    va, vb = ref["va"].clone().requires_grad_(True), ref["vb"].clone().requires_grad_(True)
    wd = torch.zeros_like(ref["pa"] @ ref["pb"])
    wd[ref["at"][:, 0], ref["at"][:, 1]] = weight.double()
    ((va @ vb) * wd).sum().backward()
    pc = (wd != 0).double()
    # (operand, float64 gradient, terms of every entry, sum of their magnitudes), dense; read at the operand's pattern
    sides = [(ad, a, None, va.grad, pc @ ref["pb"].t(), wd.abs() @ ref["vb"].abs().t()),
             (bd, b, ref["cols"], vb.grad, ref["pa"].t() @ pc, ref["va"].abs().t() @ wd.abs())]
    for (dev, host, cols, g64, n, scale), on in zip(sides, (wa, wb)):
        if not on:
            assert dev.val is None
            continue
        r, cc = host.row_index(), host.col.long() if cols is None else torch.searchsorted(cols, host.col.long())
        err = (dev.val.grad.cpu().double() - g64[r, cc]).abs()
        bound = (n[r, cc] + 1) * U * scale[r, cc]
        print("grad", "b" if cols is not None else "a", "worst error / bound", float((err / bound.clamp(min=1e-300)).max()))
        assert bool((err <= bound).all())


def test_khop_coarsen_matmul_and_the_refusal_of_a_repeated_column():
    a, b, _ = _case("all-11")
    ad, bd = a.to("cuda"), b.to("cuda")
    c, viaop = ops_spgemm.spgemm(ad, bd), ad @ bd
    assert torch.equal(c.rowptr, viaop.rowptr) and torch.equal(c.col, viaop.col) and torch.equal(c.val, viaop.val)
    edges = torch.tensor([[0, 0, 1, 2, 3, 4, 4, 5, 6, 6], [1, 4, 2, 0, 3, 5, 6, 0, 2, 6]])
    wts = torch.randn(10, generator=torch.Generator().manual_seed(14))
    g = CSRGraph.from_coo(edges[0], edges[1], wts, (7, 7))
    gd = g.to("cuda")
    two, ref = ops_spgemm.khop_graph(gd, 2), ops_spgemm.spgemm(gd, gd, values=False)
    assert two.val is None and torch.equal(two.rowptr, ref.rowptr) and torch.equal(two.col, ref.col)
    cluster = torch.tensor([2, 0, 0, 1, 2, 1, 0])
    s = torch.zeros(7, 3, dtype=torch.float64)
    s[torch.arange(7), cluster] = 1.0
    pat, val = _dense(g)
    small = ops_spgemm.coarsen(gd, cluster.cuda())
    got = torch.zeros(3, 3, dtype=torch.float64)
    got[small.row_index().cpu(), small.col.cpu().long()] = small.val.cpu().double()
    assert small.shape == (3, 3) and torch.equal(_dense(small.to("cpu"))[0], ((s.t() @ pat @ s) > 0).double())
    assert torch.allclose(got, s.t() @ val @ s, rtol=0, atol=11 * U * float(wts.abs().sum()))     # at most 10 terms per entry
    twice = CSRGraph(torch.tensor([0, 1, 3], device="cuda"), torch.tensor([0, 2, 2], dtype=torch.int32, device="cuda"), None, 2, len(B_ALL))
    with pytest.raises(ValueError, match="operand a must be strictly increasing"):
        ops_spgemm.spgemm(twice, bd)
