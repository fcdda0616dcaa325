"""Every geometry of the second-generation GAT passes (gat2_kernel, csrc/gat_kernel.hpp) against the float64 reference of
gat_ref.py: the 19 (lanes per row, heads per wavefront) pairs gat_choose() can reach, for fp32 and for bf16, in the forward, the rows
pass with exact and with stored dd, and the transposed pass -- plus ragged head blocks, several column blocks, heads without an idle
lane, the workgroup finalize kernel and one row per wavefront (the table and what it reaches: gat_ref.CASES, pinned by
test_gat_ref_host.py).  The graph is gat_ref.sweep_graph(): 531 x 760, rows of 1 .. 700 entries around the plan's chunk length,
long rows in A and in its transpose, columns that no row references.  No dropout (test_gat_dropout_gpu.py), mode 0 only.

One test per case runs five forms of the layer against the reference of that case:
  A  ops.gat_aggregate with compact fp32 scores: out, grad_h, grad_s, grad_t
  B  ops.gat_layer, t_j formed from the gathered rows in the forward and the rows pass: out, grad_h, grad_A
  C  ops.gat_layer with gathered scores (both row-score switches off) and the score-gradient epilogue: out, grad_h, grad_A
  D  ops.gat_layer with the scores in the padding of the rows (one head: the in-row form in all three passes): out, grad_h, grad_A
  E  the compact-score entry points of the partitioned path with the stored-dd rows pass: out, grad_s, grad_h, grad_t
and for each: finite outputs, exact zeros in grad_h / grad_t of the unreferenced columns, a second backward that is bit-identical.

Bars (gat_ref.check).  fp32: forward elementwise rtol 1e-4 / atol 1e-5, gradients elementwise rtol 2e-3 / atol 2e-4.
bf16, on the reference of the bf16-rounded operands: form A's forward elementwise 2^-8 |ref| + 1e-4 max|ref| -- the kernel
accumulates in fp32 and stores once, round-to-nearest-even (pack_bf16x2): half a bf16 step, plus the fp32 forward bar for the order
of the sums and the ELU's exp - 1; every other forward max|err| <= 2e-2 max|ref|, every gradient relative L2 <= 1.5e-2."""
import pytest
import torch

import gat_ref
from gat_ref import ALPHA, BASE_CASES, CASES, N_COLS, N_ROWS, USED_COLS, case_id, check

pytestmark = pytest.mark.gpu

DEV = "cuda"
# apply_elu alternates with the case's index; the two base cases of 8 heads on 32 lanes run both settings
RUNS = [(case, i % 2 == 0) for i, case in enumerate(CASES)]
RUNS += [(case, not elu) for case, elu in RUNS if case in BASE_CASES and case[1] == 8 and case[3] == 32]
assert len(RUNS) == len(CASES) + 2 == 51


@pytest.fixture(scope="module")
def graph():
    from dgll_amd import CSRGraph

    rowptr, col = gat_ref.sweep_graph()
    g = CSRGraph(rowptr.to(DEV), col.to(DEV), None, N_ROWS, N_COLS)
    assert g.num_long_rows() == 3 and g.transpose()[0].num_long_rows() == 2
    return g


def test_sweep_graph_has_long_rows_on_both_sides(graph):
    gt, _ = graph.transpose()
    assert (graph.n_rows, graph.n_cols, gt.n_rows, gt.n_cols) == (531, 760, 760, 531)
    assert graph.num_long_rows() == 3 and gt.num_long_rows() == 2
    assert int(graph.degrees().max()) == 700 and int(gt.degrees().max()) == 531 and int(gt.degrees()[USED_COLS:].sum()) == 0


def _tags(timer, word):
    return sum(word in key for key in timer.summary() if key[0] == "gat")


def _same_bits(first, second):
    return all(torch.equal(a, b) for a, b in zip(first, second))


def _unreferenced_rows_are_zero(name, grad):
    tail = grad[USED_COLS:]
    assert tail.shape[0] == 10
    return [] if float(tail.float().abs().max()) == 0.0 else ["%s: rows of unreferenced columns are not exactly 0" % name]


@pytest.mark.parametrize("case,apply_elu", RUNS, ids=lambda v: case_id(v) if isinstance(v, tuple) else ("elu" if v else "plain"))
def test_all_forms_against_float64(graph, case, apply_elu, monkeypatch):
    from dgll_amd import ops, ops_edge

    _, heads, fo = case[:3]
    dtype = gat_ref.torch_dtype(case)
    width, esz = heads * fo, (2 if dtype == torch.bfloat16 else 4)
    x = gat_ref.case_inputs(case)
    ref_st = gat_ref.case_reference(case, apply_elu, False)
    ref_A = gat_ref.case_reference(case, apply_elu, True)
    h0, gout = x["h"].to(DEV).to(dtype), x["gout"].to(DEV).to(dtype)            # exact: the values are representable
    s0, t0, A0 = x["s"].to(DEV), x["t"].to(DEV), x["A"].to(DEV)
    mask = x["A"] != 0                                                          # only the block-diagonal entries are parameters
    assert int(mask.sum()) == 2 * width
    label = "%s %s" % (case_id(case), "elu" if apply_elu else "plain")
    bad = []

    # ---- A: compact scores, one autograd node (forward, exact-dd rows pass with {s, dd} side by side, transposed pass)
    h, s, t = h0.clone().requires_grad_(), s0.clone().requires_grad_(), t0.clone().requires_grad_()
    out = ops.gat_aggregate(graph, h, s, t, heads, ALPHA, apply_elu=apply_elu, mode=0)
    assert out.dtype == dtype and out.shape == (N_ROWS, width)
    grads = torch.autograd.grad(out, (h, s, t), gout, retain_graph=True)
    again = torch.autograd.grad(out, (h, s, t), gout)
    bad += check(label + " A out", out, ref_st["out"], dtype, form_a=True)
    for name, got in zip(("grad_h", "grad_s", "grad_t"), grads):
        bad += check("%s A %s" % (label, name), got, ref_st[name], dtype)
    bad += _unreferenced_rows_are_zero("A grad_h", grads[0]) + _unreferenced_rows_are_zero("A grad_t", grads[2])
    if not _same_bits(grads, again):
        bad.append("A: the second backward differs")

    # ---- B, C, D: the layer as one node, scores from A
    def layer(form, h_leaf, pack):
        A = A0.clone().requires_grad_()
        with ops.LaunchTimer() as timer:
            out = ops.gat_layer(graph, h_leaf, A, heads, ALPHA, apply_elu=apply_elu, pack_scores=pack)
            grads = torch.autograd.grad(out, (h_leaf, A), gout, retain_graph=True)
        again = torch.autograd.grad(out, (h_leaf, A), gout)
        assert out.dtype == dtype and out.shape == (N_ROWS, width)
        found = check("%s %s out" % (label, form), out, ref_A["out"], dtype)
        found += check("%s %s grad_h" % (label, form), grads[0], ref_A["grad_h"], dtype)
        found += check("%s %s grad_A" % (label, form), grads[1].detach().cpu()[mask], ref_A["grad_A"][mask], dtype)
        found += _unreferenced_rows_are_zero(form + " grad_h", grads[0])
        if not _same_bits(grads, again):
            found.append(form + ": the second backward differs")
        return found, timer

    monkeypatch.setattr(ops_edge, "ROW_SCORES", True)
    monkeypatch.setattr(ops_edge, "ROW_SCORES_BWD", True)
    found, timer = layer("B", h0.clone().requires_grad_(), False)
    bad += found
    assert _tags(timer, "rowscore") == 2 and _tags(timer, "packed") == 0, list(timer.summary())

    monkeypatch.setattr(ops_edge, "ROW_SCORES", False)
    monkeypatch.setattr(ops_edge, "ROW_SCORES_BWD", False)
    found, timer = layer("C", h0.clone().requires_grad_(), False)
    bad += found
    assert _tags(timer, "rowscore") == 0 and _tags(timer, "packed") == 0, list(timer.summary())
    monkeypatch.undo()

    pad = -(-(8 * heads) // 16) * 16 // esz                 # at least 8 bytes per head behind every row, rows on a 16-byte pitch
    store = torch.zeros(N_COLS, width + pad, dtype=dtype, device=DEV)
    hp = store[:, :width]
    hp.copy_(h0)
    found, timer = layer("D", hp.requires_grad_(), True)
    bad += found
    assert _tags(timer, "packed") == 3 and _tags(timer, "rowscore") == 0, list(timer.summary())

    # ---- E: the entry points of the partitioned path, compact scores, dd_i from the stored output row
    def rows(n):                        # the layouts _GatAggregateStrided allocates, poisoned: what a pass leaves unwritten shows
        return ops_edge._empty_like_rows(n, h0).fill_(float("nan"))

    def scores(n):
        return torch.full((n, heads), float("nan"), dtype=torch.float32, device=DEV)

    gt, _ = graph.transpose()
    out_e, rowsum = rows(N_ROWS), scores(N_ROWS)
    ops_edge.gat_fwd_part(graph, h0, s0, t0, out_e, rowsum, heads, fo, ALPHA, apply_elu, raw=False, accumulate=False)

    def backward():
        dn, dd, grad_s = rows(N_ROWS), scores(N_ROWS), scores(N_ROWS)
        ops_edge.gat_bwd_rows_part(graph, h0, s0, t0, out_e, gout, rowsum, dn, dd, grad_s, heads, fo, ALPHA, apply_elu, accumulate=False)
        grad_h, grad_t = rows(N_COLS), scores(N_COLS)
        ops_edge.gat_bwd_cols_part(gt, dn, h0, t0, s0, dd, grad_h, grad_t, heads, fo, ALPHA)
        return grad_h, grad_s, grad_t

    grads, again = backward(), backward()
    bad += check(label + " E out", out_e, ref_st["out"], dtype)
    for name, got in zip(("grad_h", "grad_s", "grad_t"), grads):
        bad += check("%s E %s" % (label, name), got, ref_st[name], dtype)
    bad += _unreferenced_rows_are_zero("E grad_h", grads[0]) + _unreferenced_rows_are_zero("E grad_t", grads[2])
    if not _same_bits(grads, again):
        bad.append("E: the second backward differs")

    assert not bad, "%s:\n  %s" % (label, "\n  ".join(bad))
