"""Every row kernel spmm_launch can instantiate (csrc/spmm.hip: 208 -- wave-per-row at 4 .. 64 lanes and 2 / 4 / 8 gathers in flight,
its prefetch variant, row-per-slot, row-group, flattened, one element per lane; x three dtype pairs x weighted x the accumulate / gate
epilogue) against the float64 reference of spmm_ref.py, on operands whose sums are exact in fp32: the comparison has no tolerance.
The table of launches is spmm_ref.CASES; test_spmm_ref_host.py pins, without a GPU, that it reaches all 208 and what each case runs.
The graph is spmm_ref.sweep_graph(): 1103 x 4200, rows of 0 .. 4 097 edges on both sides of every round, index batch and chunk edge,
five rows above the plan's threshold (33 chunk items; the finalize kernel's second and third trip), unreferenced columns.

One test per (knob set, dtype pair, width) runs weighted x six forms (spmm_ref.FORMS), "default" also the unaligned launches.  For
every launch: the kernel is the one the table names (asked of dgll_hip_debug_spmm_choice under the live knobs); X sits in a buffer
whose padding, and whose rows of the unreferenced columns, are NaN -- the output must be finite, so idle slots and lanes are zeroed
by selection and never by multiplication; the output's padding (for P3: its neighbouring rows and columns too) keeps a sentinel; a
second launch gives the same bits; the result meets spmm_ref.check().

Bars (spmm_ref.check).  Exact forms (reduce = "sum", or any row_scale): fp32 output equal to the reference cast to
fp32, bf16 output equal to the reference cast to bf16.  reduce = "mean" without row_scale: |got - ref| <= 2^-21 (|S| / len + |bias|)
-- 1.0f / len within 2.5 ulp, the product and the bias add half an ulp each --, for a bf16 output plus 2^-8 |ref|.  No atol."""
import numpy as np
import pytest
import torch

import spmm_ref
from spmm_ref import F32, FORMS, KNOB_SETS, RUNS, check, expected_kernel, form_reference, operands, run_cases, run_id, storage
from test_spmm_choice_host import knobs
from test_spmm_ref_host import choice_of, shown

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -77.0            # exact in bf16; no launch of the sweep may write it or overwrite it
_graphs = {}


def device_graph(name, plan_knobs):
    """(CSRGraph without values, its fp32 weights on the device) of a sweep graph, one per (graph, knobs read at plan creation):
    the plan is created here, inside the knobs, on a CSRGraph nobody else holds."""
    key = (name, tuple(sorted(plan_knobs.items())))
    if key not in _graphs:
        from dgll_amd import CSRGraph

        g = spmm_ref.GRAPHS[name]()
        cg = CSRGraph(torch.from_numpy(g.rowptr).to(DEV), torch.from_numpy(g.col).to(DEV), None, g.n_rows, g.n_cols)
        if g.max_degree is not None:
            cg.max_degree = g.max_degree
        with knobs(**plan_knobs):
            cg.plan()
        assert cg.num_long_rows() == g.n_long and cg.workspace_bytes(8) == g.n_chunks * 8 * 4
        _graphs[key] = (cg, torch.from_numpy(g.val).to(DEV))
    return _graphs[key]


def _vec(t):
    return 16 // t.element_size()


def in_buffer(t, fill, top=0, bottom=0, left=0, not_pitch=None):
    """(view, buffer): the CPU tensor t on the device inside a buffer of `fill`, rows on a 16-byte pitch at least one vector wider than
    t (and not `not_pitch` elements), `top` / `bottom` rows and `left` columns of fill around it."""
    n, width = t.shape
    pitch = -(-(left + width) // _vec(t)) * _vec(t) + _vec(t)
    pitch += _vec(t) if pitch == not_pitch else 0
    buf = torch.full((top + n + bottom, pitch), fill, dtype=t.dtype, device=DEV)
    view = buf[top:top + n, left:left + width]
    view.copy_(t)
    return view, buf


def untouched_outside(view, buf):
    """Everything of buf outside view still holds the sentinel."""
    rest = buf.clone()
    rest[view.storage_offset() // buf.stride(0):view.storage_offset() // buf.stride(0) + view.shape[0],
         view.storage_offset() % buf.stride(0):view.storage_offset() % buf.stride(0) + view.shape[1]] = SENTINEL
    return bool((rest == SENTINEL).all())


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_every_form_is_exact(run):
    from dgll_amd import ops

    name, xd, yd, width = run
    ks = KNOB_SETS[name]
    g = spmm_ref.GRAPHS[ks.graph]()
    cg, val = device_graph(ks.graph, ks.plan_knobs)
    op = operands(ks.graph, width, xd)
    x = storage(op["x"], xd)
    x[0] = float("nan")                                      # rows of the columns no edge references: read by idle slots at the most
    x[spmm_ref.END_COL:] = float("nan")
    x_aligned, _ = in_buffer(x, float("nan"))
    x_off, _ = in_buffer(x, float("nan"), left=1)           # one element off 16-byte alignment: the one-element-per-lane kernel
    assert ops.rows16_ok(x_aligned) and not ops.rows16_ok(x_off) and x_aligned.stride(0) > width
    bias = storage(op["bias"], F32).to(DEV)
    row_scale = storage(op["row_scale"], F32).to(DEV)
    gate, _ = in_buffer(storage(op["gate"], yd), float("nan"))
    y_old = storage(op["y_old"], yd)
    y_old_nan = y_old.clone()
    y_old_nan[torch.from_numpy(g.deg == 0)] = float("nan")   # the increment form must not touch a row without edges
    live = g.deg > 0
    live_t = torch.from_numpy(live)
    bits = torch.int32 if yd == F32 else torch.int16
    bad = []

    def launch(case):
        f = FORMS[case.form]
        if case.form == "P3":                                # a column-and-row slice of a larger buffer: ldy != ldx
            out, buf = in_buffer(torch.full((g.n_rows, width), SENTINEL, dtype=y_old.dtype), SENTINEL, top=3, bottom=5, left=_vec(y_old),
                                 not_pitch=x_aligned.stride(0))
            assert out.stride(0) != x_aligned.stride(0)
        else:
            start = {0: torch.full_like(y_old, SENTINEL), 1: y_old, 2: y_old_nan}[f.get("accumulate", 0)]
            out, buf = in_buffer(start, SENTINEL)
        kw = dict(reduce=f["reduce"], relu=bool(f.get("relu")), accumulate=f.get("accumulate", 0))
        got = ops.spmm_raw(cg, x_aligned if case.aligned else x_off, val=val if case.weighted else None, out=out,
                           bias=bias if f.get("bias") else None, row_scale=row_scale if f.get("row_scale") else None,
                           gate=gate if f.get("gate") else None, **kw)
        assert got is out
        return out, buf

    with knobs(**ks.knobs):
        for case in run_cases(*run):
            label = "%s%s%s" % (case.form, " weighted" if case.weighted else "", "" if case.aligned else " unaligned")
            assert shown(choice_of(case)) == expected_kernel(case), (label, shown(choice_of(case)))
            out, buf = launch(case)
            again, _ = launch(case)
            ref, bound = form_reference(ks.graph, width, xd, case.weighted, case.form)
            got = out.cpu()
            if case.form == "E3":
                found = check(label, got, ref, bound, yd, g.deg, rows=live)
                if not torch.equal(got[~live_t].view(bits), y_old_nan[~live_t].view(bits)):
                    found.append("%s: a row without edges was written" % label)
            else:
                found = check(label, got, ref, bound, yd, g.deg)
            if not untouched_outside(out, buf):
                found.append("%s: wrote outside the output's rows and columns" % label)
            if not torch.equal(got.view(bits), again.cpu().view(bits)):
                found.append("%s: the second launch differs" % label)
            bad += found
    assert not bad, "%s:\n  %s" % (run_id(run), "\n  ".join(bad))


def test_sweep_graph_on_the_device():
    g = spmm_ref.sweep_graph()
    cg, _ = device_graph("sweep", {})
    assert (cg.n_rows, cg.n_cols, cg.nnz, cg.num_long_rows()) == (1103, 4200, g.nnz, 5)
    assert np.array_equal(cg.degrees().cpu().numpy(), g.deg)
    fine, _ = device_graph("sweep", KNOB_SETS["flat64"].plan_knobs)
    assert fine is not cg and fine.plan() != cg.plan()
    block, _ = device_graph("block", {})
    assert block.num_long_rows() == 0 and block.workspace_bytes(523) == 0
