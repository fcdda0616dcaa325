"""Every lane geometry make_head_geometry can give the passes on csrc/row_tiles.hpp that carry heads -- 22 (lanes of a head, lanes of
a row) pairs per dtype, rowtile_ref.CASES: 25 cases per dtype with idle lanes inside a head, idle lanes after the last head, ragged
and full column blocks -- for sparse attention (sparse_attn.hip), GATv2 (gatv2.hip) and the two node passes of mp_ops.hip, against
the float64 per-edge references of rowtile_ref.py on its 307 x 760 sweep graph (rows of 0 .. 700 entries on both sides of every
index batch and of LONG_ROW, a ragged last tile at every tile size, long rows and the threshold in the transpose too).

Per case and operator three legs (rowtile_ref's module text has the operands, the bars and their derivations):
  onehot   forward only; out must EQUAL the winner's value row, lse within 2^-22 |s|.  The gathered operands sit on a pitch one
           vector wider than heads * D with NaN in the padding and in the rows of the sources nobody references.
  flat     alpha = 1 / deg in closed form: forward within 2^-21 |S| / deg (+ 2^-8 for a bf16 store), every gradient within
           2^-23 sum K_t |term_t| (+ 2^-8 |ref| for a bf16 store); `zero` (q = 0, attn = 0) once per dtype.
  random   the bars of test_sparse_attn_gpu.py / test_gatv2_gpu.py, and the largest |err| / scale is recorded.
Every leg: empty rows and the rows of unreferenced sources exactly 0, everything finite, a second launch bit-identical.  k is v on
every second sparse-attention case.  The GATv2 rows pass also runs through ops_gatv2._launch with 1 and 3 grad_attn partials (every
tile grid-stride in one workgroup; three workgroups for 10 and for 77 tiles); the default, ceil(307 / 16) = 20 workgroups, already
gives workgroups without a tile at lpr = 8 (10 tiles) and four tiles a workgroup at lpr = 64 (77).  The grid-stride loop past
kMaxGridX needs 2^22 tiles and stays out of scope.  The last test prints what was measured."""
import numpy as np
import pytest
import torch

import rowtile_ref as R
from rowtile_ref import CASES, F32

pytestmark = pytest.mark.gpu

DEV = "cuda"
RECORD = {}                 # (operator, leg, quantity, dtype) -> (largest value, case)
INDEXED = list(enumerate(CASES))
ZERO_LEG = ("fp32-8x8", "bf16-8x16")


def _id(v):
    return R.case_id(v[1])


def _note(op, leg, name, case, value):
    key = (op, leg, name, "fp32" if case.dtype == F32 else "bf16")
    if value > RECORD.get(key, (-1.0, None))[0]:
        RECORD[key] = (value, R.case_id(case))


@pytest.fixture(scope="module")
def sweep():
    g = R.sweep_graph()
    cg = g.csr(DEV)
    cg.transpose()
    return g, cg


def _gathered(t, graph, rows=None):
    """t on the device on a wider pitch, NaN behind its columns and in the rows no entry references"""
    view, _ = R.padded(t.to(DEV), nan_rows=graph.unreferenced if rows is None else rows)
    return view


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32 if x.dtype == F32 else torch.int16), y.view(torch.int32 if y.dtype == F32 else torch.int16))
               for x, y in zip(a, b))


def _common(g, got, lse, row_side, col_side):
    """finite everywhere; empty rows and the rows of unreferenced sources exactly 0"""
    empty = np.flatnonzero(g.deg == 0)
    bad = R.check_finite("lse", lse) + R.check_zero_rows("lse", lse, empty)
    for name, t in got.items():
        bad += R.check_finite(name, t)
        if name in row_side:
            bad += R.check_zero_rows(name, t, empty)
        if name in col_side:
            bad += R.check_zero_rows(name, t, g.unreferenced)
    return bad


# ---- sparse attention ----------------------------------------------------------------------------------------------------------------
def _attn_run(cg, q, k, v, gr, heads, scale, backward):
    from dgll_amd import ops_attn

    out, lse = ops_attn.sparse_attention_forward_raw(cg, q, k, v, heads, scale)
    got = {"out": out}
    if backward:
        got["dq"], got["dk"], got["dv"] = ops_attn.sparse_attention_backward_raw(cg, q, k, v, heads, scale, lse, gr)
    return got, lse


def _attn_leg(g, cg, case, leg, shared):
    q, k, v, gr, scale = R.attn_operands(g, case, leg, shared)
    ref = R.attn_reference(g, q, k, v, gr, case.heads, scale)
    if leg == "onehot":
        kd = _gathered(k, g)
        dev = (q.to(DEV), kd, kd if shared else _gathered(v, g), gr.to(DEV))
    else:
        kd = k.to(DEV)
        dev = (q.to(DEV), kd, kd if shared else v.to(DEV), gr.to(DEV))
    got, lse = _attn_run(cg, *dev, case.heads, scale, leg != "onehot")
    again, lse2 = _attn_run(cg, *dev, case.heads, scale, leg != "onehot")
    bad = [] if _same_bits(list(got.values()) + [lse], list(again.values()) + [lse2]) else ["the second launch differs"]
    got, lse = {n: t.cpu() for n, t in got.items()}, lse.cpu()
    bad += _common(g, got, lse, ("out", "dq"), ("dk", "dv"))
    if leg == "onehot":
        win, mult, top = R.winners(g, ref["s"])
        want, keep = R.onehot_expected(g, v, win, mult, case.heads)
        bad += R.check_equal("out", got["out"], want, keep, case.heads)
        found, frac = R.check_lse("lse", lse, *R.onehot_lse(top, mult))
        _note("attn", leg, "lse", case, frac)
        bad += found
    elif leg in ("flat", "zero"):
        found, frac = R.check_flat_forward("out", got["out"], ref["mean"])
        _note("attn", leg, "out", case, frac)
        bad += found
        found, frac = R.check_lse("lse", lse, ref["lse"], R.flat_lse_bar(g, ref))
        _note("attn", leg, "lse", case, frac)
        bad += found
        for name in ("dq", "dk", "dv"):
            found, frac = R.check_units(name, got[name], ref[name])
            _note("attn", leg, name, case, frac)
            bad += found
        if leg == "zero" and got["dk"].abs().max().item() != 0.0:
            bad.append("dk is not exactly 0 for q = 0")
    else:
        for name in ("out", "dq", "dk", "dv"):
            bad += R.check_project(name, case.dtype, got[name], ref[name].ref, name == "out")
            _note("attn", leg, name, case, R.err_over_scale(got[name], ref[name]))
    return ["%s: %s" % (leg, b) for b in bad]


@pytest.mark.parametrize("indexed", INDEXED, ids=_id)
def test_sparse_attention(sweep, indexed):
    index, case = indexed
    g, cg = sweep
    legs = ("onehot", "flat", "random") + (("zero",) if R.case_id(case) in ZERO_LEG else ())
    bad = [b for leg in legs for b in _attn_leg(g, cg, case, leg, shared=index % 2 == 1)]
    assert not bad, "%s:\n  %s" % (R.case_id(case), "\n  ".join(bad))


# ---- GATv2 -------------------------------------------------------------------------------------------------------------------------
def _gatv2_run(cg, xl, xr, attn, gr, heads, slope, backward):
    from dgll_amd import ops_gatv2

    out, lse = ops_gatv2.gatv2_forward_raw(cg, xl, xr, attn, heads, slope)
    got = {"out": out}
    if backward:
        got["dxl"], got["dxr"], dattn = ops_gatv2.gatv2_backward_raw(cg, xl, xr, attn, heads, slope, lse, gr)
        got["dattn"] = dattn.view(1, -1)
    return got, lse


def _gatv2_checks(g, case, leg, ref, got, lse, names):
    bad = []
    if leg in ("flat", "zero"):
        for name in names:
            found, frac = R.check_units(name, got[name], ref[name])
            _note("gatv2", leg, name, case, frac)
            bad += found
        if leg == "zero" and got["dxr"].abs().max().item() != 0.0:
            bad.append("dxr is not exactly 0 for attn = 0")
    else:
        for name in names:
            bad += R.check_project(name, case.dtype, got[name], ref[name].ref, False)
            _note("gatv2", leg, name, case, R.err_over_scale(got[name], ref[name]))
    return bad


def _gatv2_leg(g, cg, case, leg):
    xl, xr, attn, gr, slope = R.gatv2_operands(g, case, leg)
    ref = R.gatv2_reference(g, xl, xr, attn, gr, case.heads, slope)
    dev = (_gathered(xl, g) if leg == "onehot" else xl.to(DEV), xr.to(DEV), attn.to(DEV), gr.to(DEV))
    got, lse = _gatv2_run(cg, *dev, case.heads, slope, leg != "onehot")
    again, lse2 = _gatv2_run(cg, *dev, case.heads, slope, leg != "onehot")
    bad = [] if _same_bits(list(got.values()) + [lse], list(again.values()) + [lse2]) else ["the second launch differs"]
    got, lse = {n: t.cpu() for n, t in got.items()}, lse.cpu()
    bad += _common(g, got, lse, ("out", "dxr"), ("dxl",))
    if leg == "onehot":
        win, mult, top = R.winners(g, ref["s"])
        want, keep = R.onehot_expected(g, xl, win, mult, case.heads)
        bad += R.check_equal("out", got["out"], want, keep, case.heads)
        found, frac = R.check_lse("lse", lse, *R.onehot_lse(top, mult))
        _note("gatv2", leg, "lse", case, frac)
        bad += found
    else:
        if leg in ("flat", "zero"):
            found, frac = R.check_flat_forward("out", got["out"], ref["mean"])
            _note("gatv2", leg, "out", case, frac)
            bad += found
            found, frac = R.check_lse("lse", lse, ref["lse"], R.flat_lse_bar(g, ref))
            _note("gatv2", leg, "lse", case, frac)
            bad += found
        else:
            bad += R.check_project("out", case.dtype, got["out"], ref["out"].ref, True)
            _note("gatv2", leg, "out", case, R.err_over_scale(got["out"], ref["out"]))
        bad += _gatv2_checks(g, case, leg, ref, got, lse, ("dxl", "dxr", "dattn"))
    return ["%s: %s" % (leg, b) for b in bad]


@pytest.mark.parametrize("indexed", INDEXED, ids=_id)
def test_gatv2(sweep, indexed):
    _, case = indexed
    g, cg = sweep
    legs = ("onehot", "flat", "random") + (("zero",) if R.case_id(case) in ZERO_LEG else ())
    bad = [b for leg in legs for b in _gatv2_leg(g, cg, case, leg)]
    assert not bad, "%s:\n  %s" % (R.case_id(case), "\n  ".join(bad))


BY_ID = {R.case_id(c): c for c in CASES}


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("case", [BY_ID["fp32-5x4"], BY_ID["bf16-8x64"]], ids=R.case_id)         # lpr = 8: 10 tiles; lpr = 64: 77 tiles
def test_gatv2_rows_pass_with_few_partials(sweep, case, blocks):
    """The rows pass as a direct descriptor launch with `blocks` grad_attn partials: every workgroup takes its tiles grid-stride."""
    from dgll_amd import _lib, ops_gatv2
    from dgll_amd.ops import alloc_features

    g, cg = sweep
    assert case.geo.lpr in (8, 64)
    H, D, F = case.heads, case.D, case.heads * case.D
    bad = []
    for leg in ("flat", "random"):
        xl, xr, attn, gr, slope = R.gatv2_operands(g, case, leg)
        ref = R.gatv2_reference(g, xl, xr, attn, gr, H, slope)
        xl, xr, attn, gr = (t.to(DEV) for t in (xl, xr, attn, gr))
        _, lse = ops_gatv2.gatv2_forward_raw(cg, xl, xr, attn, H, slope)
        runs = []
        for _ in range(2):
            dxr = alloc_features(g.n_rows, F, case.dtype, DEV, pad_to=R.epv(case.dtype))
            ld2 = torch.full((g.n_rows, 2 * H), float("nan"), device=DEV)
            part = torch.full((blocks, F), float("nan"), device=DEV)
            dattn = torch.full((H, D), float("nan"), device=DEV)
            ops_gatv2._launch(_lib.GATV2_ROWS, cg, H, D, slope, xl, xr, attn, dxr, grad_out=gr, lse=lse, lse_delta=ld2, part=part, dattn=dattn)
            runs.append((dxr, ld2, part, dattn))
        if not _same_bits(*runs):
            bad.append("%s: the second launch differs" % leg)
        dxr, ld2, part, dattn = (t.cpu() for t in runs[0])
        got = {"dxr": dxr, "dattn": dattn.view(1, -1), "delta": ld2[:, H:]}
        live = torch.from_numpy(g.deg > 0)
        for name, t in (("dxr", dxr), ("dattn", dattn), ("partials", part), ("lse, delta", ld2[live])):
            bad += ["%s: %s" % (leg, b) for b in R.check_finite(name, t)]
        if not torch.equal(ld2[live][:, :H], lse.cpu()[live]):
            bad.append("%s: lse_delta does not carry the forward's lse" % leg)
        if blocks == 1 and not torch.equal(part[0], dattn.view(-1)):
            bad.append("%s: grad_attn is not its single partial" % leg)
        bad += ["%s: %s" % (leg, b) for b in R.check_zero_rows("dxr", dxr, np.flatnonzero(g.deg == 0))]
        if leg == "flat":
            found, _ = R.check_lse("lse", ld2[:, :H] * live.unsqueeze(1), ref["lse"], R.flat_lse_bar(g, ref))
            bad += ["flat: %s" % b for b in found]
            bad += ["flat: %s" % b for b in _gatv2_checks(g, case, leg, ref, {n: (t * live.unsqueeze(1) if n == "delta" else t) for n, t in got.items()},
                                                           None, ("dxr", "dattn", "delta"))]
        else:
            bad += ["random: %s" % b for b in _gatv2_checks(g, case, leg, ref, got, None, ("dxr", "dattn"))]
            err = ((got["delta"][live].double() - ref["delta"].ref[live]).abs().max() / ref["delta"].ref.abs().max()).item()
            if not err <= (2e-3 if case.dtype == F32 else 2e-2):
                bad.append("random: delta %.3e of max|ref|" % err)
    assert not bad, "%s, %d partials:\n  %s" % (R.case_id(case), blocks, "\n  ".join(bad))


def test_gatv2_with_xr_is_xl_on_a_square_graph(sweep):
    """xr is xl (shared weights) on the sweep graph padded with empty rows to 760 x 760: one gradient, the sum of the two."""
    from dgll_amd import ops_gatv2

    g, _ = sweep
    sq = R.Graph([list(r) for r in g.rows] + [[] for _ in range(g.n_cols - g.n_rows)], g.n_cols, g.special, g.dup_row, g.dup_col, g.unreferenced)
    case = BY_ID["fp32-8x8"]
    xl, _, attn, _, slope = R.gatv2_operands(sq, case, "random")
    gr = torch.randn(sq.n_rows, xl.shape[1], generator=torch.Generator().manual_seed(5))
    ref = R.gatv2_reference(sq, xl, xl, attn, gr, case.heads, slope)
    x, a = xl.to(DEV).requires_grad_(), attn.to(DEV).requires_grad_()
    out = ops_gatv2.gatv2_aggregate(sq.csr(DEV), x, x, a, case.heads, slope)
    dx, da = torch.autograd.grad(out, (x, a), gr.to(DEV))
    want = ref["dxl"].ref + ref["dxr"].ref
    bad = R.check_project("out", F32, out.detach().cpu(), ref["out"].ref, True) + R.check_project("dx", F32, dx.cpu(), want, False) \
        + R.check_project("dattn", F32, da.cpu().view(1, -1), ref["dattn"].ref, False)
    assert not bad, bad


# ---- the node passes of mp_ops.hip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("indexed", INDEXED, ids=_id)
def test_mp_node_passes_are_exact(sweep, indexed):
    from dgll_amd import ops_mp

    _, case = indexed
    g, cg = sweep
    x, y, w = R.mp_operands(g, case)
    fwd, bwd, dots, cap = R.mp_reference(g, x, y, w, case.heads)
    assert cap < 2 ** 24
    xd, yd, wd = _gathered(x, g), _gathered(y, g, rows=np.flatnonzero(g.deg == 0)), w.to(DEV)

    def run():
        return (ops_mp.u_mul_e_sum_raw(cg, xd, wd, case.heads), ops_mp.u_mul_e_sum_raw(cg, yd, wd, case.heads, transposed=True),
                ops_mp.u_dot_v_raw(cg, xd, yd, case.heads))

    got, again = run(), run()
    bad = [] if _same_bits(got, again) else ["the second launch differs"]
    for name, t, want in zip(("u_mul_e_sum", "u_mul_e_sum over A^T", "u_dot_v"), got, (fwd, bwd, dots)):
        assert t.shape == want.shape, name
        bad += R.check_finite(name, t.cpu()) + R.check_equal(name, t.cpu(), want)
    assert not bad, "%s:\n  %s" % (R.case_id(case), "\n  ".join(bad))


def test_zz_what_was_measured():
    """Prints the records of this run (pytest -s): per operator, leg, quantity and dtype the largest fraction of a derived bar (onehot,
    flat, zero) or the largest |err| / scale (random), with its case."""
    for key in sorted(RECORD):
        print("%-6s %-7s %-6s %-5s %.3e  [%s]" % (key + RECORD[key]))
    for key, (value, case) in RECORD.items():
        if key[1] != "random":
            assert value <= 1.0, (key, value, case)
