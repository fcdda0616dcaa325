"""Every lane geometry make_flat_geometry can give the flat passes on csrc/row_tiles.hpp -- flat_ref.TABLE: lpr = 8, 16, 32 and 64 with
idle lanes and with every lane busy, one, two and three column blocks, in fp32 and bf16 -- for the six operators whose own GPU files
run lpr 8 and 64 only: edge_feat.hip (ops_ef), edge_proj.hip (ops_efp), gmm.hip (ops_gmm), soft_agg.hip (ops_softagg), gated.hip
(ops_gated) and res_gated.hip (ops_res_gated), through the entry points those files use, on rowtile_ref's 307 x 760 sweep graph and its
transpose (rows of 0 .. 700 entries on both sides of every index batch and of LONG_ROW, a ragged last tile at every tile size, many
tiles at every lane width, long rows anywhere in a tile, hub columns for the transposed passes), against the operators' float64
restatements under the PER-ROW comparator of flat_ref.py (its module text has the operands, the bars and the fallbacks).

Per operator the first configuration runs the whole table, the others one width per lane width (flat_ref.LPR_WIDTHS); between them
every kernel template instantiation an operator's wrapper can reach with these operands runs: edge_feat 3 ops x 3 passes; edge_proj
3 ops x the De buckets 4, 8, 16 x 4 passes (COLS not for "add", which has none); gmm EXPAND / CONTRACT at K = 3 and PARAM; soft_agg
2 modes x with / without e x 3 passes; gated and res_gated all passes, with and without a gradient through ehat / sum and mean.
Legs: random (per-row comparator) everywhere; exact where the operator is linear in what it sums -- edge_feat on integers with the
row scale absent or a power of two, edge_proj on dyadic inputs, gmm in the hard-assignment limit -- where the results must EQUAL the
float64 result rounded once.  Every run: everything finite, empty rows and the rows of unreferenced sources exactly 0, a second launch
bit-identical.  edge_proj's add_relu runs the random leg at every width flat_ref.EFP_SEEDS pins a seed for (near_gate = 0 asserted).
bf16 gated runs against the reference on the intermediates as the kernel stores them, and without a gradient through ehat the
one-entry rows are masked out of its grad_a / grad_b / grad_c (flat_ref.py: RESTATED ROUNDINGS, Gated.judged).  Once per
(operator, dtype), at vpr = 17, the forward runs again with NaN in the rows of the gathered operands that no entry references and
must give the same bits.  The soft_agg rows pass also runs as a direct descriptor launch with 1 and 3 partials
(every workgroup takes its tiles grid-stride).  The grid-stride loop past kMaxGridX needs 2^22 tiles and stays out of scope.  The last
test prints what was measured."""
import numpy as np
import pytest
import torch

import flat_ref as FR
import rowtile_ref as R
from flat_ref import DTYPES, LPR_WIDTHS, NAN_VPR, VPRS, dname
from rowtile_ref import BF16, F32

pytestmark = pytest.mark.gpu

DEV = "cuda"
RECORD = {}                 # (operator, quantity, dtype) -> [largest |err| / S_r (a whole sum: its error), its case, largest fraction of the bar, its case]
WIDTHS = [(vpr, dt) for dt in DTYPES for vpr in VPRS]
_ids = lambda v: "%s-vpr%d" % (dname(v[1]), v[0]) if isinstance(v, tuple) else str(v)        # noqa: E731


@pytest.fixture(scope="module")
def sweep():
    g = R.sweep_graph()
    cg = g.csr(DEV)
    cg.transpose()
    return g, cg


def _dev(t, grad=False):
    return None if t is None else t.to(DEV).requires_grad_(grad)


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _same_bits(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _with_nan(t, rows):
    t = t.clone()
    t[list(rows)] = float("nan")
    return t


# ---- the entry points: ins (CPU, as stored) -> {quantity: device tensor}; forward_only: no backward ------------------------------------
def _run_ef(cg, ins, config, forward_only=False, nan_rows=()):
    from dgll_amd import _lib, ops_ef
    from test_edge_feat_gpu import _op_act

    op, red = config
    if ins["scale"] is not None:                            # a caller's row scale: the three raw passes, which take one
        code = {"add": _lib.EF_ADD, "add_relu": _lib.EF_ADD_RELU, "mul": _lib.EF_MUL}[op]
        x, e, g, scale = (ins[k].to(DEV) for k in ("x", "e", "g", "scale"))
        out = ops_ef.forward_raw(cg, x, e, code, scale)
        return {"out": out, "grad_x": ops_ef.cols_raw(cg, x, e, g, code, scale), "grad_e": ops_ef.edge_raw(cg, x, e, g, code, scale)}
    x, e = _dev(_with_nan(ins["x"], nan_rows), not forward_only), _dev(ins["e"], not forward_only)
    out = ops_ef.u_op_e_sum(cg, x, e, *_op_act(op), reduce=red)
    if forward_only:
        return {"out": out}
    gx, ge = torch.autograd.grad(out, (x, e), ins["g"].to(DEV))
    return {"out": out.detach(), "grad_x": gx, "grad_e": ge}


def _run_efp(cg, ins, config, forward_only=False, nan_rows=()):
    from dgll_amd import ops_efp
    from test_edge_feat_gpu import _op_act

    op, red = config[:2]
    names = [k for k in ("x", "a", "W", "b") if ins[k] is not None]
    leaves = {k: _dev(_with_nan(ins[k], nan_rows) if k == "x" else ins[k], not forward_only) for k in names}
    out = ops_efp.u_op_proj_e_sum(cg, leaves["x"], leaves["a"], leaves["W"], leaves.get("b"), *_op_act(op), reduce=red)
    if forward_only:
        return {"out": out}
    grads = torch.autograd.grad(out, [leaves[k] for k in names], ins["g"].to(DEV))
    return dict({"out": out.detach()}, **{"grad_" + k: t for k, t in zip(names, grads)})


def _run_gmm(cg, ins, config, forward_only=False, nan_rows=()):
    from dgll_amd import ops_gmm

    names = ("x", "pseudo", "mu", "sigma")
    leaves = [_dev(_with_nan(ins[k], nan_rows) if k == "x" else ins[k], not forward_only) for k in names]
    z = ops_gmm.gmm_expand(cg, *leaves, reduce=config)
    if forward_only:
        return {"Z": z}
    grads = torch.autograd.grad(z, leaves, ins["g"].to(DEV))
    return dict({"Z": z.detach()}, **dict(zip(("grad_x", "grad_pseudo", "grad_mu", "grad_inv_sigma"), grads)))


def _run_softagg(cg, ins, config, forward_only=False, nan_rows=()):
    from dgll_amd import ops_softagg

    mode, theta, with_e = config
    x, e = _dev(_with_nan(ins["x"], nan_rows), not forward_only), _dev(ins["e"], not forward_only)
    th = torch.tensor([theta], device=DEV, requires_grad=not forward_only)
    fn = ops_softagg.softmax_aggregate if mode == "softmax" else ops_softagg.powermean_aggregate
    out = fn(cg, x, e, th, eps=FR.SOFT_EPS)
    if forward_only:
        return {"out": out}
    grads = torch.autograd.grad(out, [x, th] + ([e] if with_e else []), ins["g"].to(DEV))
    res = {"out": out.detach(), "grad_x": grads[0], "grad_theta": grads[1]}
    if with_e:
        res["grad_e"] = grads[2]
    return res


def _run_gated(cg, ins, config, forward_only=False, nan_rows=()):
    from dgll_amd import ops_gated

    leaves = [_dev(_with_nan(ins[k], nan_rows) if k in "bv" else ins[k], not forward_only) for k in "abcv"]
    out, ehat = ops_gated.gated_sum(cg, *leaves, FR.GATED_EPS)
    if forward_only:
        return {"out": out, "ehat": ehat}
    outs, gos = [out], [ins["g"].to(DEV)]
    if ins["ge"] is not None:
        outs.append(ehat)
        gos.append(ins["ge"].to(DEV))
    grads = torch.autograd.grad(outs, leaves, gos)
    return dict({"out": out.detach(), "ehat": ehat.detach()}, **{"grad_" + k: t for k, t in zip("abcv", grads)})


def _run_res_gated(cg, ins, config, forward_only=False, nan_rows=()):
    from dgll_amd import ops_res_gated

    leaves = [_dev(_with_nan(ins[k], nan_rows) if k in "qv" else ins[k], not forward_only) for k in "kqv"]
    out = ops_res_gated.res_gated_sum(cg, *leaves, reduce=config)
    if forward_only:
        return {"out": out}
    grads = torch.autograd.grad(out, leaves, ins["g"].to(DEV))
    return dict({"out": out.detach()}, **{"grad_" + k: t for k, t in zip("kqv", grads)})


RUN = {"edge_feat": _run_ef, "edge_proj": _run_efp, "gmm": _run_gmm, "soft_agg": _run_softagg, "gated": _run_gated, "res_gated": _run_res_gated}


# ---- one run against its reference ---------------------------------------------------------------------------------------------------
def _common(g, op, ins, config, ref, label):
    """two launches: the same bits, finite, exact zeros where nothing is summed -> (findings, the first launch on the host)"""
    got, again = RUN[op.name](g[1], ins, config), RUN[op.name](g[1], ins, config)
    bad = [] if _same_bits(got, again) else [label + "the second launch differs"]
    got = {k: t.cpu() for k, t in got.items()}
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    empty = np.flatnonzero(g[0].deg == 0)
    for name, t in got.items():
        bad += R.check_finite(label + name, t)
        if ref[name].side == "row":
            bad += R.check_zero_rows(label + name, t, empty)
        if ref[name].side == "col":
            bad += R.check_zero_rows(label + name, t, g[0].unreferenced)
    return bad, got


def _random_leg(g, op, vpr, dtype, config, pair=None):
    ins, ref = FR.case(op, vpr, dtype, config) if pair is None else pair
    label = "%s random: " % (config,)
    bad, got = _common(g, op, ins, config, ref, label)
    if dtype == BF16 and hasattr(op, "restated"):           # the reference on the intermediates as the kernel stores them
        ref = op.restated(g[0], ins, config, got, ref)
    for name, q in ref.items():
        rows = op.judged(g[0], config, name) if hasattr(op, "judged") else None
        found, frac, of_bar = FR.judge(op, dtype, name, got[name], q, label, rows)
        bad += found
        rec = RECORD.setdefault((op.name, name, dname(dtype)), [-1.0, None, -1.0, None])
        where = "vpr %d %s" % (vpr, config)
        if frac > rec[0]:
            rec[:2] = [frac, where]
        if of_bar > rec[2]:
            rec[2:] = [of_bar, where]
    return bad


def _exact_leg(g, op, vpr, dtype, config, equal, zero=()):
    """equal: the quantities that must EQUAL the float64 reference rounded once to their dtype; zero: those that must be exactly 0"""
    ins, ref = FR.case(op, vpr, dtype, config, "exact")
    assert op.magnitude(g[0], ins, config) < 2 ** 24        # the leg's premise: every partial sum exact in fp32
    label = "%s exact: " % (config,)
    bad, got = _common(g, op, ins, config, ref, label)
    for name in equal:
        if name in ref:
            bad += R.check_equal(label + name, got[name], ref[name].ref)
    for name in zero:
        if got[name].abs().max().item() != 0.0:
            bad.append(label + name + " is not exactly 0")
    return bad


def _configs(op, vpr, configs=None):
    configs = op.CONFIGS if configs is None else configs
    return configs[:1] + (configs[1:] if vpr in LPR_WIDTHS else [])


def _report(op, vpr, dtype, bad):
    assert not bad, "%s %s vpr %d (F = %d):\n  %s" % (op.name, dname(dtype), vpr, FR.width(vpr, dtype), "\n  ".join(bad))


# ---- the operators ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WIDTHS, ids=_ids)
def test_edge_feat(sweep, case):
    vpr, dtype = case
    op, bad = FR.EdgeFeat, []
    for config in _configs(op, vpr):
        bad += _exact_leg(sweep, op, vpr, dtype, config, ("out", "grad_x", "grad_e"))
        bad += _random_leg(sweep, op, vpr, dtype, config)
    _report(op, vpr, dtype, bad)


@pytest.mark.parametrize("case", WIDTHS, ids=_ids)
def test_edge_proj(sweep, case):
    vpr, dtype = case
    op, bad = FR.EdgeProj, []
    for config in _configs(op, vpr, op.DYADIC):
        bad += _exact_leg(sweep, op, vpr, dtype, config, ("out", "grad_x", "grad_a", "grad_W", "grad_b"))
    relu = [op.RELU] if (vpr, dname(dtype)) in FR.EFP_SEEDS else []       # its reference asserts near_gate == 0 for the pinned seed
    for config in _configs(op, vpr) + relu:
        bad += _random_leg(sweep, op, vpr, dtype, config)
    _report(op, vpr, dtype, bad)


@pytest.mark.parametrize("case", WIDTHS, ids=_ids)
def test_gmm(sweep, case):
    from test_gmm_emulated import MAX_CONDITIONING

    vpr, dtype = case
    op, bad = FR.Gmm, []
    # the hard-assignment limit: Z and grad_x EQUAL the one-hot aggregation, the other gradients exactly 0
    ins = op.inputs(sweep[0], vpr, dtype, "sum", "exact")
    want_z, want_gx = op.hard_expected(sweep[0], ins)
    assert op.magnitude(sweep[0], ins) < 2 ** 24
    got, again = _run_gmm(sweep[1], ins, "sum"), _run_gmm(sweep[1], ins, "sum")
    if not _same_bits(got, again):
        bad.append("hard limit: the second launch differs")
    got = {k: t.cpu() for k, t in got.items()}
    bad += R.check_equal("hard limit: Z", got["Z"], want_z) + R.check_equal("hard limit: grad_x", got["grad_x"], want_gx)
    bad += ["hard limit: %s is not exactly 0" % n for n in ("grad_pseudo", "grad_mu", "grad_inv_sigma") if got[n].abs().max().item() != 0.0]
    for config in _configs(op, vpr):
        ins = op.inputs(sweep[0], vpr, dtype, config, "random")
        ref, terms = op.reference(sweep[0], ins, config, terms=True)
        assert all(FR.gmm_ref.conditioning(t) <= MAX_CONDITIONING for t in terms), (vpr, config)      # a precondition on the seed, not a skip
        bad += _random_leg(sweep, op, vpr, dtype, config, (ins, ref))
    _report(op, vpr, dtype, bad)


@pytest.mark.parametrize("case", WIDTHS, ids=_ids)
def test_soft_agg(sweep, case):
    vpr, dtype = case
    op = FR.SoftAgg
    _report(op, vpr, dtype, [b for config in _configs(op, vpr) for b in _random_leg(sweep, op, vpr, dtype, config)])


@pytest.mark.parametrize("case", WIDTHS, ids=_ids)
def test_gated(sweep, case):
    vpr, dtype = case
    op = FR.Gated
    _report(op, vpr, dtype, [b for config in _configs(op, vpr) for b in _random_leg(sweep, op, vpr, dtype, config)])


@pytest.mark.parametrize("case", WIDTHS, ids=_ids)
def test_res_gated(sweep, case):
    vpr, dtype = case
    op = FR.ResGated
    _report(op, vpr, dtype, [b for config in _configs(op, vpr) for b in _random_leg(sweep, op, vpr, dtype, config)])


# ---- NaN where nothing is gathered from ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("op", FR.OPERATORS, ids=lambda o: o.name)
def test_nan_in_unreferenced_source_rows_reaches_nothing(sweep, op, dtype):
    g, cg = sweep
    config = op.CONFIGS[0]
    ins = op.inputs(g, NAN_VPR, dtype, config, "random")
    clean = RUN[op.name](cg, ins, config, forward_only=True)
    dirty = RUN[op.name](cg, ins, config, forward_only=True, nan_rows=g.unreferenced)
    assert all(bool(torch.isfinite(t.float()).all()) for t in dirty.values())
    assert _same_bits(clean, dirty)


# ---- soft_agg: the rows pass with fewer partials than tiles -----------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("case", [(1, F32), (17, BF16), (129, F32)], ids=_ids)       # 10 tiles of 32 rows; 39 of 8; 77 of 4 in three column blocks
@pytest.mark.parametrize("config", [FR.SoftAgg.CONFIGS[0], FR.SoftAgg.CONFIGS[3]], ids=["softmax-e", "power-noe"])
def test_soft_agg_rows_pass_with_few_partials(sweep, config, case, blocks):
    """The rows pass as a direct descriptor launch with n_partials = `blocks` workgroups per column block: every workgroup takes
    several tiles grid-stride and carries the scalar gradient's sum over them."""
    from dgll_amd import _lib, ops_softagg

    g, cg = sweep
    vpr, dtype = case
    op = FR.SoftAgg
    mode, theta, with_e = config
    lpr, col_blocks, tiles = FR.flat_geometry(vpr, g.n_rows)
    assert tiles > 3 * blocks
    ins, ref = FR.case(op, vpr, dtype, config, keep=True)          # read again by the other partial count
    x, e, go = ins["x"].to(DEV), _dev(ins["e"]), ins["g"].to(DEV)
    th = torch.tensor([theta], device=DEV)
    code = ops_softagg.SOFTMAX if mode == "softmax" else ops_softagg.POWER
    _, stats = ops_softagg.forward_raw(cg, code, x, e, th, FR.SOFT_EPS)
    runs = []
    for _ in range(2):
        ge = torch.full((g.nnz, x.shape[1]), float("nan"), dtype=dtype, device=DEV) if with_e else None
        parts = torch.full((blocks * col_blocks,), float("nan"), device=DEV)
        gth = torch.full((1,), float("nan"), device=DEV)
        ops_softagg._launch(_lib.SOFT_AGG_ROWS, code, cg, x, th, FR.SOFT_EPS, False, nnz=g.nnz, n_partials=blocks,
                            x=x, e=e, stats=stats, grad_out=go, grad_e=ge, partials=parts, grad_theta=gth)
        runs.append({k: t for k, t in (("grad_e", ge), ("partials", parts), ("grad_theta", gth)) if t is not None})
    bad = [] if _same_bits(*runs) else ["the second launch differs"]
    got = {k: t.cpu() for k, t in runs[0].items()}
    for name, t in got.items():
        bad += R.check_finite(name, t)
    if abs(got["partials"].double().sum().item() - got["grad_theta"].item()) > 2.0 ** -20 * got["partials"].double().abs().sum().item():
        bad.append("grad_theta is not the sum of its partials")
    for name in ("grad_e", "grad_theta"):
        if name in got:
            bad += FR.judge(op, dtype, name, got[name], ref[name])[0]
    assert not bad, "%s %s vpr %d, %d partials:\n  %s" % (config, dname(dtype), vpr, blocks, "\n  ".join(bad))


def test_zz_what_was_measured():
    """Prints the records of this run (pytest -s): per operator, quantity and dtype the largest |err| / S_r of the random leg (for a sum
    over all entries: its error on its own scale) and the largest fraction of the bar, each with its case.  For a bf16 store
    |err| / S_r is 3.9e-3 = 2^-8 by construction (the store's half ulp), so the fraction of the bar is the figure that speaks of the
    accumulation there.  An fp32 fraction above one half asks for a look at the kernel before it is accepted.  One is (MI355X):
    soft_agg grad_e fp32 1.78e-3 of S_r against B = 2e-3, at vpr 1 (four columns) on an entry of the 257-entry row whose three other
    columns are gated off and whose own factor 1 + t (m - out) is 3.6e-4: the kernel forms it as fmaf(t, m - out, 1) from the
    forward's fp32 out (2.016, a 257-term sum), whose few ulps become 1.8e-3 of a number 2,800 times smaller than its terms.  The
    formula's conditioning on a row of four columns, not a lane fault."""
    for key in sorted(RECORD):
        print("%-10s %-15s %-5s  |err|/S_r %.3e [%s]  of the bar %.3f [%s]" % (key + tuple(RECORD[key])))
