"""The sweep of the FLAT passes on csrc/row_tiles.hpp -- those whose launch comes from make_flat_geometry(vpr, n_rows): edge_feat.hip,
edge_proj.hip, gated.hip, res_gated.hip, soft_agg.hip and gmm.hip (multi_agg.hip and typed_spmm.hip keep their own files, with
widths added) -- on rowtile_ref.sweep_graph(): the table of widths, the operands, the float64 references (the operators' own
restatements, unchanged) and a comparator PER ROW.  test_flat_ref_host.py pins all of it without a GPU, test_flat_geometry_gpu.py runs
it on the card.

GEOMETRY.  A row of F columns is vpr = F / epv 16-byte vectors (epv = 4 fp32, 8 bf16).  lpr, the lanes of a row, is the power of two
at or above min(vpr, 64), at least 8; col_blocks = ceil(vpr / lpr); a tile holds 256 / lpr rows.  TABLE lists eleven vpr: each of
lpr = 8, 16, 32, 64 with idle lanes and with every lane busy, then a second column block of one vector, two full blocks, and three
blocks of which the last holds one vector.  LPR_WIDTHS is the one width per lpr the secondary configurations run at.

OPERANDS.  Random leg: the operator's own helper (test_edge_feat_gpu._inputs, efp_ref.inputs, gmm_ref.inputs, test_soft_agg_gpu._inputs,
test_gated_gpu._inputs, test_res_gated_gpu._inputs) with the pinned seed 1000 vpr + (0 fp32, 1 bf16) + an offset per operator; GMM
adds GMM_SEED_STEP * n for the first n whose parameter gradients are conditioned as test_gmm_emulated.well_conditioned asks (the
pinned n are in GMM_SEEDS, asserted where used).  Exact leg: edge_feat -- integers in [-4, 4], the row scale absent or a power of
two; edge_proj -- efp_ref.inputs(dyadic=True); gmm -- the hard-assignment limit of test_gmm_gpu.py on the sweep graph.

edge_proj's random leg: "mul" and "add" as above, and add_relu (RELU = add_relu, mean, De = 3, bias) at every width for which a seed
is pinned.  efp_ref.near_gate must count no element before add_relu may be compared on random inputs (efp_ref.py); EFP_SEEDS holds, per
(vpr, dtype), the first n of seed + EFP_SEED_STEP * n, n < 40, for which it counts none, found the way test_edge_proj_emulated.SEEDS
were, and EdgeProj.reference asserts the count wherever such inputs are used (host and GPU).  The expected count is about
5,000 F x 2.4e-6: seeds exist for every fp32 width but vpr 129 (F = 516: 2 .. 10 elements in each of 40 seeds) and for bf16 vpr 1 .. 32;
none of 40 does for bf16 vpr 33 (1 .. 7 elements), 64 (2 .. 12), 65 (2 .. 10), 128 (3 .. 16) and 129 (3 .. 17), which are left out
of this one configuration.  So random add_relu runs every lane width and a second column block in fp32 and lpr 8, 16 and 32 in bf16; at
every width add_relu also runs the dyadic leg (reduce "sum"), where the result must be EQUAL, gates included.

COMPARATOR (check_rows).  For an output with rows r let S_r = max_c |ref[r, c]|.  An element passes when

    |got - ref| <= B S_r + (2^-8 |ref[r, c]| if the output is stored in bf16)

with B the project's fp32 bar of DESIGN section 8 -- 1e-4 forward, 2e-3 gradients -- for BOTH dtypes: the accumulators are fp32 either
way and the reference sees the rounded inputs, so what bf16 adds is one store rounding (half an ulp of 2^-8 relative: 2^-9 |ref|,
doubled).  S_r = 0 (empty rows, unreferenced sources) demands exactly 0.  Quantities that are one number or one small matrix summed
over all entries keep the bars and preconditions of their operator's own test (check_whole): edge_proj grad_W / grad_b, gmm grad_mu /
grad_inv_sigma (conditioning <= 50 asserted), soft_agg grad_theta (on the reference's sum |g d out / d theta|).

RESTATED ROUNDINGS.  Where a wrapper or a kernel rounds an intermediate to the storage dtype, the call to the reference restates it
and no bar is widened for it:
  gmm, mean        ops_gmm scales the gradient's rows once in the storage dtype, the scale rounded first: the reference's gradients run
                   on dz = g * scale.to(dtype) with reduce "sum".
  res_gated, mean  ops_res_gated multiplies the gradient by the fp32 1 / deg and stores the product in the storage dtype: the
                   reference's gradients run on (g.float() * inv_deg).to(dtype) with mean=False.
  gated, bf16      gated.hip rounds ehat to the storage dtype and every pass takes the sigmoid of the STORED value (ops_gated's module
                   text); the columns pass sums the stored t = grad_c.  Gated.restated: ehat stays held to the float64 sum; out and the
                   gradients are gated_ref's with c := the kernel's own stored ehat and a = b = 0 (the same ehat, the same formulas);
                   grad_b is the column sums of the kernel's stored grad_c, itself held to that reference.  fp32 needs none of it
                   and runs against the plain reference.
                   The fed-back arrays are the kernel's OUTPUTS, not the dtype-rounded inputs: each is held to float64 first (ehat
                   on the tight form, grad_c against the reference built on that ehat), so an error in them cannot hide, but an
                   error shared by the forward's and the backward's gather of ehat would cancel here; the fp32 runs, which use the
                   plain reference through the same kernels' index code, are what excludes it.
Without a gradient through ehat the rows of ONE entry are masked out of the gated grad_a, grad_c (their edges) and grad_b (the columns
fed by such rows alone): Gated.judged has the derivation -- there they are differences of order eps that fp32 holds to 6e-2 of S_r.
Every other row, edge and column is judged on the tight form.

FALLBACK (bf16 only; 2e-2 S_r per row in place of the tight form), each with the reason found in the wrapper:
  gated grad_v     ops_gated.rows_raw allocates w_i = g_i / S_i, which the rows pass leaves for the columns pass, in the storage
                   dtype: grad_v[j] = sum sig w_i sums terms rounded to 2^-9 each, and gated_ref.gradients has no argument through
                   which a rounded w could be handed in.  Measured on the tight form: up to 2.7 times the bar (|err| / S_r 7.6e-3),
                   every other gated quantity inside it.  The fallback misses, of the planted faults of test_flat_ref_host.py, the
                   dropped and the doubled last entry of the 513-entry row (FALLBACK_MISSES: one term sig g_i / S_i with S_i the sum
                   of 513 gates, under 2e-2 of that column's S_r); it rejects the other eight.
No fp32 quantity falls back.

PLANTED FAULTS.  fault(graph, row, pos, how) drops or doubles one entry and returns the edge map, so that per-edge operands follow the
entries.  The quantities that SUM over entries (row side: over a row; column side: over an A^T row) are judged; a per-edge quantity
(grad_e, grad_a of edge_proj, grad_c, ehat, grad_pseudo) is one entry's own value and a dropped entry has no row of it to compare.
"""
from collections import namedtuple

import numpy as np
import torch

import ef_ref
import efp_ref
import gated_ref
import gmm_ref
import res_gated_ref
import rowtile_ref as R
import softagg_ref
from rowtile_ref import BF16, F32

DTYPES = (F32, BF16)
# (vpr, lpr, column blocks)
TABLE = [(1, 8, 1), (8, 8, 1), (9, 16, 1), (16, 16, 1), (17, 32, 1), (32, 32, 1), (33, 64, 1), (64, 64, 1), (65, 64, 2), (128, 64, 2),
         (129, 64, 3)]
VPRS = tuple(v for v, _, _ in TABLE)
LPR_WIDTHS = (8, 16, 17, 65)            # lpr 8 full, 16 full, 32 with idle lanes, 64 with a second block of one vector
NAN_VPR = 17
FAULT_VPR = 9
FAULT_ROWS = (9, 65, 257, 513)          # entry counts; the rows are sweep_graph().special[n]
HUB = R.HUBS[1]                         # 257 in-edges
B_FWD, B_GRAD = 1e-4, 2e-3
FALLBACK_BAR = 2e-2
FALLBACK = {("gated", "grad_v")}
# (operator, quantity, planted fault, how): what the fallback form misses in test_flat_ref_host.py
FALLBACK_MISSES = [("gated", "grad_v", "row of 513", "drop"), ("gated", "grad_v", "row of 513", "twice")]
GMM_K, GMM_DIM = 3, 2
GMM_SEED_STEP = 7919
SOFT_EPS, GATED_EPS = 1e-7, 1e-6

Qty = namedtuple("Qty", "ref kind side")        # kind: "fwd" / "grad"; side: "row", "col", "edge" or "whole"


def dname(dtype):
    return "fp32" if dtype == F32 else "bf16"


def width(vpr, dtype):
    return vpr * R.epv(dtype)


def flat_geometry(vpr, n_rows):
    """make_flat_geometry of csrc/row_tiles.hpp, restated: (lpr, col_blocks, tiles)"""
    lpr = 8
    while lpr < min(vpr, 64):
        lpr *= 2
    return lpr, -(-vpr // lpr), -(-n_rows // (256 // lpr))


def seed_of(vpr, dtype, offset=0):
    return 1000 * vpr + (0 if dtype == F32 else 1) + offset


# ---- planted faults ------------------------------------------------------------------------------------------------------------------
def fault(graph, row, pos, how):
    """(graph with entry `pos` of `row` dropped ("drop") or listed twice in a row ("twice"), keep): keep[k] is the entry of `graph`
    that entry k of the new graph is."""
    assert how in ("drop", "twice")
    rows = [list(r) for r in graph.rows]
    pos = pos % len(rows[row])
    at = int(graph.rowptr[row]) + pos
    if how == "drop":
        rows[row].pop(pos)
        keep = list(range(at)) + list(range(at + 1, graph.nnz))
    else:
        rows[row].insert(pos, rows[row][pos])
        keep = list(range(at + 1)) + list(range(at, graph.nnz))
    return R.Graph(rows, graph.n_cols, graph.special, graph.dup_row, graph.dup_col, graph.unreferenced), torch.tensor(keep)


def planted_faults(graph):
    """[(label, side, row, pos)]: the last entry of the rows of 9, 65, 257 and 513 entries (what Graph.without_last_entry and
    with_last_entry_twice touch), and an in-edge of the hub column of 257 in-edges taken from a row in the middle of the graph"""
    out = [("row of %d" % n, "row", graph.special[n], -1) for n in FAULT_ROWS]
    holder = next(r for r in range(graph.n_rows // 2, graph.n_rows) if HUB in graph.rows[r])
    return out + [("hub column %d" % HUB, "col", holder, graph.rows[holder].index(HUB))]


# ---- the comparators: each returns (findings, largest |err| / S_r, largest fraction of the bar) -----------------------------------------
def check_rows(label, got, ref, kind, fallback=False):
    assert got.shape == ref.shape, (label, tuple(got.shape), tuple(ref.shape))
    assert not (fallback and got.dtype == F32), label
    S = ref.abs().amax(1, keepdim=True)
    if fallback:
        bar = FALLBACK_BAR * S.expand_as(ref)
    else:
        bar = (B_FWD if kind == "fwd" else B_GRAD) * S + (2.0 ** -8 * ref.abs() if got.dtype == BF16 else 0.0)
    err = (got.double() - ref).abs()
    found, of_bar = R._worst(label, err, bar)
    live = (S > 0).squeeze(1)
    frac = (err[live] / S[live]).max().item() if bool(live.any()) else 0.0
    return found, frac, of_bar


def check_whole(label, dtype, got, ref, scale=None):
    """a sum over all entries, at its operator's own bar by the OPERANDS' dtype: fp32 max |err| <= 2e-3 max |ref|, bf16 relative L2
    <= 1.5e-2 (scale given -- soft_agg's grad_theta: |err| <= 2e-3 / 1.5e-2 of scale).  Returns (findings, the error, its fraction of the
    bar)."""
    a, ref = got.double().reshape(-1), ref.double().reshape(-1)
    if scale is not None:
        err, bar = (a - ref).abs().max().item() / scale, (2e-3 if dtype == F32 else 1.5e-2)
    elif dtype == F32:
        err, bar = ((a - ref).abs().max() / ref.abs().max()).item(), 2e-3
    else:
        err, bar = ((a - ref).norm() / ref.norm()).item(), 1.5e-2
    return ([] if err <= bar else ["%s: %.3e over the bar %.1e" % (label, err, bar)]), err, err / bar


# ---- the operators ---------------------------------------------------------------------------------------------------------------------
# Each: CONFIGS (the first runs the whole table, the others LPR_WIDTHS), inputs(graph, vpr, dtype, config, leg) -> dict of CPU tensors
# as stored, EDGE (the keys of per-edge operands), reference(graph, ins, config) -> {quantity: Qty}.
def _edge_map(ins, edge_keys, keep):
    return {k: (v[keep] if k in edge_keys and v is not None else v) for k, v in ins.items()}


class EdgeFeat:
    name = "edge_feat"
    CONFIGS = [(op, red) for red in ("mean", "sum") for op in ("add_relu", "mul", "add")]
    EDGE = ("e",)
    UNIT = 4.0                                              # the exact leg's values are multiples of 1 / UNIT (scale down to 1/4)

    @staticmethod
    def inputs(graph, vpr, dtype, config, leg):
        from test_edge_feat_gpu import _inputs

        F = width(vpr, dtype)
        if leg == "random":
            x, e, g = _inputs(graph, F, dtype, seed_of(vpr, dtype, 10))
            return {"x": x, "e": e, "g": g, "scale": None}
        gen = torch.Generator().manual_seed(seed_of(vpr, dtype, 11))
        x, e, g = (R._ints(gen, (n, F), -4, 4).to(dtype) for n in (graph.n_cols, graph.nnz, graph.n_rows))
        # exact leg: reduce "sum" is the absent scale, "mean" stands for a power-of-two row scale 1, 1/2, 1/4 (0 for an empty row)
        scale = None if config[1] == "sum" else (2.0 ** -(torch.arange(graph.n_rows) % 3).float()) * torch.from_numpy(graph.deg > 0).float()
        return {"x": x, "e": e, "g": g, "scale": scale}

    @staticmethod
    def reference(graph, ins, config):
        op, red = config
        x, e, g = ins["x"].double(), ins["e"].double(), ins["g"].double()
        if ins["scale"] is not None:                        # an explicit row scale: the sum's reference, scaled (exactly: powers of two)
            s = ins["scale"].double().unsqueeze(1)
            out = ef_ref.forward(graph.rowptr, graph.col, x, e, op, "sum") * s
            gx, ge = ef_ref.gradients(graph.rowptr, graph.col, x, e, g * s, op, "sum")
        else:
            out = ef_ref.forward(graph.rowptr, graph.col, x, e, op, red)
            gx, ge = ef_ref.gradients(graph.rowptr, graph.col, x, e, g, op, red)
        return {"out": Qty(out, "fwd", "row"), "grad_x": Qty(gx, "grad", "col"), "grad_e": Qty(ge, "grad", "edge")}

    @staticmethod
    def magnitude(graph, ins, config):
        """max over every output of the sum of |term|, in units of 1 / UNIT: the exact leg's premise is that this is < 2^24"""
        big = {k: (v.abs() if v is not None and k != "scale" else v) for k, v in ins.items()}
        ref = EdgeFeat.reference(graph, big, ("add" if config[0] == "add_relu" else config[0], config[1]))
        return max(q.ref.abs().max().item() for q in ref.values()) * EdgeFeat.UNIT


class EdgeProj:
    name = "edge_proj"
    # (op, reduce, De, bias): the first is the random leg's full-table configuration; De 3, 8, 16 are the three DB buckets
    CONFIGS = [("mul", "mean", 3, True), ("add", "sum", 8, False), ("mul", "sum", 16, True), ("add", "mean", 16, True)]
    RELU = ("add_relu", "mean", 3, True)                    # the random leg's gated configuration: at every width EFP_SEEDS has
    # the dyadic leg (equality, reduce "sum"): the first runs the whole table, and every (op, De bucket) runs
    DYADIC = [("add_relu", "sum", 3, True)] + [(op, "sum", De, bias) for op in efp_ref.OPS for De, bias in ((3, False), (8, True), (16, True))
                                               if (op, De) != ("add_relu", 3)] + [("add_relu", "sum", 16, False)]
    EDGE = ("a",)
    UNIT = 512.0                                            # x, a, g, W, b are k / 8: a term of grad_a or grad_W is a multiple of 1 / 512

    @staticmethod
    def inputs(graph, vpr, dtype, config, leg):
        op, _, De, bias = config
        seed = seed_of(vpr, dtype, 20 + De)
        if op == "add_relu" and leg == "random":            # KeyError: no seed is pinned for this width (module text)
            seed += EFP_SEED_STEP * EFP_SEEDS[(vpr, dname(dtype))]
        x, a, g, W, b = efp_ref.inputs(graph, width(vpr, dtype), De, dtype, seed, leg == "exact", bias)
        return {"x": x, "a": a, "g": g, "W": W, "b": b}

    @staticmethod
    def reference(graph, ins, config):
        op, red = config[:2]
        x, a, g, W = (ins[k].double() for k in ("x", "a", "g", "W"))
        b = None if ins["b"] is None else ins["b"].double()
        if op == "add_relu" and not _is_dyadic(ins):        # a precondition on the seed, not a skip
            assert efp_ref.near_gate(graph.col, x, a, W, b) == 0, "the pinned seed leaves elements within the gate margin"
        out = efp_ref.forward(graph.rowptr, graph.col, x, a, W, b, op, red)
        gx, ga, gW, gb = efp_ref.gradients(graph.rowptr, graph.col, x, a, W, b, g, op, red)
        res = {"out": Qty(out, "fwd", "row"), "grad_x": Qty(gx, "grad", "col"), "grad_a": Qty(ga, "grad", "edge"),
               "grad_W": Qty(gW, "grad", "whole")}
        if b is not None:
            res["grad_b"] = Qty(gb, "grad", "whole")
        return res

    @staticmethod
    def magnitude(graph, ins, config):
        big = {k: (None if v is None else v.abs()) for k, v in ins.items()}
        ref = EdgeProj.reference(graph, big, ("add" if config[0] == "add_relu" else config[0],) + tuple(config[1:]))
        return max(q.ref.abs().max().item() for q in ref.values()) * EdgeProj.UNIT


# n per (vpr, dtype): efp_ref.near_gate counts no element for EdgeProj.RELU's inputs at seed + EFP_SEED_STEP * n (the first such n < 40)
EFP_SEED_STEP = 7919
EFP_SEEDS = {(1, "fp32"): 0, (8, "fp32"): 0, (9, "fp32"): 0, (16, "fp32"): 0, (17, "fp32"): 0, (32, "fp32"): 1, (33, "fp32"): 15,
             (64, "fp32"): 25, (65, "fp32"): 5, (128, "fp32"): 38,
             (1, "bf16"): 0, (8, "bf16"): 1, (9, "bf16"): 1, (16, "bf16"): 2, (17, "bf16"): 11, (32, "bf16"): 19}


def _is_dyadic(ins):
    return all(v is None or bool((v.double() * 8 == (v.double() * 8).round()).all()) for v in ins.values())


class Gmm:
    name = "gmm"
    CONFIGS = ["mean", "sum"]
    EDGE = ("pseudo",)
    UNIT = 8.0

    @staticmethod
    def inputs(graph, vpr, dtype, config, leg):
        F = width(vpr, dtype)
        if leg == "random":
            seed = seed_of(vpr, dtype, 30) + GMM_SEED_STEP * GMM_SEEDS.get((vpr, dname(dtype)), 0)
            x, pseudo, mu, sigma, g = gmm_ref.inputs(graph, F, GMM_K, GMM_DIM, dtype, seed)
            return {"x": x, "pseudo": pseudo, "mu": mu, "sigma": sigma, "g": g}
        # the hard-assignment limit of test_gmm_gpu.test_hard_assignment_limit_is_exact
        gen = torch.Generator().manual_seed(seed_of(vpr, dtype, 31))
        grid = torch.tensor([[k % 3, k // 3] for k in range(GMM_K)], dtype=torch.float32)
        owner = torch.randint(0, GMM_K, (graph.nnz,), generator=gen)
        x = (torch.randint(-8, 9, (graph.n_cols, F), generator=gen).float() / 8).to(dtype)
        g = (torch.randint(-8, 9, (graph.n_rows, GMM_K * F), generator=gen).float() / 8).to(dtype)
        return {"x": x, "pseudo": grid[owner], "mu": grid.clone(), "sigma": torch.full((GMM_K, GMM_DIM), 32.0), "g": g, "owner": owner}

    @staticmethod
    def reference(graph, ins, config, terms=False):
        x, pseudo, mu, sigma, g = (ins[k] for k in ("x", "pseudo", "mu", "sigma", "g"))
        z = gmm_ref.expand(graph.rowptr, graph.col, x, pseudo, mu, sigma, config)
        if config == "mean":                                # the wrapper's one rounding: g * scale.to(dtype), in the storage dtype
            g = g * gmm_ref.row_scale(graph.rowptr, "mean").to(g.dtype).unsqueeze(1)
        gx, gp, gm, gs, tm = gmm_ref.gradients(graph.rowptr, graph.col, x, pseudo, mu, sigma, g, "sum")
        res = {"Z": Qty(z, "fwd", "row"), "grad_x": Qty(gx, "grad", "col"), "grad_pseudo": Qty(gp, "grad", "edge"),
               "grad_mu": Qty(gm, "grad", "whole"), "grad_inv_sigma": Qty(gs, "grad", "whole")}
        return (res, tm) if terms else res

    @staticmethod
    def hard_expected(graph, ins):
        """(Z, grad_x) float64 of the hard-assignment limit, and the premise on the weights"""
        K, F, owner = GMM_K, ins["x"].shape[1], ins["owner"]
        w64 = gmm_ref.weights(ins["pseudo"], ins["mu"], ins["sigma"])
        hot = torch.nn.functional.one_hot(owner, K).bool()
        assert bool((w64[hot] == 1.0).all()) and w64[~hot].max().item() < 2.0 ** -200
        z = torch.zeros(graph.n_rows, K, F, dtype=torch.float64).index_put_((graph.row, owner), ins["x"].double()[graph.col.long()], accumulate=True)
        gx = torch.zeros(graph.n_cols, F, dtype=torch.float64).index_add_(0, graph.col.long(), ins["g"].double().view(-1, K, F)[graph.row, owner])
        return z.reshape(graph.n_rows, K * F), gx

    @staticmethod
    def magnitude(graph, ins, config=None):
        big = dict(ins, x=ins["x"].abs(), g=ins["g"].abs())
        return max(t.abs().max().item() for t in Gmm.hard_expected(graph, big)) * Gmm.UNIT


# n per (vpr, dtype) for which gmm_ref.conditioning of both parameter gradients is <= 50 with either reduction (0 where absent);
# found by counting n up from 0, asserted by test_flat_ref_host.py and again where the GPU test uses them
GMM_SEEDS = {(8, "fp32"): 3, (9, "fp32"): 1, (16, "fp32"): 1, (32, "fp32"): 3, (65, "fp32"): 2, (1, "bf16"): 1, (9, "bf16"): 2, (32, "bf16"): 1,
             (64, "bf16"): 1, (65, "bf16"): 2, (128, "bf16"): 1, (129, "bf16"): 1}


class SoftAgg:
    name = "soft_agg"
    # (mode, theta, with_e)
    CONFIGS = [("softmax", 1.0, True), ("power", 2.0, True), ("softmax", -0.5, False), ("power", 0.5, False)]
    EDGE = ("e",)

    @staticmethod
    def inputs(graph, vpr, dtype, config, leg):
        from test_soft_agg_gpu import _inputs

        x, e, g = _inputs(graph, width(vpr, dtype), dtype, seed_of(vpr, dtype, 40))
        return {"x": x, "e": e if config[2] else None, "g": g}

    @staticmethod
    def reference(graph, ins, config):
        mode, theta, _ = config
        r = softagg_ref.reference(graph.rowptr, graph.col, ins["x"], ins["e"], theta, ins["g"], mode, SOFT_EPS)
        res = {"out": Qty(r["out"], "fwd", "row"), "grad_x": Qty(r["grad_x"], "grad", "col"),
               "grad_theta": Qty((torch.tensor([r["grad_theta"]], dtype=torch.float64), r["scale"]), "grad", "whole")}
        if r["grad_e"] is not None:
            res["grad_e"] = Qty(r["grad_e"], "grad", "edge")
        return res


class Gated:
    name = "gated"
    CONFIGS = [True, False]                                 # with and without a gradient through ehat
    EDGE = ("c", "ge")
    @staticmethod
    def judged(graph, config, name):
        """The rows of quantity `name` that are compared (a bool mask), or None for all of them.  Without a gradient through ehat,
        t = g (v_j - out_i) / S_i sig (1 - sig) is ALL of grad_c, and in a row of one entry v_j - out_i = v_j eps / (sig + eps): a
        difference of order eps = 1e-6 of two numbers an fp32 kernel holds to 2^-24 each, so any fp32 evaluation is off by up to
        2^-24 / 1e-6 = 6e-2 of that row's S_r (measured: 2e-7 against references of 1e-6), and S_r is no scale of the row's terms.
        Masked there: grad_a's one-entry rows, grad_c's edges of such rows, grad_b's columns whose every in-edge comes from one."""
        if config or name not in ("grad_a", "grad_b", "grad_c"):
            return None
        single = torch.from_numpy(graph.deg == 1)
        if name == "grad_a":
            return ~single
        if name == "grad_c":
            return ~single[graph.row]
        fed = torch.zeros(graph.n_cols, dtype=torch.int64).index_add_(0, graph.col.long(), (~single[graph.row]).long())
        return (fed > 0) | torch.from_numpy(graph.indeg == 0)

    @staticmethod
    def inputs(graph, vpr, dtype, config, leg):
        from test_gated_gpu import _inputs

        a, b, c, v, g, ge = _inputs(graph, width(vpr, dtype), dtype, seed_of(vpr, dtype, 50))
        return {"a": a, "b": b, "c": c, "v": v, "g": g, "ge": ge if config else None}

    @staticmethod
    def reference(graph, ins, config):
        a, b, c, v, g = (ins[k].double() for k in "abcvg")
        ge = None if ins["ge"] is None else ins["ge"].double()
        out, ehat = gated_ref.forward(graph.rowptr, graph.col, a, b, c, v, GATED_EPS)
        ga, gb, gc, gv = gated_ref.gradients(graph.rowptr, graph.col, a, b, c, v, GATED_EPS, g, ge)
        return {"out": Qty(out, "fwd", "row"), "ehat": Qty(ehat, "fwd", "edge"), "grad_a": Qty(ga, "grad", "row"),
                "grad_b": Qty(gb, "grad", "col"), "grad_c": Qty(gc, "grad", "edge"), "grad_v": Qty(gv, "grad", "col")}

    @staticmethod
    def restated(graph, ins, config, got, ref):
        """bf16: the reference on the intermediates AS STORED.  gated.hip rounds ehat to the storage dtype and every pass takes the
        sigmoid of that stored value (ops_gated's module text), and the columns pass sums the stored t = grad_c.  ehat itself stays
        held to the float64 sum; out and the gradients are gated_ref's with c := the kernel's stored ehat and a = b = 0 (the same ehat,
        the same formulas); grad_b is the column sums of the kernel's stored grad_c, itself held to that reference."""
        ehat = got["ehat"].double()
        zero_a, zero_b = torch.zeros_like(ins["a"], dtype=torch.float64), torch.zeros_like(ins["b"], dtype=torch.float64)
        v, g = ins["v"].double(), ins["g"].double()
        ge = None if ins["ge"] is None else ins["ge"].double()
        out, _ = gated_ref.forward(graph.rowptr, graph.col, zero_a, zero_b, ehat, v, GATED_EPS)
        ga, _, gc, gv = gated_ref.gradients(graph.rowptr, graph.col, zero_a, zero_b, ehat, v, GATED_EPS, g, ge)
        gb = torch.zeros_like(zero_b).index_add_(0, graph.col.long(), got["grad_c"].double())
        return {"out": Qty(out, "fwd", "row"), "ehat": ref["ehat"], "grad_a": Qty(ga, "grad", "row"),
                "grad_b": Qty(gb, "grad", "col"), "grad_c": Qty(gc, "grad", "edge"), "grad_v": Qty(gv, "grad", "col")}


class ResGated:
    name = "res_gated"
    CONFIGS = ["mean", "sum"]
    EDGE = ()

    @staticmethod
    def inputs(graph, vpr, dtype, config, leg):
        from test_res_gated_gpu import _inputs

        k, q, v, g = _inputs(graph, width(vpr, dtype), dtype, seed_of(vpr, dtype, 60))
        return {"k": k, "q": q, "v": v, "g": g}

    @staticmethod
    def reference(graph, ins, config):
        k, q, v, g = (ins[n].double() for n in "kqvg")
        out = res_gated_ref.forward(graph.rowptr, graph.col, k, q, v, mean=config == "mean")
        if config == "mean":        # the wrapper's one rounding: g times the fp32 1 / deg, stored in the storage dtype; then the sum's passes
            inv = 1.0 / torch.from_numpy(np.maximum(graph.deg, 1)).float()
            g = (ins["g"].float() * inv.unsqueeze(1)).to(ins["g"].dtype).double()
        gk, gq, gv = res_gated_ref.gradients(graph.rowptr, graph.col, k, q, v, g, mean=False)
        return {"out": Qty(out, "fwd", "row"), "grad_k": Qty(gk, "grad", "row"), "grad_q": Qty(gq, "grad", "col"),
                "grad_v": Qty(gv, "grad", "col")}


OPERATORS = (EdgeFeat, EdgeProj, Gmm, SoftAgg, Gated, ResGated)

_REFS = {}


def case(op, vpr, dtype, config, leg="random", keep=False):
    """(inputs, reference) on the sweep graph.  keep: the pair stays cached (unchanged) for a later test -- only where one reads it
    again; a reference holds [nnz, F] float64 arrays."""
    key = (op.name, vpr, dtype, config, leg)
    if key in _REFS:
        return _REFS[key]
    g = R.sweep_graph()
    ins = op.inputs(g, vpr, dtype, config, leg)
    pair = (ins, op.reference(g, ins, config))
    if keep:
        _REFS[key] = pair
    return pair


def faulted_reference(op, graph, ins, config, row, pos, how):
    fg, keep = fault(graph, row, pos, how)
    return fg, keep, op.reference(fg, _edge_map(ins, op.EDGE, keep), config)


def judge(op, dtype, name, got, q, label="", rows=None):
    """(findings, largest |err| / S_r -- for a whole sum its error on its own scale --, largest fraction of the bar) for one quantity by
    its comparator; rows: a bool mask of the rows compared (None: all)"""
    if q.side == "whole":
        if isinstance(q.ref, tuple):
            return check_whole(label + name, dtype, got, q.ref[0], scale=q.ref[1])
        return check_whole(label + name, dtype, got, q.ref)
    ref = q.ref
    if rows is not None:
        got, ref = got[rows], ref[rows]
    return check_rows(label + name, got, ref, q.kind, fallback=got.dtype == BF16 and (op.name, name) in FALLBACK)


def stored(q, name, dtype):
    """the float64 reference rounded once to the dtype the operator stores the quantity in"""
    ref = q.ref[0] if isinstance(q.ref, tuple) else q.ref
    fp32_always = name in ("grad_W", "grad_b", "grad_mu", "grad_inv_sigma", "grad_pseudo", "grad_theta")
    return ref.to(F32 if fp32_always else dtype)
