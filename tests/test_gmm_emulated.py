"""csrc/gmm.hip without a GPU: the kernel source and csrc/row_tiles.hpp, both UNMODIFIED, compiled with g++ against the host stand-ins
of tests/kernel_emu/ and run in lock step (tests/kernel_emu.py; test_sparse_attn_emulated.py says what that checks and what it cannot)
against the float64 entry-by-entry restatement of gmm_ref.py.  All three passes (EXPAND, CONTRACT, PARAM) on the graphs of
test_pna_emulated.py: rows of 0, 1, 64, 65 entries, one column five times, LONG_ROW, LONG_ROW + 1 and 400 entries, an empty last row
and an unreferenced last source.  pseudo sits on a pitch wider than dim with NaN behind it; P for PARAM is computed here in float64 and
rounded to fp32; the slabs start as the emulator's 0xCD fill, so an element no workgroup writes shows in the sum.

Bars, each against max |ref| of its tensor: fp32 forward max |err| <= 1e-4, gradients <= 2e-3; bf16 forward <= 2e-2,
gradients relative L2 <= 1.5e-2, the reference computed on the bf16-rounded x and gradient.  grad_mu and grad_inv_sigma are sums over
all entries: for the pinned seed the float64 reference must have max(sum_e |term|) / max |sum_e term| <= 50 (asserted: a precondition
on the seed, not a skip)."""
import os
import subprocess

import pytest
import torch

import gmm_ref
from kernel_emu import build_emulator
from test_pna_emulated import _dump, _err, _graph, _read

# (F, K, dim, dtype): one vector and one kernel; bf16 storage; a vector count that is no power of two; two kernel blocks; four kernel
# blocks; dim at its limit; 65 vectors (two column blocks, on the small graph) in both dtypes
CASES = [(4, 1, 1, torch.float32), (8, 3, 2, torch.bfloat16), (24, 3, 3, torch.float32), (24, 9, 2, torch.float32),
         (8, 25, 2, torch.bfloat16), (8, 8, 8, torch.float32), (260, 3, 2, torch.float32), (520, 3, 2, torch.bfloat16)]
# seeds of gmm_ref.inputs per (F, K, dim): gmm_ref.conditioning of both parameter gradients is at most MAX_CONDITIONING for them, with
# either reduction (asserted where they are used)
SEEDS = {(4, 1, 1): 2, (8, 3, 2): 1, (24, 3, 3): 1, (24, 9, 2): 1, (8, 25, 2): 1, (8, 8, 8): 1, (260, 3, 2): 1, (520, 3, 2): 1}
MAX_CONDITIONING = 50.0


def graph_of(F):
    return _graph(full=F < 260)


def well_conditioned(terms, what):
    for name, t in zip(("grad_mu", "grad_inv_sigma"), terms):
        c = gmm_ref.conditioning(t)
        print("%s conditioning of %s: %.1f" % (what, name, c))
        assert c <= MAX_CONDITIONING, (what, name, c)


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return build_emulator(tmp_path_factory, "gmm.hip", "gmm_main.cpp")


def _run(emulator, tmp_path, F, K, dim, dtype, reduce, partials):
    from dgll_amd import ops_gmm

    d, half = str(tmp_path), dtype == torch.bfloat16
    graph = graph_of(F)
    n_dst, n_src, nnz = graph.n_rows, graph.n_cols, graph.nnz
    gt, perm = graph.transpose()
    assert not torch.equal(perm, torch.arange(nnz))             # the transposed order really differs from A's
    x, pseudo, mu, sigma, g = gmm_ref.inputs(graph, F, K, dim, dtype, SEEDS[(F, K, dim)])
    scale = gmm_ref.row_scale(graph.rowptr, reduce)
    dz = (g.double() * scale.unsqueeze(1)).to(dtype)            # the wrapper scales the gradient's rows once, in the storage dtype
    ld_pseudo = dim + 1
    pseudo_p = torch.full((nnz, ld_pseudo), float("nan"))       # behind dim: must reach no result
    pseudo_p[:, :dim] = pseudo
    want_z = gmm_ref.expand(graph.rowptr, graph.col, x, pseudo, mu, sigma, reduce)
    want_gx, want_gp, want_gm, want_gs, terms = gmm_ref.gradients(graph.rowptr, graph.col, x, pseudo, mu, sigma, dz)
    well_conditioned(terms, "%s %s" % ((F, K, dim), reduce))
    p = torch.zeros(nnz, (K + 3) // 4 * 4)
    p[:, :K] = gmm_ref.edge_dots(graph.rowptr, graph.col, x, dz, K).float()
    if partials is None:
        partials = max(1, min(-(-nnz // 256), ops_gmm.MAX_PARTIALS))
    for name, t in (("rowptr", graph.rowptr), ("col", graph.col), ("trowptr", gt.rowptr), ("tcol", gt.col), ("perm", perm),
                    ("scale", scale.float()), ("pseudo", pseudo_p), ("mu", mu), ("sigma", sigma), ("x", x), ("dz", dz), ("p", p)):
        _dump(t, os.path.join(d, name + ".bin"))
    res = subprocess.run([emulator, d, str(n_dst), str(n_src), str(F), str(K), str(dim), "1" if half else "0", str(ld_pseudo),
                          "1" if reduce == "mean" else "0", str(partials)], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and "emu ok" in res.stdout, res.stdout + res.stderr

    fwd, grad = ("fwd16", "grad16") if half else ("fwd32", "grad32")
    z = _read(os.path.join(d, "z.bin"), dtype, (n_dst, K * F))
    gx = _read(os.path.join(d, "dx.bin"), dtype, (n_src, F))
    gp = _read(os.path.join(d, "gp.bin"), torch.float32, (nnz, dim))
    total = _read(os.path.join(d, "slabs.bin"), torch.float32, (partials, 2, K, dim)).sum(0)
    _err("z", z, want_z, fwd)
    _err("gx", gx, want_gx, grad)
    _err("gp", gp, want_gp, grad)
    _err("gmu", total[0], want_gm, grad)
    _err("gsigma", total[1], want_gs, grad)
    # rows without entries give zeros; the source no row references gets no gradient
    assert z[0].abs().max().item() == 0.0 and z[-1].abs().max().item() == 0.0
    assert gx[-1].abs().max().item() == 0.0


@pytest.mark.parametrize("n,case", list(enumerate(CASES)), ids=lambda v: str(v).replace("torch.", "") if isinstance(v, tuple) else None)
def test_all_passes_in_lock_step(emulator, tmp_path, n, case):
    F, K, dim, dtype = case
    # the reduction and the slab count alternate over the cases: partials 1 (every entry in one workgroup), 2, and the wrapper's default
    _run(emulator, tmp_path, F, K, dim, dtype, ("sum", "mean")[n % 2], (1, 2, None)[n % 3])
