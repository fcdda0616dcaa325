"""csrc/edge_proj.hip without a GPU: the kernel source and csrc/row_tiles.hpp, both UNMODIFIED, compiled with g++ against the host
stand-ins of tests/kernel_emu/ and run in lock step (tests/kernel_emu.py; test_sparse_attn_emulated.py says what that checks and what
it cannot) against the float64 entry-by-entry restatement of efp_ref.py.  All four passes (FORWARD, COLS, PARAM, DOTS), all three ops,
with and without the per-row scale of the mean reduce, on the graphs of test_pna_emulated.py; x, out and grad_x on a pitch wider than
F and a, grad_a on one wider than De, the padding proved unwritten by the 0xCD fill; `partials` 1, 2 and the tile count.  (COLS of
op "add" is edge_feat.hip's pass and is covered by test_edge_feat_emulated.py.)

Two kinds of input (efp_ref.py says why):
  dyadic   every value k / 8: all arithmetic is exact in fp32, so with reduce "sum" fp32 results EQUAL the float64 reference, gates and
           exact-zero sums included, and bf16 results equal it rounded once to bf16; grad_W and grad_b (fp32 slabs) equal it in both.
  random   after asserting that no element of x + aW + b is within 2^-19 (relative to its terms) of 0 for the seed used, the bars of
           DESIGN section 8: fp32 forward max |err| <= 1e-4 max |ref|, gradients <= 2e-3 max |ref|; bf16 forward <= 2e-2 max |ref|,
           gradients relative L2 <= 1.5e-2, the reference computed on the bf16-rounded inputs.  grad_W and grad_b leave the kernel
           as fp32 sums and meet the same bars."""
import os
import subprocess

import numpy as np
import pytest
import torch

import efp_ref
from kernel_emu import build_emulator
from test_edge_feat_emulated import FILL, _err
from test_pna_emulated import _dump, _graph, _read

# seeds of the random inputs, per (F, De): efp_ref.near_gate counts no element for them (asserted below)
SEEDS = {(4, 1): 1, (24, 3): 1, (24, 16): 1, (260, 8): 2, (8, 3): 1, (48, 8): 1, (48, 16): 1, (520, 16): 1, (520, 1): 1}


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return build_emulator(tmp_path_factory, "edge_proj.hip", "edge_proj_main.cpp")


def _tiles(n_rows, F, dtype):
    from dgll_amd import ops_efp

    return ops_efp.geometry(n_rows, F, dtype)


def _run(emulator, tmp_path, graph, F, De, dtype, dyadic, nulls, bias, partials):
    d, half = str(tmp_path), dtype == torch.bfloat16
    vec = 8 if half else 4
    n_dst, n_src, nnz = graph.n_rows, graph.n_cols, graph.nnz
    ld_x, ld_a = F + vec, (De + vec - 1) // vec * vec + vec
    gt, perm = graph.transpose()
    x, a, go, W, b = efp_ref.inputs(graph, F, De, dtype, 0 if dyadic else SEEDS[(F, De)], dyadic, bias)
    junk = torch.full((1,), float("nan")).to(dtype)           # behind the widths: must reach no result
    x_p, a_p = junk.repeat(n_src, ld_x), junk.repeat(nnz, ld_a)
    x_p[:, :F], a_p[:, :De] = x, a
    deg = graph.degrees().to(torch.float32)
    scale = torch.where(deg > 0, 1.0 / deg.clamp(min=1.0), torch.zeros_like(deg))
    for name, t in (("rowptr", graph.rowptr), ("col", graph.col), ("trowptr", gt.rowptr), ("tcol", gt.col), ("perm", perm),
                    ("scale", scale), ("x", x_p), ("a", a_p), ("go", go), ("w", W.t().contiguous())) + ((("b", b),) if bias else ()):
        _dump(t, os.path.join(d, name + ".bin"))
    tiles, col_blocks = _tiles(n_dst, F, dtype)
    partials = tiles if partials == "tiles" else partials
    res = subprocess.run([emulator, d, str(n_dst), str(n_src), str(F), "1" if half else "0", str(De), str(ld_x), str(ld_a), str(nulls),
                          "1" if bias else "0", str(partials)], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and "emu ok" in res.stdout, res.stdout + res.stderr

    assert not torch.equal(perm, torch.arange(nnz))             # the transposed order really differs from A's
    x64, a64, g64, W64, b64 = x.double(), a.double(), go.double(), W.double(), None if b is None else b.double()
    if not dyadic:                                              # a precondition on the seed, not a skip
        assert efp_ref.near_gate(graph.col, x64, a64, W64, b64) == 0
    fwd, grad = ("fwd16", "grad16") if half else ("fwd32", "grad32")
    np_dtype, fill = FILL[dtype]

    def unwritten(name, rows, ld, width):
        raw = np.fromfile(os.path.join(d, name), dtype=np_dtype).reshape(rows, ld)
        assert (raw[:, width:] == fill).all(), name

    for o, op in enumerate(efp_ref.OPS):
        for m, reduce in enumerate(("sum", "mean")):
            tag = "_%d_%d.bin" % (o, m)
            name = "%s/%s" % (op, reduce)
            exact = dyadic and reduce == "sum"
            want_out = efp_ref.forward(graph.rowptr, graph.col, x64, a64, W64, b64, op, reduce)
            want = dict(zip(("gx", "ga", "gw", "gb"), efp_ref.gradients(graph.rowptr, graph.col, x64, a64, W64, b64, g64, op, reduce)))
            got = {"out": _read(os.path.join(d, "out" + tag), dtype, (n_dst, ld_x))[:, :F]}
            unwritten("out" + tag, n_dst, ld_x, F)
            if o:
                got["gx"] = _read(os.path.join(d, "gx" + tag), dtype, (n_src, ld_x))[:, :F]
                unwritten("gx" + tag, n_src, ld_x, F)
            if col_blocks == 1:
                got["ga"] = _read(os.path.join(d, "ga" + tag), dtype, (nnz, ld_a))[:, :De]
                unwritten("ga" + tag, nnz, ld_a, De)
            else:                                               # the blocks' partial dots, summed in block order as the wrapper does
                part = _read(os.path.join(d, "gap" + tag), torch.float32, (col_blocks, nnz, De))
                acc = part[0]
                for blk in range(1, col_blocks):
                    acc = acc + part[blk]
                got["ga"] = acc.to(dtype)
            slabs = _read(os.path.join(d, "slabs" + tag), torch.float32, (partials, De + 1, F))
            total = slabs.sum(0)                                # every element of every slab is written: no fill survives
            got["gw"], got["gb"] = total[:De].t(), total[De]
            want["out"] = want_out
            for key in ("out", "gx", "ga", "gw", "gb"):
                if key not in got:
                    continue
                if exact:
                    ref = want[key] if key in ("gw", "gb") or not half else want[key].to(dtype)
                    assert torch.equal(got[key].double(), ref.double()), (name, key, (got[key].double() - ref.double()).abs().max())
                else:
                    _err("%s %s" % (key, name), got[key], want[key], fwd if key == "out" else grad)
            # rows without entries give zeros; the source no row references gets no gradient
            assert got["out"][0].abs().max().item() == 0.0 and got["out"][-1].abs().max().item() == 0.0
            if o:
                assert got["gx"][-1].abs().max().item() == 0.0


# F: one vector (seven idle lanes of the group), six vectors (not a power of two), 65 vectors (two column blocks, on the small graph:
# three tiles there, so partials = 1 carries a workgroup's sums across tiles and 2 gives workgroups of two tiles and one); De over all
# three buckets and both halves of the bf16 De = 16 sums; nulls: the operands a (pass, op) does not read are NULL; 0: all are given
CASES = [(4, 1, torch.float32, 1, True, 1), (24, 3, torch.float32, 0, True, 2), (24, 16, torch.float32, 1, False, 1),
         (260, 8, torch.float32, 1, True, 1), (260, 8, torch.float32, 0, True, 2),
         (8, 3, torch.bfloat16, 0, True, 2), (48, 8, torch.bfloat16, 1, False, 1), (48, 16, torch.bfloat16, 1, True, 2),
         (520, 16, torch.bfloat16, 1, True, "tiles"), (520, 1, torch.bfloat16, 0, True, 2)]


@pytest.mark.parametrize("dyadic", [True, False], ids=["dyadic", "random"])
@pytest.mark.parametrize("F,De,dtype,nulls,bias,partials", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_all_passes_in_lock_step(emulator, tmp_path, F, De, dtype, nulls, bias, partials, dyadic):
    _run(emulator, tmp_path, _graph(full=F < 260), F, De, dtype, dyadic, nulls, bias, partials)
