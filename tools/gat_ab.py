#!/usr/bin/env python3
"""Per-pass timing of the three GAT gather passes next to the SpMM at the same width on the same graph (config 4 shape:
8 heads x 32 = 256 columns bf16, products-sized graph + self-loops, engine reorder).  HIP events, `reps` launches each.

    python tools/gat_ab.py [locality] [probe-list]     probe-list: comma-separated dgll_hip_debug_tune(8, v) values
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dgll_amd import _lib, ops, ops_edge, synth  # noqa: E402

dev = torch.device("cuda:0")
loc = float(sys.argv[1]) if len(sys.argv) > 1 else 0.9
probes = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [0]
unrolls = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [2]
g = synth.products_like_graph(dev, seed=0, locality=loc, self_loops=True, exact=True, permute_ids=True)
g = g.reorder(method="lpa", seed=0)[0]
gt, perm = g.transpose()
g.plan(), gt.plan()
heads, fo = 8, 32
n, F = g.n_rows, heads * fo
torch.manual_seed(0)
h = torch.randn(n, F, device=dev).to(torch.bfloat16)
s = torch.randn(n, heads, device=dev)
t = torch.randn(n, heads, device=dev)
go = torch.randn(n, F, device=dev).to(torch.bfloat16)
w = torch.rand(g.nnz, device=dev)


def timeit(fn, reps=10):
    fn()
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


out = torch.empty_like(h)
rowsum = torch.empty(n, heads, device=dev)
dn = torch.empty_like(h)
dd = torch.empty(n, heads, device=dev)
gs = torch.empty(n, heads, device=dev)
gh = torch.empty_like(h)
gtt = torch.empty(n, heads, device=dev)

ref = {
    "spmm mean unweighted A": timeit(lambda: ops.spmm_raw(g, h, reduce="mean")),
    "spmm sum weighted A^T": timeit(lambda: ops.spmm_raw(gt, h, val=w, reduce="sum")),
}
for k, v in ref.items():
    print("%-28s %.3f ms" % (k, v), flush=True)
b_alg = g.nnz * (F * 2 + 4 + 4 * heads) + n * (F * 2 + 8 + 8 * heads)
gens = [int(v) for v in sys.argv[4].split(",")] if len(sys.argv) > 4 else [0]
sd = torch.empty(n, 2 * heads, device=dev)
for gen in gens:
    _lib.lib.dgll_hip_debug_tune(9, gen)
    f = timeit(lambda: ops_edge.gat_fwd_part(g, h, s, t, out, rowsum, heads, fo, 0.2, 1, 0, 0))
    r = timeit(lambda: ops_edge.gat_bwd_rows_part(g, h, s, t, out, go, rowsum, dn, dd, gs, heads, fo, 0.2, 1, 0))
    c = timeit(lambda: ops_edge.gat_bwd_cols_part(gt, dn, h, t, s, dd, gh, gtt, heads, fo, 0.2))
    base = ref["spmm mean unweighted A"]
    print("gen %d: fwd %.3f ms (%.2fx spmm, alg %.0f GB/s = %.2f of 8 TB/s) | bwd_rows %.3f ms (%.2fx) | "
          "bwd_cols (separate S, DD arrays) %.3f ms (%.2fx)" % (gen, f, f / base, b_alg / f / 1e6, b_alg / f / 1e6 / 8000, r, r / base,
                                                               c, c / base), flush=True)
    if gen == 0:   # both backward passes in the strided form ({s, dd} side by side): cols = total - rows
        ws = ops_edge._ws(g.plan(), heads, fo, dev, gt.plan())

        def both():
            ops_edge._gat_pass(_lib.GAT_ROWS, g, heads, fo, 0.2, h, apply_elu=1, ws=ws, phase=_lib.GAT_ROWS_EXACT_ONLY, row_score=s.data_ptr(),
                               col_score=t.data_ptr(), col_score_stride=heads, out=out.data_ptr(), ld_out=out.stride(0),
                               grad_out=go.data_ptr(), ld_grad_out=go.stride(0), rowsum=rowsum.data_ptr(), dn=dn.data_ptr(),
                               ld_dn=dn.stride(0), sd=sd.data_ptr(), sd_stride=2 * heads, grad_score=gs.data_ptr())
            ops_edge._gat_pass(_lib.GAT_TRANSPOSED, gt, heads, fo, 0.2, h, ws=ws, dn=dn.data_ptr(), ld_dn=dn.stride(0),
                               row_score=t.data_ptr(), col_score=sd.data_ptr(), col_dd=sd.data_ptr() + 4 * heads,
                               col_score_stride=2 * heads, grad_h=gh.data_ptr(), ld_grad_h=gh.stride(0), grad_score=gtt.data_ptr())

        bt = timeit(both)
        print("gen 0: both backward passes, {s, dd} side by side: %.3f ms -> bwd_cols %.3f ms (%.2fx)" % (bt, bt - r, (bt - r) / base),
              flush=True)
_lib.lib.dgll_hip_debug_tune(9, 0)
