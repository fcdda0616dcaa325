#!/usr/bin/env python3
"""Per-pass timing of the three gated-aggregation passes (csrc/gated.hip: FORWARD, ROWS, COLS) at F = 64 and 256, bf16 and fp32,
next to three comparisons:

  (a) the torch composition the passes replace: sigmoid(c + a[row] + b[col]) into two index_add_ and a division, and its autograd
      backward;
  (b) the same composed from the engine's general ops: ops_mp.u_add_v (fp32 per-edge), a torch sigmoid, ops_ef.u_mul_e_sum_full, the
      denominator gather ops_mp.copy_e_sum, a torch division -- forward, and forward plus autograd backward;
  (c) the floor by traffic: ops.spmm of the same width over A (the gather of one operand) plus one streamed read of c and one write
      of ehat, timed as a device copy of an [nnz, F] array.

    python tools/gated_bench.py --graph reddit|products [--reps 3 --rounds 1 --widths 64,256 --dtypes bf16,fp32]

Synthetic graphs (reddit-shaped: 232 965 nodes, 57.3 M undirected edges; products-shaped: synth.products_like_graph defaults), with
self-loops.  HIP events round `reps` launches after two warm-up launches, one process on the card; the median of `rounds` is
reported.  c, ehat, grad_ehat and grad_c are real [nnz, F] arrays: their bytes are printed, and a shape whose arrays do not fit the
card's free memory is skipped with a note (as are the compositions where their temporaries do not fit).  Prints a table and one JSON
line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dgll_amd import ops, ops_ef, ops_gated, ops_mp, synth  # noqa: E402

GRAPHS = {"products": dict(), "reddit": dict(n=232_965, n_undirected=57_300_000)}
EPS = 1e-6


def timeit(fn, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=sorted(GRAPHS), default="reddit")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--widths", default="64,256")
    ap.add_argument("--dtypes", default="bf16,fp32")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = synth.products_like_graph(dev, seed=0, locality=0.9, self_loops=True, **GRAPHS[args.graph])
    g.transpose()
    g.plan()
    n, nnz = g.n_rows, g.nnz
    rows, col = g.row_index(), g.col.long()
    print("%s-shaped graph: %d nodes, %d entries" % (args.graph, n, nnz), flush=True)
    result = {"graph": args.graph, "nodes": n, "nnz": nnz, "shapes": {}}
    torch.manual_seed(0)
    med = lambda fn: statistics.median(timeit(fn, args.reps) for _ in range(args.rounds))      # noqa: E731
    for name in args.dtypes.split(","):
        dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[name]
        for F in (int(w) for w in args.widths.split(",")):
            key = "%s_F%d" % (name, F)
            e_bytes = nnz * F * (2 if dtype == torch.bfloat16 else 4)
            free = torch.cuda.mem_get_info(dev)[0]
            print("F = %d %s: c is %.2f GB (ehat, grad_ehat and grad_c as much)" % (F, name, e_bytes / 1e9), flush=True)
            if 4.4 * e_bytes > free:
                print("  skipped: the four per-edge arrays need %.1f GB, %.1f GB are free" % (4.4 * e_bytes / 1e9, free / 1e9), flush=True)
                result["shapes"][key] = {"e_bytes": e_bytes, "skipped": "memory"}
                continue
            a, b, v, go = (torch.randn(n, F, device=dev).to(dtype) for _ in range(4))
            c = torch.empty(nnz, F, device=dev, dtype=dtype).normal_()
            ge = torch.empty(nnz, F, device=dev, dtype=dtype).normal_()
            # at most four [nnz, F] arrays are alive at any time: c, ge, ehat and one grad_c (every raw pass allocates its outputs)
            row = {"spmm": med(lambda: ops.spmm_raw(g, v, reduce="sum")),
                   "copy [nnz, F]": med(lambda: ge.copy_(c)),
                   "forward": med(lambda: ops_gated.forward_raw(g, a, b, c, v, EPS))}
            ge.normal_()
            out, ehat, inv_s, out32 = ops_gated.forward_raw(g, a, b, c, v, EPS)
            row["rows"] = med(lambda: ops_gated.rows_raw(g, v, ehat, inv_s, out32, go, ge, EPS))
            row["rows (no grad_ehat)"] = med(lambda: ops_gated.rows_raw(g, v, ehat, inv_s, out32, go, None, EPS))
            gc, _, w = ops_gated.rows_raw(g, v, ehat, inv_s, out32, go, ge, EPS)
            row["cols"] = med(lambda: ops_gated.cols_raw(g, gc, ehat, w, eps=EPS))
            row["floor (spmm + copy)"] = row["spmm"] + row["copy [nnz, F]"]
            del out, ehat, inv_s, out32, gc, w
            torch.cuda.empty_cache()

            def torch_composed(backward):
                ins = [t.detach().requires_grad_(backward) for t in (a, b, c, v)]
                eh = ins[2] + ins[0][rows] + ins[1][col]
                sig = torch.sigmoid(eh)
                num = torch.zeros(n, F, device=dev, dtype=dtype).index_add_(0, rows, sig * ins[3][col])
                den = torch.zeros(n, F, device=dev, dtype=dtype).index_add_(0, rows, sig)
                res = num / (den + EPS)
                if backward:
                    torch.autograd.backward([res, eh], [go, ge])

            def engine_composed(backward):
                ins = [t.detach().requires_grad_(backward) for t in (a, b, c, v)]
                eh = ins[2].float() + ops_mp.u_add_v(g, ins[1].float(), ins[0].float())
                sig = torch.sigmoid(eh)
                num = ops_ef.u_mul_e_sum_full(g, ins[3], sig.to(dtype))
                den = ops_mp.copy_e_sum(g, sig)
                res = num.float() / (den + EPS)
                if backward:
                    torch.autograd.backward([res, eh], [go.float(), ge.float()])

            # the gathers, the sum, the gate, the product and what autograd keeps of them, in fp32 for (b): about a dozen arrays like c
            for label, fn, arrays in (("torch", torch_composed, 10), ("engine ops", engine_composed, 16 if dtype == torch.bfloat16 else 10)):
                free = torch.cuda.mem_get_info(dev)[0]
                if arrays * e_bytes > free:
                    print("  %s composition skipped: its [nnz, F] temporaries need about %.1f GB, %.1f GB are free"
                          % (label, arrays * e_bytes / 1e9, free / 1e9), flush=True)
                    continue
                fwd = med(lambda: fn(False))
                both = med(lambda: fn(True))
                row[label + " forward"], row[label + " backward"] = fwd, both - fwd
                torch.cuda.empty_cache()
            for k, ms in row.items():
                print("  %-26s %9.3f ms" % (k, ms), flush=True)
            result["shapes"][key] = dict({k: round(ms, 4) for k, ms in row.items()}, e_bytes=e_bytes)
            del a, b, v, go, c, ge
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
