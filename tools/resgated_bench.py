#!/usr/bin/env python3
"""Per-pass timing of the three ResGated passes (csrc/res_gated.hip: FORWARD, ROWS, COLS) at F = 64 and 256, bf16 and fp32, next to
three comparisons:

  (a) ops.spmm of the same width over A: the gather of ONE operand.  Every ResGated pass gathers two rows per entry, so its floor by
      traffic is two such gathers;
  (b) the three ops_gated passes (csrc/gated.hip) at the same shape, with a real c [nnz, F]: the same gathers plus streamed per-edge
      arrays, strictly more bytes.  A shape whose per-edge arrays do not fit the card's free memory is skipped with a note;
  (c) on the Reddit shape, the torch composition the passes replace: sigmoid(k[row] + q[col]) * v[col] into one index_add_, and its
      autograd backward (skipped where its [nnz, F] temporaries do not fit).

Also timed: FORWARD and ROWS with q and v as the two halves of ONE [n_src, 2F] buffer (pitched views: the two gathers of an entry
then hit adjacent lines), COLS with one output alone, and FORWARD with `mean`.

    python tools/resgated_bench.py --graph reddit|products [--reps 3 --rounds 1 --widths 64,256 --dtypes bf16,fp32 --no-gated]

Synthetic graphs (reddit-shaped: 232 965 nodes, 57.3 M undirected edges; products-shaped: synth.products_like_graph defaults), with
self-loops.  HIP events round `reps` launches after two warm-up launches, one process on the card; the median of `rounds` is
reported.  Prints a table and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dgll_amd import ops, ops_gated, ops_res_gated, synth  # noqa: E402

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
    ap.add_argument("--no-gated", action="store_true", help="leave out the ops_gated passes")
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
            print("F = %d %s: the node arrays are %.3f GB each; one [nnz, F] array would be %.2f GB" %
                  (F, name, n * F * (2 if dtype == torch.bfloat16 else 4) / 1e9, e_bytes / 1e9), flush=True)
            k, q, v, go = (torch.randn(n, F, device=dev).to(dtype) for _ in range(4))
            qv = torch.cat([q, v], 1)                       # q and v as the halves of one product
            qh, vh = qv[:, :F], qv[:, F:]
            row = {"spmm": med(lambda: ops.spmm_raw(g, v, reduce="sum")),
                   "forward": med(lambda: ops_res_gated.forward_raw(g, k, q, v)),
                   "forward (mean)": med(lambda: ops_res_gated.forward_raw(g, k, q, v, True)),
                   "forward (q|v one buffer)": med(lambda: ops_res_gated.forward_raw(g, k, qh, vh)),
                   "rows": med(lambda: ops_res_gated.rows_raw(g, k, q, v, go)),
                   "rows (q|v one buffer)": med(lambda: ops_res_gated.rows_raw(g, k, qh, vh, go)),
                   "cols": med(lambda: ops_res_gated.cols_raw(g, k, q, v, go)),
                   "cols (grad_q alone)": med(lambda: ops_res_gated.cols_raw(g, k, q, v, go, True, False)),
                   "cols (grad_v alone)": med(lambda: ops_res_gated.cols_raw(g, k, q, v, go, False, True))}
            row["floor (2 x spmm)"] = 2 * row["spmm"]
            del qv, qh, vh

            free = torch.cuda.mem_get_info(dev)[0]
            if args.no_gated:
                pass
            elif 3.4 * e_bytes > free:
                print("  ops_gated skipped: its per-edge arrays (c, ehat, grad_c) need %.1f GB, %.1f GB are free"
                      % (3.4 * e_bytes / 1e9, free / 1e9), flush=True)
            else:
                c = torch.zeros(nnz, F, device=dev, dtype=dtype)
                row["gated forward"] = med(lambda: ops_gated.forward_raw(g, k, q, c, v, EPS))
                out, ehat, inv_s, out32 = ops_gated.forward_raw(g, k, q, c, v, EPS)
                del c
                row["gated rows"] = med(lambda: ops_gated.rows_raw(g, v, ehat, inv_s, out32, go, None, EPS))
                gc, _, w = ops_gated.rows_raw(g, v, ehat, inv_s, out32, go, None, EPS)
                row["gated cols"] = med(lambda: ops_gated.cols_raw(g, gc, ehat, w, eps=EPS))
                del out, ehat, inv_s, out32, gc, w
                torch.cuda.empty_cache()

            def torch_composed(backward):
                ins = [t.detach().requires_grad_(backward) for t in (k, q, v)]
                res = torch.zeros(n, F, device=dev, dtype=dtype).index_add_(0, rows, torch.sigmoid(ins[0][rows] + ins[1][col]) * ins[2][col])
                if backward:
                    res.backward(go)

            if args.graph == "reddit":
                free = torch.cuda.mem_get_info(dev)[0]
                if 9 * e_bytes > free:      # the three gathers, the sum, the gate, the product, and their gradients
                    print("  torch composition skipped: its [nnz, F] temporaries need about %.1f GB, %.1f GB are free"
                          % (9 * e_bytes / 1e9, free / 1e9), flush=True)
                else:
                    fwd = med(lambda: torch_composed(False))
                    both = med(lambda: torch_composed(True))
                    row["torch forward"], row["torch backward"] = fwd, both - fwd
                    torch.cuda.empty_cache()
            for label, ms in row.items():
                print("  %-26s %9.3f ms" % (label, ms), flush=True)
            result["shapes"][key] = dict({label: round(ms, 4) for label, ms in row.items()}, e_bytes=e_bytes)
            del k, q, v, go
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
