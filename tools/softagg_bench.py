#!/usr/bin/env python3
"""Per-pass timing of the three soft-aggregation passes (csrc/soft_agg.hip: FORWARD, ROWS, COLS) at F = 64 and 256, bf16 and fp32,
both modes (softmax, power mean), with and without e, next to:

  (a) ops.spmm of the same width over A: the gather of x alone, the traffic floor of every pass without e;
  (b) the ops_ef ADD_RELU passes (csrc/edge_feat.hip) of the same width: the same gather plus the same streamed e and the same relu
      gate with a plain sum, the traffic floor of every pass with e.  A shape whose [nnz, F] operands do not fit the card's free
      memory is run without e, with a note;
  (c) on the Reddit shape, the torch composition the passes replace (relu(x[col] + e) + eps, a scatter softmax per column, one
      index_add_) and its autograd backward, skipped where its [nnz, F] temporaries do not fit.

Also: the peak memory of one forward + backward of the autograd op above its inputs, next to the size of one [nnz, F] array.

    python tools/softagg_bench.py --graph reddit|products [--reps 3 --rounds 1 --widths 64,256 --dtypes bf16,fp32 --modes softmax,power]

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

from dgll_amd import _lib, ops, ops_ef, ops_softagg, synth  # noqa: E402

GRAPHS = {"products": dict(), "reddit": dict(n=232_965, n_undirected=57_300_000)}
EPS = 1e-7
MODES = {"softmax": (ops_softagg.SOFTMAX, 1.0), "power": (ops_softagg.POWER, 2.0)}


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
    ap.add_argument("--modes", default="softmax,power")
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
            print("F = %d %s: the node arrays are %.3f GB each; one [nnz, F] array is %.2f GB" %
                  (F, name, n * F * (2 if dtype == torch.bfloat16 else 4) / 1e9, e_bytes / 1e9), flush=True)
            x, go = (torch.randn(n, F, device=dev).to(dtype) for _ in range(2))
            row = {"spmm": med(lambda: ops.spmm_raw(g, x, reduce="sum"))}
            free = torch.cuda.mem_get_info(dev)[0]
            e = None
            if 2.3 * e_bytes > free:        # e and grad_e
                print("  without e: e and grad_e need %.1f GB, %.1f GB are free" % (2.3 * e_bytes / 1e9, free / 1e9), flush=True)
            else:
                e = torch.randn(nnz, F, device=dev).to(dtype)
                row["ef add_relu forward"] = med(lambda: ops_ef.forward_raw(g, x, e, _lib.EF_ADD_RELU))
                row["ef add_relu cols"] = med(lambda: ops_ef.cols_raw(g, x, e, go, _lib.EF_ADD_RELU))
                ge = torch.empty_like(e)
                row["ef add_relu edge"] = med(lambda: ops_ef.edge_raw(g, x, e, go, _lib.EF_ADD_RELU, out=ge))
                del ge
            for mode in args.modes.split(","):
                code, value = MODES[mode]
                th = torch.full((1,), value, device=dev)
                for tag, ee in (("", None),) + ((("+e", e),) if e is not None else ()):
                    label = mode + tag
                    row[label + " forward"] = med(lambda: ops_softagg.forward_raw(g, code, x, ee, th, EPS))
                    _, stats = ops_softagg.forward_raw(g, code, x, ee, th, EPS)
                    row[label + " rows (scalar)"] = med(lambda: ops_softagg.rows_raw(g, code, x, ee, th, EPS, stats, go, need_e=False))
                    if ee is not None:
                        row[label + " rows (grad_e, scalar)"] = med(lambda: ops_softagg.rows_raw(g, code, x, ee, th, EPS, stats, go))
                    row[label + " cols"] = med(lambda: ops_softagg.cols_raw(g, code, x, ee, th, EPS, stats, go))
                    del stats
                # the peak of one forward + backward of the autograd op, without e, a learned scalar
                op = ops_softagg.softmax_aggregate if mode == "softmax" else ops_softagg.powermean_aggregate
                xg, tg = x.clone().requires_grad_(), th.clone().requires_grad_()
                op(g, xg, None, tg, eps=EPS).backward(go)
                xg.grad = tg.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                op(g, xg, None, tg, eps=EPS).backward(go)
                torch.cuda.synchronize()
                row[mode + " peak MB (fwd + bwd, no e)"] = (torch.cuda.max_memory_allocated() - before) / 1e6
                del xg, tg

            def torch_composed(backward):
                xs = x.detach().requires_grad_(backward)
                es = e.detach().requires_grad_(backward)
                m = torch.relu(xs[col] + es) + EPS
                index = rows.unsqueeze(1).expand(-1, F)
                top = torch.full((n, F), -float("inf"), device=dev, dtype=dtype).scatter_reduce(0, index, m.detach(), "amax")
                w = torch.exp(m - top[rows])
                a = w / torch.zeros(n, F, device=dev, dtype=dtype).index_add_(0, rows, w)[rows]
                res = torch.zeros(n, F, device=dev, dtype=dtype).index_add_(0, rows, a * m)
                if backward:
                    res.backward(go)

            if args.graph == "reddit" and e is not None:
                free = torch.cuda.mem_get_info(dev)[0]
                if 12 * e_bytes > free:     # the gather, the sum, m, the index, w, the gathered maxima and sums, a, a m, and their gradients
                    print("  torch composition skipped: its [nnz, F] temporaries need about %.1f GB, %.1f GB are free"
                          % (12 * e_bytes / 1e9, free / 1e9), flush=True)
                else:
                    fwd = med(lambda: torch_composed(False))
                    both = med(lambda: torch_composed(True))
                    row["torch softmax+e forward"], row["torch softmax+e backward"] = fwd, both - fwd
                    torch.cuda.empty_cache()
            for label, v in row.items():
                print("  %-36s %9.3f %s" % (label, v, "MB" if "peak" in label else "ms"), flush=True)
            result["shapes"][key] = dict({label: round(v, 4) for label, v in row.items()}, e_bytes=e_bytes)
            del x, go, e
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
