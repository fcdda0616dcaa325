#!/usr/bin/env python3
"""Per-pass timing and peak memory of the fused edge projection (csrc/edge_proj.hip: FORWARD, COLS, PARAM, DOTS) next to the
composition it replaces -- torch's Linear over the edge attributes into a real e [nnz, F], then the ops_ef pass of the same name
(for PARAM: ops_ef's EDGE pass into a real grad_e [nnz, F], then the Linear's backward grad_e.T @ a and grad_e.sum(0); for DOTS the
further grad_e @ W) -- and next to the floor by traffic: ops.spmm of the same width over A (over A^T for COLS) plus one streamed
read of a (nnz * pitch of a), which is printed as bytes and as the time at the card's measured copy rate.

    python tools/edge_proj_bench.py --graph reddit|products [--reps 3 --rounds 1 --widths 64 --dtypes bf16,fp32 --des 4,16 --ops add_relu]

Synthetic graphs as tools/edge_feat_bench.py (reddit-shaped: 232 965 nodes, 57.3 M undirected edges; products-shaped:
synth.products_like_graph defaults), with self-loops.  HIP events round `reps` launches after two warm-up launches, one process on the
card; the median of `rounds` is reported.  The composition's e and grad_e are real arrays: a shape where they do not fit the card's
free memory runs the fused passes alone, with a note.  Peak memory: torch's allocator peak over one forward and backward through
autograd (all five gradients), above what is allocated before it, for the fused op and for the composition.  Prints a table and one
JSON line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dgll_amd import _lib, ops, ops_ef, ops_efp, synth  # noqa: E402

GRAPHS = {"products": dict(), "reddit": dict(n=232_965, n_undirected=57_300_000)}
OPS = {"add": _lib.EF_ADD, "add_relu": _lib.EF_ADD_RELU, "mul": _lib.EF_MUL}
ACT = {"add": ("add", None), "add_relu": ("add", "relu"), "mul": ("mul", None)}


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


def peak_of(fn, leaves, go):
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn(*leaves).backward(go)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - before
    for t in leaves:
        t.grad = None
    return used


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=sorted(GRAPHS), default="reddit")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--widths", default="64")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--des", default="4,16")
    ap.add_argument("--ops", default="add_relu")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = synth.products_like_graph(dev, seed=0, locality=0.9, self_loops=True, **GRAPHS[args.graph])
    gt, _ = g.transpose()
    g.plan(), gt.plan()
    n, nnz = g.n_rows, g.nnz
    print("%s-shaped graph: %d nodes, %d entries" % (args.graph, n, nnz), flush=True)
    src = torch.empty(1 << 28, device=dev, dtype=torch.uint8)
    dst = torch.empty_like(src)
    copy_gbs = 2 * src.numel() / timeit(lambda: dst.copy_(src), 5) / 1e6         # read + write
    del src, dst
    result = {"graph": args.graph, "nodes": n, "nnz": nnz, "copy_GBps": round(copy_gbs, 1), "shapes": {}}
    torch.manual_seed(0)
    for name in args.dtypes.split(","):
        dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[name]
        esz = 2 if dtype == torch.bfloat16 else 4
        for F in (int(w) for w in args.widths.split(",")):
            for De in (int(v) for v in args.des.split(",")):
                key = "%s_F%d_De%d" % (name, F, De)
                x = torch.randn(n, F, device=dev).to(dtype)
                go = torch.randn(n, F, device=dev).to(dtype)
                a = ops.as_rows16(torch.empty(nnz, De, device=dev, dtype=dtype).normal_())
                W = (torch.randn(F, De, device=dev) / De ** 0.5)
                b = torch.randn(F, device=dev)
                wt, bk = ops_efp.kernel_weights(W, b)
                a_bytes, e_bytes = nnz * a.stride(0) * esz, nnz * F * esz
                a_ms = a_bytes / copy_gbs / 1e6
                print("%s: a is %.2f GB (%.3f ms at the copy rate of %.0f GB/s), e would be %.2f GB" % (key, a_bytes / 1e9, a_ms, copy_gbs,
                                                                                                     e_bytes / 1e9), flush=True)
                free = torch.cuda.mem_get_info(dev)[0]
                composed = 3.3 * e_bytes < free             # e, grad_e, and the e its timed forward builds anew
                if not composed:
                    print("  composition skipped: its [nnz, F] arrays need %.1f GB, %.1f GB are free" % (3.3 * e_bytes / 1e9, free / 1e9), flush=True)
                table = {"spmm": lambda: ops.spmm_raw(g, x, reduce="sum"), "spmm_t": lambda: ops.spmm_raw(gt, go, reduce="sum")}
                Wc, bc = W.to(dtype), b.to(dtype)
                if composed:
                    e = torch.nn.functional.linear(a, Wc, bc)
                    ge = torch.empty(nnz, F, device=dev, dtype=dtype)
                for op_name in args.ops.split(","):
                    op = OPS[op_name]
                    table["forward %s fused" % op_name] = lambda op=op: ops_efp.forward_raw(g, x, a, wt, bk, op)
                    table["cols %s fused" % op_name] = lambda op=op: ops_efp.cols_raw(g, x, a, wt, bk, go, op)
                    table["param %s fused" % op_name] = lambda op=op: ops_efp.param_raw(g, x, a, wt, bk, go, op)
                    table["dots %s fused" % op_name] = lambda op=op: ops_efp.param_raw(g, x, a, wt, bk, go, op, want_a=True, want_w=False)
                    if composed:
                        table["forward %s composed" % op_name] = lambda op=op: ops_ef.forward_raw(g, x, torch.nn.functional.linear(a, Wc, bc), op)
                        table["cols %s composed" % op_name] = lambda op=op: ops_ef.cols_raw(g, x, e, go, op)
                        table["param %s composed" % op_name] = lambda op=op: (ops_ef.edge_raw(g, x, e, go, op, out=ge), ge.t() @ a, ge.sum(0))
                        table["dots %s composed" % op_name] = lambda op=op: (ops_ef.edge_raw(g, x, e, go, op, out=ge), ge @ Wc)
                samples = {k: [] for k in table}
                for _ in range(args.rounds):
                    for k, fn in table.items():
                        samples[k].append(timeit(fn, args.reps))
                row = {k: statistics.median(v) for k, v in samples.items()}
                if composed:
                    del e, ge
                del table
                torch.cuda.empty_cache()
                for k, ms in row.items():
                    note = ""
                    if k.endswith("fused"):
                        floor = row["spmm_t" if k.startswith("cols") else "spmm"] + a_ms
                        note = "  %.2fx the floor (spmm + a)" % (ms / floor)
                        other = k[:-5] + "composed"
                        if other in row:
                            note += ", %.2fx the composition" % (ms / row[other])
                    print("  %-30s %9.3f ms%s" % (k, ms, note), flush=True)
                op_name = args.ops.split(",")[0]
                leaves = [t.clone().requires_grad_() for t in (x, a, W, b)]
                fused = lambda x_, a_, W_, b_: ops_efp.u_op_proj_e_sum(g, x_, a_, W_, b_, *ACT[op_name])                        # noqa: E731
                comp = lambda x_, a_, W_, b_: ops_ef.u_op_e_sum(g, x_, torch.nn.functional.linear(a_, W_.to(dtype), b_.to(dtype)),    # noqa: E731
                                                                 *ACT[op_name])
                peaks = {"peak fused": peak_of(fused, leaves, go)}
                if composed:
                    peaks["peak composed"] = peak_of(comp, leaves, go)
                for k, v in peaks.items():
                    print("  %-30s %9.1f MB (forward and backward, above the inputs)" % (k, v / 1e6), flush=True)
                result["shapes"][key] = dict({k: round(ms, 4) for k, ms in row.items()}, a_bytes=a_bytes, e_bytes=e_bytes,
                                             a_ms_at_copy_rate=round(a_ms, 4), **{k.replace(" ", "_") + "_bytes": v for k, v in peaks.items()})
                del x, go, a, leaves
                torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
