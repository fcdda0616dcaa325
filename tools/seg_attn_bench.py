"""Times segment_attention (csrc/seg_attn.hip), forward and backward, next to the composition it replaces: the same graphs padded to
[B, heads, max_n, D] and run through torch.nn.functional.scaled_dot_product_attention with a key mask.

    python tools/seg_attn_bench.py [--rounds 5] [--heads 4] [--out FILE.json]

Shapes: 512 graphs of 20-40 nodes (seeded), and 8 graphs of 4 000 nodes; fp32 and bf16; D = 32 and 64.  Both sides run in this one
process, in alternating rounds after a warm-up of every shape, each pass between device events; the figure is the median round.
The padded side is timed on inputs that are ALREADY padded and its output is left padded: to_dense_batch and the gather back are not
charged to it.  Prints one line per case with the ratio torch / ours per pass (> 1: segment_attention is faster).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dgll_amd.ops_dense_attn import segment_attention  # noqa: E402

DEV = "cuda"


def shapes():
    gen = torch.Generator().manual_seed(0)
    return {"512 graphs of 20-40": torch.randint(20, 41, (512,), generator=gen).tolist(), "8 graphs of 4000": [4000] * 8}


def timed(prepare, run, iters):
    """ms per call of run(state), state = prepare() outside the timed window"""
    spans = []
    for _ in range(iters):
        state = prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run(state)
        b.record()
        spans.append((a, b))
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in spans) / iters


def case(sizes, heads, D, dtype, rounds):
    n, B, mx = sum(sizes), len(sizes), max(sizes)
    gen = torch.Generator().manual_seed(1)
    q, k, v, g = (torch.randn(n, heads * D, generator=gen).to(dtype).to(DEV).requires_grad_(i < 3) for i in range(4))
    rows = torch.cat([torch.arange(s) + i * mx for i, s in enumerate(sizes)]).to(DEV)
    pad = lambda t: torch.zeros(B * mx, heads, D, dtype=dtype, device=DEV).index_copy_(0, rows, t.detach().view(n, heads, D)) \
        .view(B, mx, heads, D).transpose(1, 2).contiguous()                                                     # noqa: E731
    qp, kp, vp, gp = (pad(t).requires_grad_(i < 3) for i, t in enumerate((q, k, v, g)))
    mask = torch.zeros(B * mx, dtype=torch.bool, device=DEV).index_fill_(0, rows, True).view(B, 1, 1, mx)
    ours = lambda: segment_attention(q, k, v, heads, segs=sizes)                                                # noqa: E731
    theirs = lambda: torch.nn.functional.scaled_dot_product_attention(qp, kp, vp, attn_mask=mask)              # noqa: E731
    sides = {"ours": (ours, (q, k, v), g), "torch": (theirs, (qp, kp, vp), gp)}
    iters = max(3, min(200, int(4e8 / (sum(s * s for s in sizes) * heads * D / 32))))        # a window of some tens of ms per side
    res = {name + "_" + p: [] for name in sides for p in ("fwd", "bwd")}
    for rnd in range(rounds + 1):                           # round 0 is the warm-up
        for name, (fn, leaves, go) in sides.items():
            f = timed(lambda: None, lambda _: fn(), iters)
            b = timed(fn, lambda out: torch.autograd.grad(out, leaves, go), iters)
            if rnd:
                res[name + "_fwd"].append(f)
                res[name + "_bwd"].append(b)
    med = {k_: statistics.median(v_) for k_, v_ in res.items()}
    med.update(ratio_fwd=med["torch_fwd"] / med["ours_fwd"], ratio_bwd=med["torch_bwd"] / med["ours_bwd"], iters=iters,
               spread={k_: (min(v_), max(v_)) for k_, v_ in res.items()})
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_attn_bench needs the GPU: there is nothing to time without one")
    results = []
    for label, sizes in shapes().items():
        for dtype in (torch.float32, torch.bfloat16):
            for D in (32, 64):
                r = case(sizes, args.heads, D, dtype, args.rounds)
                r.update(shape=label, dtype=str(dtype), D=D, heads=args.heads)
                results.append(r)
                print("%-20s %-14s D=%-3d fwd ours %8.3f ms torch %8.3f ms (x%5.2f)   bwd ours %8.3f ms torch %8.3f ms (x%5.2f)"
                      % (label, dtype, D, r["ours_fwd"], r["torch_fwd"], r["ratio_fwd"], r["ours_bwd"], r["torch_bwd"], r["ratio_bwd"]),
                      flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
