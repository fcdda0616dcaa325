"""What tests/test_segment_mm_gpu.py and tests/test_segment_mm_edges_gpu.py share: the segment lists, the operand builder, the float64
Problems, one run of the public operator into a sentinel buffer, and the comparison of one result on either leg (the comparators and
bars are those of tests/dense_small_cases.py).  Imports with torch on the CPU alone."""
import torch

import dense_small_cases as sc
from segmm_ref import grouped_refs

EDGES = [0, 1, 0, 31, 32, 33, 0]     # empty first, middle and last segments; the wave tile's edge
WG = [127, 128, 129]                 # four tiles of one segment side by side
ONE = [300]                          # one segment: every tile reuses the weight
SHORT = [1, 2, 3] * 14               # the weight changes every tile
SLAB = [700, 1, 1, 5]                # a slab-split grad_b segment next to single-row ones
DTYPES = [torch.bfloat16, torch.float32]


def operands(seglen, k, n, extra_types, exact, bf16, seed):
    """float64 a, b, g holding values exact in the operand format, and the two |.| bounds' ingredients."""
    gen = torch.Generator().manual_seed(seed)
    m, r = sum(seglen), len(seglen) + extra_types
    a, g = sc._draw(gen, (m, k), exact, bf16), sc._draw(gen, (m, n), exact, bf16)
    b = sc._draw(gen, (r, k, n), exact, bf16, scale=0.1)
    return a, b, g


def problems(a, b, g, idx):
    refs, bounds = grouped_refs(a, b, g, idx), grouped_refs(a.abs(), b.abs(), g.abs(), idx)
    reductions = (a.shape[1], g.shape[1], int(torch.bincount(idx, minlength=1).max()))
    return [sc.Problem(None, None, None, None, ref, bound, red) for ref, bound, red in zip(refs, bounds, reductions)]


def run(op, a, b, g, grouping, dtype, device):
    """(c in its sentinel buffer, grad_a, grad_b) of the public operator; the forward once more through the raw product into the buffer."""
    from dgll_amd import ops_segmm

    m, n = g.shape
    pitch = sc.bf16_pitch(a.shape[1]) if dtype == torch.bfloat16 else sc.f32_pitch(a.shape[1], "vec")[0]
    ad = sc.padded(a, device, dtype, pitch, spare_rows=2).requires_grad_(True)
    bd = b.to(device=device, dtype=torch.float32).requires_grad_(True)      # an fp32 parameter, under bf16 activations too: grad_b is fp32
    c = ops_segmm.gather_mm(ad, bd, idx_b=grouping) if op == "gather" else ops_segmm.segment_mm(ad, bd, grouping)
    c.backward(g.to(device=device, dtype=dtype))
    buf = sc.sentinel_buffer(m + 3, n + 5, dtype, device)
    if op == "gather":
        ids, rows = torch.sort(grouping, stable=True)
        seglen = torch.bincount(ids, minlength=b.shape[0])
    else:
        seglen, rows = grouping, None
    ops_segmm._product_raw(ad.detach(), bd.detach(), seglen, rows, False, out=buf[:m, :n])
    assert torch.equal(buf[:m, :n], c), "the operator and the raw product differ"
    return buf, ad.grad[:, :a.shape[1]], bd.grad


def check(name, got, p, exact, dtype, kind, slabs=2):
    """slabs: an upper bound on the slab count of grad_b's longest segment (the S of f32_random_ok)."""
    bf16 = dtype == torch.bfloat16
    assert bool(torch.isfinite(got).all()), (name, kind, "NaN from the padding or the workspace")
    print("%s %s: max |err| / (|A| |B|) = %.3g" % (name, kind, sc.error_ratio(got, p.ref, p.bound)))
    if exact:
        assert sc.exactness_holds(p)
        assert sc.exact_ok(got, p.ref, bf16_out=bf16 and kind != "grad_b"), (name, kind, float((got.double().cpu() - p.ref).abs().max()))
    elif not bf16:
        assert sc.f32_random_ok(got, p.ref, p.bound, p.R, slabs), (name, kind)
    elif kind == "grad_b":
        assert sc.gradw_bf16_random_ok(got, p.ref), (name, kind)
    else:
        assert sc.transform_random_ok(got, p.ref, f32_out=False), (name, kind)
