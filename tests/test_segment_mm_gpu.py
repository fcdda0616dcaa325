"""The grouped matrix-core products (csrc/segment_mm.hip) through dgll_amd.ops_segmm against the float64 loop of tests/segmm_ref.py, at
the smallest shapes at which they can break.  GPU box only (-m gpu).

Two legs per case with the comparators of tests/dense_small_cases.py, as the dense sweeps: (a) integer operands in [-2, 2] -- every
partial sum in any order is exact in fp32, so forward, grad_a and grad_b must EQUAL the float64 result as stored; (b) bf16-rounded randn
operands at the project's bars for this instruction (transform_random_ok, gradw_bf16_random_ok, f32_random_ok with R the reduction
length), the largest |err| / (|A| |B|) printed.  The forward runs into a sentinel buffer with spare rows and a wider pitch, from an `a`
on a wider pitch with NaN behind column K; a second run must give the same bits, grad_b included."""
import pytest
import torch

import dense_small_cases as sc
from segmm_cases import DTYPES, EDGES, ONE, SHORT, SLAB, WG, check, operands, problems, run
from segmm_ref import grouped_refs, segment_ids

pytestmark = pytest.mark.gpu

CASES =[(EDGES, 8, 1), (EDGES, 40, 33), (EDGES, 320, 64), (WG, 64, 64), (WG, 72, 100), (WG, 20, 7), (ONE, 200, 256), (ONE, 320, 64),
         (SHORT, 20, 7), (SHORT, 64, 300), (SLAB, 72, 100), (SLAB, 200, 256)]
IDS = ["%dsegs-m%d-k%d-n%d" % (len(s), sum(s), k, n) for s, k, n in CASES]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("op", ["segment", "gather"])
@pytest.mark.parametrize("seglen, k, n", CASES, ids=IDS)
def test_grouped_products(cuda_device, seglen, k, n, op, dtype):
    extra = 3 if op == "gather" else 0                       # gather: types that never occur
    idx = segment_ids(seglen)
    if op == "gather":
        idx = idx[torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(7))] + 1      # type 0 never occurs either
    grouping = idx.to(cuda_device) if op == "gather" else torch.tensor(seglen, device=cuda_device)
    m = idx.numel()
    for exact in (True, False):
        a, b, g = operands(seglen, k, n, extra + (1 if op == "gather" else 0), exact, dtype == torch.bfloat16, 11 + exact)
        buf, ga, gb = run(op, a, b, g, grouping, dtype, cuda_device)
        name = "%s %s exact=%d" % (op, dtype, exact)
        for got, p, kind in zip((buf[:m, :n], ga, gb), problems(a, b, g, idx), ("forward", "grad_a", "grad_b")):
            check(name, got, p, exact, dtype, kind)
        assert sc.outside_untouched(buf, m, n), (name, "written outside [M, N]")
        again = run(op, a, b, g, grouping, dtype, cuda_device)
        assert all(torch.equal(x, y) for x, y in zip((buf, ga, gb), again)), (name, "two runs differ")
        if op == "gather":          # bit for bit segment_mm on the sorted rows, put back in order
            from dgll_amd import ops_segmm

            order = torch.sort(grouping, stable=True)[1]
            ad, bd = a.to(device=cuda_device, dtype=dtype), b.to(device=cuda_device, dtype=torch.float32)
            sorted_c = ops_segmm.segment_mm(ad[order], bd, torch.bincount(grouping, minlength=b.shape[0]))
            back = torch.empty_like(sorted_c)
            back[order] = sorted_c
            assert torch.equal(buf[:m, :n], back), (name, "gather_mm differs from segment_mm on the sorted rows")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("seglen", [[40, 0, 30], [40, 50, 70]], ids=["short", "long"])
def test_wrong_device_seglen_stays_inside(cuda_device, seglen, dtype):
    """A device seglen whose sum is not M = 100 cannot be checked without a read-back: segments are clamped to the rows there are, rows
    that no segment covers are zeros, covered rows are right, nothing outside c is written."""
    from dgll_amd import ops_segmm

    m, k, n = 100, 40, 33
    a, b, g = operands([m, 0, 0], k, n, 0, True, True, 5)
    idx = segment_ids(seglen)[:m]
    idx = torch.cat((idx, torch.full((m - idx.numel(),), -1)))                 # uncovered rows: no type
    ref = grouped_refs(a, b, g, idx)[0]
    buf = sc.sentinel_buffer(m + 3, n + 5, dtype, cuda_device)
    ad = sc.padded(a, cuda_device, dtype, sc.bf16_pitch(k), spare_rows=2)
    ops_segmm._product_raw(ad, b.to(device=cuda_device, dtype=dtype), torch.tensor(seglen, device=cuda_device), None, False, out=buf[:m, :n])
    assert sc.exact_ok(buf[:m, :n], ref, bf16_out=dtype == torch.bfloat16)
    assert sc.outside_untouched(buf, m, n)
    grad_b = ops_segmm._gradw_raw(ad, ops_segmm._rows16(g.to(device=cuda_device, dtype=dtype)), torch.tensor(seglen, device=cuda_device), None, 3)
    assert sc.exact_ok(grad_b, grouped_refs(a, b, g, idx)[2])


def test_gather_mm_makes_no_permuted_copy(cuda_device):
    """Peak memory of a gather_mm forward above its inputs stays under |c| + half an [M, K] array (16 + 8 MiB): the sort's
    permutation and ids and a bounded packed copy of the weights fit, a permuted copy of a (16 MiB) does not."""
    from dgll_amd import ops_segmm

    m, k, r = 1 << 15, 256, 64
    a = torch.randn(m, k, device=cuda_device).to(torch.bfloat16)
    b = torch.randn(r, k, k, device=cuda_device).to(torch.bfloat16)
    idx = torch.randint(0, r, (m,), device=cuda_device)
    ops_segmm.gather_mm(a[:64], b, idx_b=idx[:64])               # (first-use allocations of the runtime are not the operator's)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    c = ops_segmm.gather_mm(a, b, idx_b=idx)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("gather_mm forward, M = 2^15, K = N = 256, R = 64, bf16: peak above the inputs %.2f MiB" % (peak / 2 ** 20))
    assert c.shape == (m, k) and peak < (16 + 8) * 2 ** 20


def test_typed_linear_step_is_capturable(cuda_device):
    """Forward and backward of a TypedLinear with a device x_type (the sort included) in one torch.cuda.graph, replayed after x changes
    in place, match eager -- nothing on the path reads the device back."""
    from dgll.nn import TypedLinear

    torch.manual_seed(0)
    layer = TypedLinear(40, 33, 6).to(cuda_device)
    x = torch.randn(200, 40, device=cuda_device, requires_grad=True)
    t = torch.randint(0, 6, (200,), device=cuda_device)

    def step():
        layer.W.grad = x.grad = None
        y = layer(x, t)
        y.square().sum().backward()
        return y.detach(), x.grad, layer.W.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for seed in range(3):
        with torch.no_grad():
            x.copy_(torch.randn(200, 40, generator=torch.Generator().manual_seed(seed)).to(cuda_device))
        graph.replay()
        replayed = [v.clone() for v in captured]
        assert all(torch.equal(u, v) for u, v in zip(replayed, step())), seed


def test_typed_linear_basis_on_the_gpu(cuda_device):
    """regularizer="basis": W_r = coeff . W runs as dense.linear of [R, B] x [B, in * out] -- a reduction of num_bases = 3 (rows that are
    no 16-byte multiple), in * out = 1320 columns in 256-column launches, and the same shapes backwards.  Output and all three
    gradients against the layer's own host path in float64, at the fp32 bars of dense_small_cases.transform_random_ok."""
    from dgll.nn import TypedLinear

    torch.manual_seed(1)
    host = TypedLinear(40, 33, 6, regularizer="basis", num_bases=3).double()
    dev = TypedLinear(40, 33, 6, regularizer="basis", num_bases=3).to(cuda_device)
    dev.load_state_dict({k: v.float() for k, v in host.state_dict().items()})
    x = torch.randn(200, 40, dtype=torch.float64, requires_grad=True)
    t = torch.randint(0, 6, (200,))
    g = torch.randn(200, 33, dtype=torch.float64)
    xd = x.detach().float().to(cuda_device).requires_grad_(True)
    want = host(x, t)
    want.backward(g)
    got = dev(xd, t.to(cuda_device))
    got.backward(g.float().to(cuda_device))
    for name, u, v in (("out", got, want), ("grad_x", xd.grad, x.grad), ("grad_W", dev.W.grad, host.W.grad), ("grad_coeff", dev.coeff.grad, host.coeff.grad)):
        assert sc.transform_random_ok(u.detach(), v.detach(), f32_out=True), (name, float((u.detach().double().cpu() - v.detach()).abs().max()))
