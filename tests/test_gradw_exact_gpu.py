"""The bf16 split-K weight gradient (csrc/gradw.hip: gradw_splitk_kernel + gradw_reduce_kernel) at small shapes, where one dropped or
doubled row is an integer off.  GPU box only (-m gpu).

tests/dense_small_cases.py lists the cases: all 20 (K1, K2) operand splits (every kslabs pair, both workgroup-type counts, ks_total no
multiple of 4), widths that leave the upper half of G's columns idle and widths that do not, ragged last steps, odd and even 64-row step
counts, 1 2 3 4 5 6 and 9 used slabs and more slabs requested than used (tests/test_dense_small_host.py asserts all of that from the
entry point's arithmetic).  The C entry points are called with an explicit n_slabs -- the public wrapper makes no slab below 256 rows.

Per case: (a) integer operands, dW must EQUAL the float64 product; (b) randn operands at the bar of tests/test_gradw_gpu.py, the largest
|err| / (|X|^T @ |G|) recorded; (c) a second launch is bit-equal; (d) dgll_hip_grad_weight_bf16_tr stores the transposes, bit for bit;
(e) dW goes into a sentinel-filled [K + 3, N + 5] ([N + 3, K + 5] transposed) buffer and nothing outside [K, N] is touched; (f) the
operands sit on wider pitches with NaN behind the last valid column and in three rows past M, the workspace is NaN before every launch:
no NaN reaches a kept output."""
import pytest
import torch

import dense_small_cases as sc

pytestmark = pytest.mark.gpu

RATIO = {}                    # largest |err| / (|X|^T @ |G|) of the random legs, by what ran


def operands(problems, device):
    """bf16 device operands of a case's Problems: pitch a multiple of 8, wider than the width, NaN behind it and in three spare rows."""
    first = next(p for p in problems if p is not None)
    place = lambda t: sc.padded(t, device, torch.bfloat16, sc.round_up(t.shape[1], 8) + 8, spare_rows=3)      # noqa: E731
    return [None if p is None else place(p.inputs["x"]) for p in problems], place(first.inputs["g"])


def launch(entry, xs, g, m, ks, n, n_slabs, device):
    """One launch through the C entry point: sentinel-filled destinations of spare rows and columns, a workspace of exactly
    dgll_hip_grad_weight_workspace bytes poisoned with NaN.  Returns the destination buffers (None for a missing operand)."""
    from dgll_amd import _lib

    tr = entry.endswith("_tr")
    need = int(_lib.lib.dgll_hip_grad_weight_workspace(ks[0], ks[1], n_slabs))
    assert need % 4 == 0 and need > 0
    ws = torch.full((need // 4,), sc.NAN, dtype=torch.float32, device=device)
    bufs = [None if not k else sc.sentinel_buffer(*((n + 3, k + 5) if tr else (k + 3, n + 5)), torch.float32, device) for k in ks]
    x1, x2 = xs
    _lib.launch(entry, device, _lib.ptr(x1), _lib.pitch(x1), ks[0], _lib.ptr(x2), _lib.pitch(x2), ks[1], _lib.ptr(g), _lib.pitch(g), n, m,
                ws.data_ptr(), need, n_slabs, bufs[0].data_ptr(), bufs[0].stride(0), _lib.ptr(bufs[1]), _lib.pitch(bufs[1]))
    return bufs


@pytest.mark.parametrize("case", sc.GRADW_CASES, ids=[c.name for c in sc.GRADW_CASES])
def test_split_k_gradient(cuda_device, case):
    dev = cuda_device
    ks, n, m = (case.K1, case.K2), case.N, case.M
    for exact in (True, False):
        problems = sc.gradw_problems(case, exact)
        xs, g = operands(problems, dev)
        bufs = launch("dgll_hip_grad_weight_bf16", xs, g, m, ks, n, case.n_slabs, dev)
        again = launch("dgll_hip_grad_weight_bf16", xs, g, m, ks, n, case.n_slabs, dev)
        turned = launch("dgll_hip_grad_weight_bf16_tr", xs, g, m, ks, n, case.n_slabs, dev)
        for p, k, buf, buf2, buf_t in zip(problems, ks, bufs, again, turned):
            if p is None:
                assert buf is None
                continue
            got = buf[:k, :n]
            assert bool(torch.isfinite(got).all()), (case.name, exact, "NaN from the padding or the workspace")          # (f)
            if exact:
                assert sc.exactness_holds(p)
                assert sc.exact_ok(got, p.ref), (case.name, k, float((got.double().cpu() - p.ref).abs().max()))         # (a)
            else:
                ratio = sc.error_ratio(got, p.ref, p.bound)
                print("gradw_splitk %s K=%d: max |err| / (|X|^T |G|) = %.3e" % (case.name, k, ratio))
                RATIO["gradw_splitk"] = max(RATIO.get("gradw_splitk", 0.0), ratio)
                assert sc.gradw_bf16_random_ok(got, p.ref), (case.name, k, ratio)                                       # (b)
            assert sc.outside_untouched(buf, k, n), (case.name, exact, "written outside [K, N]")                        # (e)
            assert torch.equal(buf, buf2), (case.name, exact, "two launches differ")                                    # (c)
            assert torch.equal(buf_t[:n, :k], got.t()), (case.name, exact, "_tr is not the transpose")                  # (d)
            assert sc.outside_untouched(buf_t, n, k), (case.name, exact, "_tr wrote outside [N, K]")


@pytest.mark.parametrize("entry", ["dgll_hip_grad_weight_bf16", "dgll_hip_grad_weight_bf16_tr"])
@pytest.mark.parametrize("k1,k2,n", [(47, 0, 65), (130, 100, 2), (256, 250, 256)])
def test_empty_reduction(cuda_device, entry, k1, k2, n):
    """M = 0: zeros of exactly the valid width, the sentinel everywhere else; the operands may be NULL."""
    tr = entry.endswith("_tr")
    bufs = launch(entry, (None, None), None, 0, (k1, k2), n, 3, cuda_device)
    for k, buf in zip((k1, k2), bufs):
        if not k:
            assert buf is None
            continue
        rows, cols = (n, k) if tr else (k, n)
        assert bool((buf[:rows, :cols] == 0).all()) and sc.outside_untouched(buf, rows, cols)


def _ints(m, k, device, seed):
    """Integers in [-2, 2], float64 on the host."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, (m, k), generator=g).double()


def test_public_grad_weight_small_exact(cuda_device):
    """dense.grad_weight at k = 602, n = 300, m = 333: 256-column blocks of x paired two per launch against 256-column blocks of g --
    every block is a column slice with real data on both sides, which must not leak into it.  Integers: exact."""
    from dgll_amd import dense, ops

    dev = cuda_device
    m, k, n = 333, 602, 300
    x64, g64 = _ints(m, k, dev, 1), _ints(m, n, dev, 2)
    x = ops.alloc_features(m, k, torch.bfloat16, dev)
    g = ops.alloc_features(m, n, torch.bfloat16, dev)
    x.copy_(x64)
    g.copy_(g64)
    assert dense._mfma_ok(x, g)
    got = dense.grad_weight(x, g)
    assert got.shape == (k, n) and got.dtype == torch.float32
    assert torch.equal(got.double().cpu(), x64.t() @ g64)
    assert torch.equal(got, dense.grad_weight(x, g))


def test_public_grad_weight_pair_wide_small_exact(cuda_device):
    """dense.grad_weight_pair on the wide path (602-column operands of unequal widths, n = 200, m = 333), into sentinel-free caller
    destinations: exact, and equal to one operand after the other."""
    from dgll_amd import dense, ops

    dev = cuda_device
    m, n = 333, 200
    x1_64, x2_64, g64 = _ints(m, 602, dev, 3), _ints(m, 300, dev, 4), _ints(m, n, dev, 5)
    tensors = []
    for t in (x1_64, x2_64, g64):
        d = ops.alloc_features(m, t.shape[1], torch.bfloat16, dev)
        d.copy_(t)
        tensors.append(d)
    x1, x2, g = tensors
    o1 = torch.full((602, n), sc.NAN, device=dev)
    o2 = torch.full((300, n), sc.NAN, device=dev)
    d1, d2 = dense.grad_weight_pair(x1, x2, g, out1=o1, out2=o2)
    assert d1 is o1 and d2 is o2
    assert torch.equal(d1.double().cpu(), x1_64.t() @ g64) and torch.equal(d2.double().cpu(), x2_64.t() @ g64)
    assert torch.equal(d1, dense.grad_weight(x1, g)) and torch.equal(d2, dense.grad_weight(x2, g))


@pytest.mark.parametrize("m,k,n1,n2", [(333, 250, 47, 130), (65, 130, 2, 256)])
def test_public_grad_weight_shared_x_small_exact(cuda_device, m, k, n1, n2):
    """dense.grad_weight_shared_x (dgll_hip_grad_weight_bf16_tr with the roles swapped): both products exact at small M."""
    from dgll_amd import dense

    dev = cuda_device
    x64, g1_64, g2_64 = _ints(m, k, dev, 6), _ints(m, n1, dev, 7), _ints(m, n2, dev, 8)
    place = lambda t: sc.padded(t, dev, torch.bfloat16, sc.round_up(t.shape[1], 8) + 8)      # noqa: E731
    x, g1, g2 = place(x64), place(g1_64), place(g2_64)
    assert dense._gradw_ok(g1, g2, x)
    d1, d2 = dense.grad_weight_shared_x(x, g1, g2)
    assert d1.shape == (k, n1) and d2.shape == (k, n2)
    assert torch.equal(d1.double().cpu(), x64.t() @ g1_64) and torch.equal(d2.double().cpu(), x64.t() @ g2_64)


def test_report_error_ratio():
    """Not a check: prints what the random legs of this file measured (run with -s), for a later tightening of the bar."""
    print("RECORD gradw.hip random legs:", {k: "%.3e" % v for k, v in RATIO.items()})
