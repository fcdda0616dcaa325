"""The fp32 matrix-core kernels (csrc/gemm_f32.hip) at small shapes: all 16 mm_f32_mfma_kernel<NT, VEC> and all 32
gradw_f32_mfma_kernel<KTL, NT, VEC>, each at a ragged and at a full width.  GPU box only (-m gpu).

v_mfma_f32_32x32x2_f32 is an fp32 fmaf chain, so both legs of tests/dense_small_cases.py are sharp: (a) integer operands, the output must
EQUAL the float64 result; (b) randn operands inside (R + S + 3) * 2**-24 * (|A| @ |B| + |addend| + |bias|) per entry, the a-priori bound
of any order of rounded fp32 additions (R: K1 + K2 of a product, M of a gradient; S: the slabs summed).  Through the C entry points:
operands on wider pitches with NaN behind the last valid column and in spare rows -- float4 loads (16-byte aligned rows, pitch a multiple
of 4) and scalar loads (a column slice at an odd offset; a pitch that is no multiple of 4) --, outputs in sentinel-filled buffers with
spare rows on pitches with ldc % 4 == 0 and != 0 (float4 and scalar stores), a NaN-poisoned slab workspace, a bit-equal second launch.
tests/test_dense_small_host.py asserts that the case tables reach every instantiation."""
import pytest
import torch

import dense_small_cases as sc

pytestmark = pytest.mark.gpu


def place(t, mode, device, spare_rows=0):
    pitch, offset = sc.f32_pitch(t.shape[1], mode)
    return sc.padded(t, device, torch.float32, pitch, spare_rows, offset)


def check(got, p, exact, slabs, what):
    assert bool(torch.isfinite(got).all()), (what, "NaN from the padding or the workspace")
    if exact:
        assert sc.exactness_holds(p)
        assert sc.exact_ok(got, p.ref), (what, float((got.double().cpu() - p.ref).abs().max()))
    else:
        worst = float(((got.double().cpu() - p.ref).abs() / sc.f32_random_bar(p.bound, p.R, slabs).clamp(min=1e-300)).max())
        print("%s: max |err| / bar = %.3f" % (what, worst))
        assert sc.f32_random_ok(got, p.ref, p.bound, p.R, slabs), (what, worst)


def run_mm(case, p, device):
    """The case's launch through dgll_hip_mm_f32 / dgll_hip_mm2_f32 into a sentinel-filled [M + 3, ldc] buffer."""
    from dgll_amd import _lib

    d, m, n = p.inputs, case.M, case.N
    a1, w1 = place(d["a1"], case.mode, device, spare_rows=3), place(d["w1"], case.mode, device, spare_rows=3)
    a2 = place(d["a2"], case.mode, device, spare_rows=3) if case.K2 else None
    w2 = place(d["w2"], case.mode, device, spare_rows=3) if case.K2 else None
    bias = d["bias"].float().to(device) if "bias" in d else None
    # the epilogue's reads: addend through float4 where the output goes through scalar stores and the other way round; the gate opposite
    addend = place(d["addend"], "pitch" if case.ldc_vec else "vec", device) if "addend" in d else None
    gate = place(d["gate"], "vec" if case.ldc_vec else "pitch", device) if "gate" in d else None
    ldc = sc.f32_pitch(n, "vec" if case.ldc_vec else "pitch")[0]
    assert (ldc % 4 == 0) == case.ldc_vec and ldc > n
    out = sc.sentinel_buffer(m + 3, ldc, torch.float32, device)
    relu = int("relu" in case.epi)
    if case.entry == "mm":
        _lib.launch("dgll_hip_mm_f32", device, a1.data_ptr(), a1.stride(0), w1.data_ptr(), w1.stride(0), out.data_ptr(), ldc, m, n, case.K1,
                    _lib.ptr(bias), relu, _lib.ptr(addend), _lib.pitch(addend))
    else:
        _lib.launch("dgll_hip_mm2_f32", device, a1.data_ptr(), a1.stride(0), w1.data_ptr(), w1.stride(0), case.K1, _lib.ptr(a2), _lib.pitch(a2),
                    _lib.ptr(w2), _lib.pitch(w2), case.K2, out.data_ptr(), ldc, m, n, _lib.ptr(bias), relu, _lib.ptr(addend),
                    _lib.pitch(addend), _lib.ptr(gate), _lib.pitch(gate))
    return out


@pytest.mark.parametrize("case", sc.MM_CASES, ids=[c.name for c in sc.MM_CASES])
def test_mm_f32(cuda_device, case):
    for exact in (True, False):
        p = sc.mm_problem(case, exact)
        out = run_mm(case, p, cuda_device)
        check(out[:case.M, :case.N], p, exact, 0, "mm_f32 " + case.name)
        assert sc.outside_untouched(out, case.M, case.N), (case.name, exact, "written outside [M, N]")
        assert torch.equal(out, run_mm(case, p, cuda_device)), (case.name, exact, "two launches differ")


@pytest.mark.parametrize("m,k,mode,epi", [(257, 100, "vec", ("bias", "relu", "addend")), (255, 33, "slice", ()), (1, 31, "pitch", ("bias",))])
def test_mm_nt_wide_output(cuda_device, m, k, mode, epi):
    """N = 300 through dense.mm_nt: two launches (256 + 44 columns), the second on weight, bias, addend and output pointers moved by 256
    columns / rows."""
    from dgll_amd import dense

    dev = cuda_device
    for exact in (True, False):
        p = sc.make_product(m, sc.MM_WIDE_N, k, 0, epi, exact, 77 + m + exact)
        d = p.inputs
        got = dense.mm_nt(place(d["a1"], mode, dev), place(d["w1"], mode, dev), relu="relu" in epi,
                          bias=d["bias"].float().to(dev) if "bias" in d else None,
                          addend=place(d["addend"], "vec", dev) if "addend" in d else None)
        assert got.shape == (m, sc.MM_WIDE_N) and got.dtype == torch.float32
        check(got, p, exact, 0, "mm_nt n300 m%d" % m)


def test_mm2_nt_wide_output_gated(cuda_device):
    """N = 300 through dense.mm2_nt: both products in one accumulation, the gate read per 256-column launch."""
    from dgll_amd import dense

    dev = cuda_device
    for exact in (True, False):
        p = sc.make_product(257, sc.MM_WIDE_N, 47, 47, ("relu", "gate"), exact, 91 + exact)
        d = p.inputs
        got = dense.mm2_nt(place(d["a1"], "vec", dev), place(d["w1"], "vec", dev), place(d["a2"], "slice", dev), place(d["w2"], "vec", dev),
                           relu=True, gate=place(d["gate"], "vec", dev))
        check(got, p, exact, 0, "mm2_nt n300")


def run_gw32(case, p, device):
    from dgll_amd import _lib

    x, g = place(p.inputs["x"], case.mode, device, spare_rows=3), place(p.inputs["g"], case.mode, device, spare_rows=3)
    need = int(_lib.lib.dgll_hip_grad_weight_f32_workspace(case.K, case.N, case.slabs))
    ws = torch.full((need // 4,), sc.NAN, dtype=torch.float32, device=device)
    out = sc.sentinel_buffer(case.K + 3, case.N + 5, torch.float32, device)
    _lib.launch("dgll_hip_grad_weight_f32", device, x.data_ptr(), x.stride(0), g.data_ptr(), g.stride(0), out.data_ptr(), out.stride(0),
                case.M, case.K, case.N, ws.data_ptr(), need, case.slabs)
    return out


@pytest.mark.parametrize("case", sc.GW32_CASES, ids=[c.name for c in sc.GW32_CASES])
def test_grad_weight_f32(cuda_device, case):
    for exact in (True, False):
        p = sc.gw32_problem(case, exact)
        out = run_gw32(case, p, cuda_device)
        check(out[:case.K, :case.N], p, exact, sc.gw32_used_slabs(case), "gradw_f32 " + case.name)
        assert sc.outside_untouched(out, case.K, case.N), (case.name, exact, "written outside [K, N]")
        assert torch.equal(out, run_gw32(case, p, cuda_device)), (case.name, exact, "two launches differ")
