"""The 4-wave bf16 transform (csrc/dense.hip: gemm_bf16_nt_kernel<2 | 4 | 8>) -- what the choice rule falls back to with an input mask,
with weight matrices of two pitches and past K1 + K2 = 512 -- at all three NT and through every form of its epilogue.  GPU box only
(-m gpu).

tests/dense_small_cases.py lists the cases (FW_CASES): per route into the kernel every width of {33, 64 | 100, 128 | 200, 256}, odd and even
chunk counts, K1 no multiple of 8 (mask_tail), M in {1, 77, 128, 129, 300}; bf16 outputs on an aligned pitch (the LDS-transposed epilogue's
16-byte stores) and on a pitch that is no multiple of 8 (its element stores), fp32 outputs with ldo % 4 == 0 and != 0; bias, relu,
row_scale, addend and out_gate alone and together; the sign_bits_kernel pass behind it.  Every case first asserts, through
dense_cases.choice, that its launch is kernel 0 at the intended NT.

Per case through dense.transform_bf16, the output a [M, N] view of a sentinel-filled buffer with spare rows and a wider pitch: (a) integer
operands -- the output must EQUAL the float64 result (rounded to bf16 for a bf16 output); (b) bf16-rounded randn operands at the bars of
tests/test_dense_steady_gpu.py, the largest |err| / (|A| @ |W|^T) of the fp32 outputs recorded; (c) the activations and the mask sit on
wider pitches with NaN behind column K, gate and addend likewise; (d) nothing outside [M, N] is written; (e) the sign bits are those of
what was stored; (f) a second launch is bit-equal.  Cases with an aligned bf16 output also go through the C entry point with relu bit 1
(zeros in [N, ldo)) and without it (the sentinel kept)."""
import pytest
import torch

import dense_small_cases as sc
from dense_cases import choice

pytestmark = pytest.mark.gpu

RATIO = {}


def to_device(case, p, device):
    d = p.inputs
    bf = torch.bfloat16
    t = {"w1": d["w1"].to(device).to(bf)}
    for key in ("a1", "a2", "mask"):
        if key in d:
            t[key] = sc.padded(d[key], device, bf, sc.bf16_pitch(d[key].shape[1]), spare_rows=3)
    if "w2" in d:
        t["w2"] = d["w2"].to(device).to(bf)
    if "row_scale" in d:
        t["row_scale"] = d["row_scale"].float().to(device)
    if "bias" in d:
        t["bias"] = d["bias"].float().to(device)
    if "addend" in d:                                  # any pitch >= N: an odd one
        t["addend"] = sc.padded(d["addend"], device, bf, case.N + 3)
    if "gate" in d:                                    # 16-byte aligned rows
        t["gate"] = sc.padded(d["gate"], device, bf, sc.round_up(case.N, 8) + 8)
    return t


def check_sign_bits(n, out, bits):
    """Every word is the sign bits of what was stored; zeros past N and in the padding words."""
    from dgll_amd import dense

    assert dense.bit_words(n) == sc.bit_words(n)
    assert bits.shape == (out.shape[0], sc.bit_words(n)) and bits.dtype == torch.int32
    assert torch.equal(bits.cpu(), sc.pack_bits((out.float() > 0).cpu().numpy()))


def run(case, t, device):
    """One launch through the public wrapper into a sentinel-filled [M + 3, ldo] buffer: (buffer, output view, sign bits or None)."""
    from dgll_amd import dense

    f32 = case.out.startswith("f32")
    dtype = torch.float32 if f32 else torch.bfloat16
    buf = sc.sentinel_buffer(case.M + 3, sc.fw_ldo(case), dtype, device)
    out = buf[:case.M, :case.N]
    res = dense.transform_bf16(t["a1"], t["w1"], t.get("a2"), t.get("w2"), relu="relu" in case.epi, out_dtype=dtype, mask=t.get("mask"),
                               bias=t.get("bias"), out_gate=t.get("gate"), row_scale=t.get("row_scale"), addend=t.get("addend"), out=out,
                               bits_out=case.bits_out)
    got, bits = res if case.bits_out else (res, None)
    assert got.data_ptr() == out.data_ptr()
    return buf, out, bits


def run_c_padding(case, t, device, expect):
    """The same launch through the C entry point into a sentinel-filled buffer whose pitch stays inside the NT * 32 columns a workgroup
    produces: with relu bit 1 the columns [N, ldo) of rows < M are zeros, without it they keep the sentinel; rows >= M always do."""
    from dgll_amd import _lib, dense

    m, n = case.M, case.N
    ldo = min(sc.round_up(n, 8) + 8, sc.fw_nt(case) * 32)
    p1 = dense._pad_wt(t["w1"])
    p2 = dense._pad_wt(t["w2"]) if "w2" in t else None
    a2, mask, gate, addend = t.get("a2"), t.get("mask"), t.get("gate"), t.get("addend")
    for own_padding in (False, True):
        buf = sc.sentinel_buffer(m + 3, ldo, torch.bfloat16, device)
        _lib.launch("dgll_hip_transform_bf16_add", device, t["a1"].data_ptr(), t["a1"].stride(0), case.K1, p1.data_ptr(), p1.stride(0),
                    _lib.ptr(a2), _lib.pitch(a2), case.K2, _lib.ptr(p2), _lib.pitch(p2), p1.shape[0], _lib.ptr(mask), _lib.pitch(mask),
                    buf.data_ptr(), ldo, _lib.BF16, m, n, int("relu" in case.epi) | (2 if own_padding else 0), _lib.ptr(t.get("bias")),
                    _lib.ptr(gate), _lib.pitch(gate), _lib.ptr(t.get("row_scale")), _lib.ptr(addend), _lib.pitch(addend))
        assert torch.equal(buf[:m, :n], expect), (case.name, own_padding)
        assert bool((buf[m:] == sc.SENTINEL).all()), (case.name, own_padding, "rows past M")
        if ldo > n:
            pad = buf[:m, n:]
            assert bool(((pad == 0) if own_padding else (pad == sc.SENTINEL)).all()), (case.name, own_padding, "columns past N")


@pytest.mark.parametrize("case", sc.FW_CASES, ids=[c.name for c in sc.FW_CASES])
def test_four_wave_transform(cuda_device, case):
    from dgll_amd import dense

    dev = cuda_device
    f32 = case.out.startswith("f32")
    for exact in (True, False):
        p = sc.fw_problem(case, exact)
        t = to_device(case, p, dev)
        # what the launch below runs: the 4-wave kernel at the intended NT, by the pitches the wrapper's own packing gives the weights
        args = sc.fw_choice_args(case)
        if case.K2:
            assert args["ldw_equal"] == (dense._pad_wt(t["w1"]).stride(0) == dense._pad_wt(t["w2"]).stride(0))
        c = choice(n_cu=torch.cuda.get_device_properties(dev).multi_processor_count, **args)
        assert c.kernel == 0 and c.nt == sc.fw_nt(case), (case.name, c.kernel, c.nt)
        buf, out, bits = run(case, t, dev)
        assert bool(torch.isfinite(out.float()).all()), (case.name, exact, "NaN from the padding")                                   # (c)
        if exact:
            assert sc.exactness_holds(p)
            assert sc.exact_ok(out, p.ref, not f32), (case.name, float((out.double().cpu() - p.ref).abs().max()))                 # (a)
        else:
            ratio = sc.error_ratio(out, p.ref, p.bound)
            key = "gemm_bf16_nt fp32 out" if f32 else "gemm_bf16_nt bf16 out"
            print("%s %s: max |err| / (|A| |W|^T) = %.3e" % (key, case.name, ratio))
            RATIO[key] = max(RATIO.get(key, 0.0), ratio)
            assert sc.transform_random_ok(out, p.ref, f32), (case.name, ratio)                                                     # (b)
        assert sc.outside_untouched(buf, case.M, case.N), (case.name, exact, "written outside [M, N]")                              # (d)
        if case.bits_out:
            check_sign_bits(case.N, out, bits)                                                                                     # (e)
        buf2, _, bits2 = run(case, t, dev)
        assert torch.equal(buf, buf2) and (bits is None or torch.equal(bits, bits2)), (case.name, exact, "two launches differ")    # (f)
        if case.out == "bf16":
            run_c_padding(case, t, dev, out)


def test_gate_bits_next_to_the_gate(cuda_device):
    """The 4-wave kernel reads the gate as bf16: gate_bits handed over with out_gate changes nothing, and the sign bits written behind it
    (sign_bits_kernel) are those of the gated output."""
    from dgll_amd import dense

    dev = cuda_device
    p = sc.make_product(129, 200, 300, 300, ("bias", "relu", "gate"), True, 5, bf16=True)
    d = p.inputs
    bf = torch.bfloat16
    a1, a2 = (sc.padded(d[k], dev, bf, sc.bf16_pitch(300)) for k in ("a1", "a2"))
    gate = sc.padded(d["gate"], dev, bf, 208)
    gbits = sc.pack_bits((d["gate"] > 0).numpy()).to(dev)
    assert choice(N=200, K1=300, K2=300, out_gate=True, gate_bits=True, M=129).kernel == 0
    out, bits = dense.transform_bf16(a1, d["w1"].to(dev).to(bf), a2, d["w2"].to(dev).to(bf), relu=True, bias=d["bias"].float().to(dev),
                                     out_gate=gate, gate_bits=gbits, bits_out=True)
    assert sc.exact_ok(out, p.ref, True)
    check_sign_bits(200, out, bits)


def test_report_error_ratio():
    """Not a check: prints what the random legs of this file measured (run with -s), for a later tightening of the bars."""
    print("RECORD gemm_bf16_nt_kernel random legs:", {k: "%.3e" % v for k, v in RATIO.items()})
