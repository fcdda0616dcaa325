"""The persistent resident-weights bf16 transform (dense.hip: gemm_bf16_res_kernel) past a workgroup's FIRST row block.  GPU box
only (-m gpu).

A workgroup stages the weights once and walks row blocks blk, blk + stride, ...; from its second block on the tail phases of one
block fetch the head of the next, the epilogue's stores share the vmcnt counter with those loads, the bit-gated epilogue waits for
gate words issued a phase ahead, and the reduction starts at chunk blk % NC -- so the ragged last chunk and the boundary between two
operands sit at another phase in every block.  At the shipped grid (256 or 512 workgroups) that state needs hundreds of thousands of
rows; dgll_hip_debug_tune(16, 16) caps the grid at 16 workgroups and brings it to 3.5 blocks per row sequence at <= 28 237 rows, which
is what every case below runs (M is taken from dgll_hip_debug_transform_choice, not from a constant).  tests/dense_cases.py lists the
cases: every reachable (family, NC, epilogue) instantiation and the four dual ones, checked at the end.  Five cases run the real grid
as well, so the knob is not what makes the sweep pass.

Per case, through the public wrappers of dgll_amd/dense.py: (a) integer operands, where every product and partial sum is exact in
fp32 -- the output must EQUAL the float64 host result (rounded to bf16 for a bf16 output); (b) random operands against the float64
product of the bf16-rounded operands, at the bars of test_mfma_transform_kernel (fp32 output rtol 1e-4 / atol 1e-3, bf16 output rtol
1e-2 / atol 2e-2); (c) the capped launch, a second capped launch and the uncapped one (every block some workgroup's first) are bit
equal -- a block's summation order depends on blk % NC alone; (d) the activations sit on a wider pitch with NaN behind column K, and
through the C entry points the output goes into a sentinel-filled buffer with spare rows and a wider pitch; (e) the sign bits that
come with a bf16 output are those of what was stored."""
import contextlib

import numpy as np
import pytest
import torch

from dense_cases import (CASES, GRID_CAP, MAX_ROWS, REACHABLE, REAL_GRID_CASES, case_choice_args, case_instantiation, choice,
                         instantiation)

pytestmark = pytest.mark.gpu

SENTINEL = 30720.0            # exact in bf16 and fp32, far outside every result here
HIT = set()                   # instantiations the cases that ran were shown to reach


@contextlib.contextmanager
def grid_cap(value):
    from dgll_amd import _lib

    _lib.check(_lib.lib.dgll_hip_debug_tune(16, value), "dgll_hip_debug_tune")
    try:
        yield
    finally:
        _lib.check(_lib.lib.dgll_hip_debug_tune(16, 0), "dgll_hip_debug_tune")


def n_cu_of(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def nan_padded(x, device):
    """bf16 device copy of x [M, K] on a pitch of whole 64-chunks + 8 with NaN behind column K: inside the last 8-element vector, in
    the rest of the last chunk and behind it."""
    m, k = x.shape
    store = torch.full((m, -(-k // 64) * 64 + 8), float("nan"), dtype=torch.bfloat16, device=device)
    view = store[:, :k]
    view.copy_(x)
    return view


def padded(x, device, dtype=torch.bfloat16):
    from dgll_amd import ops

    out = ops.alloc_features(x.shape[0], x.shape[1], dtype, device)
    out.copy_(x)
    return out


def pack_bits(positive):
    """bool [M, N] -> int32 [M, bit_words(N)]: bit b of word w = column 32 w + b."""
    from dgll_amd import dense

    m, n = positive.shape
    full = np.zeros((m, dense.bit_words(n) * 32), dtype=np.uint8)
    full[:, :n] = positive
    return torch.from_numpy(np.packbits(full, axis=1, bitorder="little").view(np.int32).copy())


def make_data(case, m, exact, seed):
    """Host operands of a case (bf16-representable, float32 / float64 tensors) and the float64 reference.  exact: operands and weights
    from {-1, 0, 1}, small integer bias, integer addend in [-4, 4], row scale from {0.5, 1}: every value along the way is an integer
    or a half, exact in fp32.  Otherwise randn operands and the asymmetric weights of test_mfma_transform_kernel.  Rows are drawn
    independently, so a block delivered to the wrong rows cannot pass."""
    g = torch.Generator().manual_seed(seed)
    d = {}

    def operand(k):
        if exact:
            return torch.randint(-1, 2, (m, k), generator=g).float()
        return torch.randn(m, k, generator=g).to(torch.bfloat16).float()

    def weight(k):                                  # stored [N, K]
        if exact:
            return torch.randint(-1, 2, (case.N, k), generator=g).float()
        return (torch.randn(case.N, k, generator=g) * 0.1 + torch.arange(case.N).float()[:, None] * 1e-3).to(torch.bfloat16).float()

    d["a1"], d["w1"] = operand(case.K1), weight(case.K1)
    if case.dual:
        d["w2"] = weight(case.K1)
        d["ref"] = (d["a1"].double() @ d["w1"].double().t(), d["a1"].double() @ d["w2"].double().t())
        return d
    z = d["a1"].double() @ d["w1"].double().t()
    if case.K2:
        d["a2"], d["w2"] = operand(case.K2), weight(case.K2)
        z += d["a2"].double() @ d["w2"].double().t()
    if case.row_scale:
        d["row_scale"] = torch.randint(1, 3, (m,), generator=g).float() * 0.5 if exact else torch.rand(m, generator=g) + 0.5
        z *= d["row_scale"].double()[:, None]
    if case.bias:
        d["bias"] = torch.randint(-3, 4, (case.N,), generator=g).float() if exact else torch.randn(case.N, generator=g)
        z += d["bias"].double()
    if case.addend:
        d["addend"] = (torch.randint(-4, 5, (m, case.N), generator=g).float() if exact
                       else torch.randn(m, case.N, generator=g).to(torch.bfloat16).float())
        z += d["addend"].double()
    if case.relu:
        z.clamp_(min=0)
    if case.gate or case.gate_bits:
        d["gate"] = torch.randint(-1, 2, (m, case.N), generator=g).float()       # random signs, zeros among them
        z *= (d["gate"] > 0)
    d["ref"] = z
    return d


def to_device(case, d, device):
    """The device tensors of a case in the layouts the wrapper takes."""
    t = {"a1": nan_padded(d["a1"], device), "w1": d["w1"].to(device).to(torch.bfloat16)}
    if "a2" in d:
        t["a2"] = nan_padded(d["a2"], device)
    if "w2" in d:
        t["w2"] = d["w2"].to(device).to(torch.bfloat16)
    if "a2" in d and -(-case.K1 // 64) != -(-case.K2 // 64):
        # The wrapper packs each weight matrix on a pitch of its own whole chunks, and weights of two pitches go to the 4-wave kernel.
        # Zero columns behind the narrower matrix put both on one pitch; K1 / K2 are still the activations' widths.
        wide = 64 * max(-(-case.K1 // 64), -(-case.K2 // 64))
        for key in ("w1", "w2"):
            w = torch.zeros((case.N, wide), dtype=torch.bfloat16, device=device)
            w[:, :t[key].shape[1]] = t[key]
            t[key] = w
    if "row_scale" in d:
        t["row_scale"] = d["row_scale"].to(device)
    if "bias" in d:
        t["bias"] = d["bias"].to(device)
    if "addend" in d:
        t["addend"] = padded(d["addend"], device) if case.addend_padded else d["addend"].to(device).to(torch.bfloat16).contiguous()
    if "gate" in d:
        if case.gate:
            t["gate"] = padded(d["gate"], device)
        if case.gate_bits:
            t["gate_bits"] = pack_bits((d["gate"] > 0).numpy()).to(device)
    return t


def run_wrapper(case, t, m, device):
    """One launch through dgll_amd.dense: (outputs, sign bits or None)."""
    from dgll_amd import dense

    if case.dual:
        return dense.transform_bf16_dual(t["a1"], t["w1"], t["w2"]), None
    dtype = torch.float32 if case.f32 else torch.bfloat16
    out = None
    if case.unaligned:                              # rows on a pitch that is no multiple of 8 elements
        ld = case.N + 3 if (case.N + 3) % 8 else case.N + 5
        out = torch.empty((m, ld), dtype=dtype, device=device)[:, :case.N]
    res = dense.transform_bf16(t["a1"], t["w1"], t.get("a2"), t.get("w2"), relu=case.relu, out_dtype=dtype, bias=t.get("bias"),
                               out_gate=t.get("gate"), row_scale=t.get("row_scale"), addend=t.get("addend"), out=out,
                               gate_bits=t.get("gate_bits"), bits_out=case.bits_out)
    return ((res[0],), res[1]) if case.bits_out else ((res,), None)


def check_sign_bits(case, out, bits):
    """(e) every word is the sign bits of what was stored; zeros past N and in the padding words."""
    from dgll_amd import dense

    assert bits.shape == (out.shape[0], dense.bit_words(case.N)) and bits.dtype == torch.int32
    assert torch.equal(bits.cpu(), pack_bits((out.float() > 0).cpu().numpy())), case.name


def run_c_padding(case, t, m, device, expect):
    """(d) the same launch through the C entry point into a sentinel-filled buffer with 5 spare rows and a wider pitch: rows >= M
    and columns >= N keep the sentinel; with relu bit 1 (the caller owns the row padding) the columns [N, ldo) of rows < M are
    zeros.  The pitch stays inside the columns the family's workgroups produce."""
    from dgll_amd import _lib, dense

    n = case.N
    width = 256 if case.dual else 64 if n <= 64 else 128 if n <= 128 else 256
    ldo = min(-(-n // 8) * 8 + 8, width)
    p1 = dense._pad_wt(t["w1"], rows=256 if case.dual else None)
    for own_padding in ((False,) if case.dual else (False, True)):
        bufs = [torch.full((m + 5, ldo), SENTINEL, dtype=torch.bfloat16, device=device) for _ in range(2 if case.dual else 1)]
        if case.dual:
            p2 = dense._pad_wt(t["w2"], rows=256)
            _lib.launch("dgll_hip_transform_bf16_dual", device, t["a1"].data_ptr(), t["a1"].stride(0), case.K1, p1.data_ptr(), p2.data_ptr(),
                        p1.stride(0), p1.shape[0], bufs[0].data_ptr(), ldo, bufs[1].data_ptr(), ldo, m, n)
        else:
            p2 = dense._pad_wt(t["w2"]) if "a2" in t else None
            a2 = t.get("a2")
            operands = (t["a1"].data_ptr(), t["a1"].stride(0), case.K1, p1.data_ptr(), p1.stride(0), _lib.ptr(a2), _lib.pitch(a2), case.K2,
                        _lib.ptr(p2), _lib.pitch(p2), p1.shape[0])
            flags = int(case.relu) | (2 if own_padding else 0)
            gate, gbits = t.get("gate"), t.get("gate_bits")
            if case.epi == 0:
                _lib.launch("dgll_hip_transform_bf16_add", device, *operands, None, 0, bufs[0].data_ptr(), ldo, _lib.BF16, m, n, flags,
                            _lib.ptr(t.get("bias")), _lib.ptr(gate), _lib.pitch(gate), _lib.ptr(t.get("row_scale")),
                            _lib.ptr(t.get("addend")), _lib.pitch(t.get("addend")))
            else:
                _lib.launch("dgll_hip_transform_bf16_bits", device, *operands, bufs[0].data_ptr(), ldo, m, n, flags, _lib.ptr(t.get("bias")),
                            _lib.ptr(gate), _lib.pitch(gate), _lib.ptr(gbits), _lib.pitch(gbits), None, 0)
        for buf, want in zip(bufs, expect):
            assert torch.equal(buf[:m, :n], want), (case.name, own_padding)
            assert (buf[m:] == SENTINEL).all(), (case.name, own_padding, "rows past M")
            if ldo > n:
                pad = buf[:m, n:]
                assert (pad == 0).all() if own_padding else (pad == SENTINEL).all(), (case.name, own_padding, "columns past N")


def compare(case, outs, refs, exact):
    for out, ref in zip(outs, refs):
        assert out.shape == ref.shape and out.dtype == (torch.float32 if case.f32 else torch.bfloat16)
        got = out.cpu()
        if exact:
            assert torch.equal(got.double(), ref if case.f32 else ref.to(torch.bfloat16).double()), case.name
        elif case.f32:
            np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-4, atol=1e-3, err_msg=case.name)
        else:
            np.testing.assert_allclose(got.float().numpy(), ref.numpy(), rtol=1e-2, atol=2e-2, err_msg=case.name)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_steady_state(cuda_device, case):
    dev = cuda_device
    want = case_instantiation(case)
    with grid_cap(GRID_CAP):
        c1 = choice(n_cu=n_cu_of(dev), **case_choice_args(case))
        m = (c1.row_sequences * 7 // 2 - 1) * c1.rows_per_block + 77
        c = choice(M=m, n_cu=n_cu_of(dev), **case_choice_args(case))
        # what the launches below run: the instantiation the case is meant for, in its steady state, unevenly loaded
        assert c.kernel == 1 and instantiation(c) == want, (case.name, instantiation(c))
        assert m <= MAX_ROWS and c.workgroups == GRID_CAP
        assert c.n_blocks >= 3 * c.row_sequences and c.n_blocks % c.row_sequences != 0
        # (a) exact arithmetic
        d = make_data(case, m, True, 1000 + len(case.name) + case.N + case.K1)
        t = to_device(case, d, dev)
        refs = d["ref"] if case.dual else (d["ref"],)
        if "a2" in t:                               # what the choice above was told: one pitch for both weight matrices
            from dgll_amd import dense

            assert dense._pad_wt(t["w1"]).stride(0) == dense._pad_wt(t["w2"]).stride(0)
        outs, bits = run_wrapper(case, t, m, dev)
        compare(case, outs, refs, True)
        if bits is not None:
            check_sign_bits(case, outs[0], bits)
        if case.pad_check:
            run_c_padding(case, t, m, dev, outs)
        # (b) random values against float64
        d = make_data(case, m, False, 2000 + len(case.name) + case.N + case.K1)
        t = to_device(case, d, dev)
        refs = d["ref"] if case.dual else (d["ref"],)
        outs, bits = run_wrapper(case, t, m, dev)
        compare(case, outs, refs, False)
        if bits is not None:
            check_sign_bits(case, outs[0], bits)
        # (c) steady state == first block, bit for bit
        again, bits_again = run_wrapper(case, t, m, dev)
    assert instantiation(choice(M=m, n_cu=n_cu_of(dev), **case_choice_args(case))) == want        # the cap is off: the same kernel,
    assert choice(M=m, n_cu=n_cu_of(dev), **case_choice_args(case)).row_sequences >= c.n_blocks   # every block a workgroup's first
    first, bits_first = run_wrapper(case, t, m, dev)
    for o, o2, o1 in zip(outs, again, first):
        assert torch.equal(o, o2), (case.name, "two capped launches differ")
        assert torch.equal(o, o1), (case.name, "capped and uncapped launches differ")
    if bits is not None:
        assert torch.equal(bits, bits_again) and torch.equal(bits, bits_first), case.name
    HIT.add(want)


@pytest.mark.parametrize("case", REAL_GRID_CASES, ids=[c.name for c in REAL_GRID_CASES])
def test_real_grid(cuda_device, case):
    """Key 16 = 0: the shipped grid with 2.5 row blocks per row sequence -- check (a) on the first and last 1 024 rows and 20 000
    random ones, and a float64 column-sum checksum over all rows (integers: exact)."""
    from dgll_amd import dense

    dev = cuda_device
    c1 = choice(n_cu=n_cu_of(dev), **case_choice_args(case))
    m = c1.row_sequences * 5 // 2 * c1.rows_per_block + 77
    c = choice(M=m, n_cu=n_cu_of(dev), **case_choice_args(case))
    assert c.kernel == 1 and instantiation(c) == case_instantiation(case)
    assert c.n_blocks > 2 * c.row_sequences and c.n_blocks % c.row_sequences != 0
    g = torch.Generator(device=dev).manual_seed(m)
    store = torch.full((m, case.K1 + 8), float("nan"), dtype=torch.bfloat16, device=dev)
    x = store[:, :case.K1]
    x.copy_(torch.randint(-1, 2, (m, case.K1), device=dev, generator=g, dtype=torch.int8))
    ws = [torch.randint(-1, 2, (case.N, case.K1), device=dev, generator=g, dtype=torch.int8).to(torch.bfloat16) for _ in range(2 if case.dual else 1)]
    bias = torch.randint(-3, 4, (case.N,), device=dev, generator=g).float() if case.bias else None
    outs = dense.transform_bf16_dual(x, ws[0], ws[1]) if case.dual else (dense.transform_bf16(x, ws[0], bias=bias),)
    rows = torch.cat([torch.arange(1024), torch.arange(m - 1024, m), torch.randint(0, m, (20000,), generator=torch.Generator().manual_seed(7))])
    xs = x[rows.to(dev)].cpu().double()
    xsum = x.double().sum(0).cpu()
    for out, w in zip(outs, ws):
        assert out.shape == (m, case.N) and out.dtype == torch.bfloat16
        wd = w.cpu().double()
        ref = xs @ wd.t() + (bias.cpu().double() if bias is not None else 0.0)
        assert torch.equal(out[rows.to(dev)].cpu().double(), ref.to(torch.bfloat16).double()), case.name
        # all rows: the entries are integers of magnitude <= 256 (|sums| of K + 3 terms stay far below it), exact in bf16 and in float64
        assert (out.float().abs() <= 256).all()
        want = xsum @ wd.t() + (bias.cpu().double() * m if bias is not None else 0.0)
        assert torch.equal(out.double().sum(0).cpu(), want), case.name


def test_every_reachable_instantiation_was_run():
    """A condition, not a measurement: the cases cover the reachable set of tests/dense_cases.py, and -- when the whole file ran --
    each of them was shown by the choice struct to reach its instantiation on this device."""
    assert {case_instantiation(case) for case in CASES} == REACHABLE
    if len(HIT) >= len({case_instantiation(case) for case in CASES}):
        assert HIT == REACHABLE
