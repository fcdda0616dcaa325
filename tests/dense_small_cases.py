"""Small-shape sweeps of the dense matrix-core kernels that had none: the case tables, operand builders, float64 references and
comparators shared by tests/test_dense_small_host.py (no GPU: coverage of the tables, the exactness condition, and that the comparators
reject small errors) and the three device files tests/test_gradw_exact_gpu.py (csrc/gradw.hip: gradw_splitk_kernel +
gradw_reduce_kernel), tests/test_dense_f32_exact_gpu.py (csrc/gemm_f32.hip: mm_f32_mfma_kernel<NT, VEC>,
gradw_f32_mfma_kernel<KTL, NT, VEC>) and tests/test_dense_fourwave_gpu.py (csrc/dense.hip: gemm_bf16_nt_kernel<2 | 4 | 8>).
Imports with numpy and torch on the CPU alone.

Two legs per case.  EXACT: integer operands in [-2, 2] (exact in bf16), small integer bias / addend, gate signs from {-1, 0, 1}: every
product and every partial sum is an integer (or a half, with a row scale) below 2**24, exact in fp32 in ANY summation order, so the kernel
must EQUAL the float64 result (rounded to bf16, RNE, for a bf16 output).  RANDOM: randn operands; the fp32 kernels are held to the a-priori
bound of R + S + 2 rounded fp32 operations per term, (R + S + 3) * 2**-24 * (|A| @ |B| + |addend| + |bias|) per entry (R the reduction
length, S the slab count; v_mfma_f32_32x32x2_f32 is a plain fmaf chain), the bf16-MFMA kernels to the project's own bars (the internal
summation of v_mfma_f32_32x32x16_bf16 is not documented) with the largest |err| / (|A| @ |B|) recorded.

A reference is ref = finish(P @ Q) with P [rows, R], Q [R, columns] in float64 (a gradient: P = X^T, Q = G; a product: P = [A1 | A2],
Q = [W1 | W2]^T) and `finish` the epilogue -- the form `mutants` needs to drop or double one reduction row."""
import collections

import numpy as np
import torch

SENTINEL = 30720.0            # exact in bf16 and fp32, far outside every result here
U = 2.0 ** -24                # unit roundoff of fp32
NAN = float("nan")


def ceil_div(a, b):
    return -(-a // b)


def round_up(a, b):
    return ceil_div(a, b) * b


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------
def padded(x, device, dtype, pitch, spare_rows=0, col_offset=0, fill=NAN):
    """[M, K] view, at column col_offset, of a `fill`-filled [M + spare_rows, pitch] buffer of `dtype` on `device`, holding x: NaN behind
    the last valid column of every row (inside the last vector and behind it), in front of the first with an offset, and in the spare rows."""
    m, k = x.shape
    assert pitch >= col_offset + k
    store = torch.full((m + spare_rows, pitch), fill, dtype=dtype, device=device)
    view = store[:m, col_offset:col_offset + k]
    view.copy_(x)
    return view


def sentinel_buffer(rows, pitch, dtype, device):
    return torch.full((rows, pitch), SENTINEL, dtype=dtype, device=device)


def outside_untouched(buf, m, n):
    """Everything of a sentinel-filled buffer outside [m, n] still holds the sentinel."""
    return bool((buf[m:] == SENTINEL).all()) and bool((buf[:m, n:] == SENTINEL).all())


def f32_pitch(k, mode):
    """(pitch, column offset) of an fp32 operand of width k.  "vec": 16-byte aligned rows on a pitch that is a multiple of 4 (the float4
    loads).  "slice": a column slice at an odd offset (the pointer is not 16-byte aligned).  "pitch": a pitch that is no multiple of 4."""
    if mode == "vec":
        return round_up(k, 4) + 4, 0
    if mode == "slice":
        return round_up(k + 1, 4) + 4, 1
    assert mode == "pitch"
    return (k + 1 if (k + 1) % 4 else k + 2), 0


def bf16_pitch(k):
    """Whole 64-chunks + 8: 16-byte aligned rows with NaN inside the last 8-element vector, in the rest of the last chunk and behind it."""
    return round_up(k, 64) + 8


def bit_words(n):
    """Words per row of a sign-bit matrix over n columns (dense.bit_words): 32 columns per word, rows padded to whole 16-byte vectors."""
    return round_up(ceil_div(n, 32), 4)


def pack_bits(positive):
    """bool numpy [M, N] -> int32 tensor [M, bit_words(N)]: bit b of word w = column 32 w + b."""
    m, n = positive.shape
    full = np.zeros((m, bit_words(n) * 32), dtype=np.uint8)
    full[:, :n] = positive
    return torch.from_numpy(np.packbits(full, axis=1, bitorder="little").view(np.int32).copy())


# ---- operands and float64 references ----------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _draw(g, shape, exact, bf16, scale=1.0, lo=-2, hi=2):
    """Rows and columns drawn independently (every entry is its own draw), float64 holding values exact in the operand's format."""
    if exact:
        return torch.randint(lo, hi + 1, shape, generator=g).double()
    x = torch.randn(shape, generator=g) * scale
    return (x.to(torch.bfloat16) if bf16 else x).double()


Problem = collections.namedtuple("Problem", "inputs P Q finish ref bound R")


def make_gradient(m, ks, n, exact, seed, bf16):
    """dW_i = X_i^T . G for the operands X_i [m, ks[i]] (ks[i] = 0: none) against one G [m, n]: a list of Problems, one per operand."""
    g = _gen(seed)

    def rows(k):                      # no row of integers is all zeros: at one row and one column the reference would be, too
        t = _draw(g, (m, k), exact, bf16)
        if exact and m:
            t[t.abs().sum(1) == 0, 0] = 1.0
        return t

    grad = rows(n)
    out = []
    for k in ks:
        if not k:
            out.append(None)
            continue
        x = rows(k)
        ref = x.t() @ grad
        out.append(Problem(inputs=dict(x=x, g=grad), P=x.t().contiguous(), Q=grad, finish=lambda z: z, ref=ref,
                           bound=x.abs().t() @ grad.abs(), R=m))
    return out


def make_product(m, n, k1, k2, epi, exact, seed, bf16=False, mask=False, wscale=1.0):
    """gate(act(row_scale * (mask(A1) . W1^T + A2 . W2^T) + bias + addend)): epi names what the epilogue is given, among "bias", "relu",
    "addend", "gate", "row_scale".  The mask zeroes entries of A1 alone.  bound = row_scale * (|A| @ |W|^T) + |bias| + |addend|."""
    g = _gen(seed)
    d = dict(a1=_draw(g, (m, k1), exact, bf16), w1=_draw(g, (n, k1), exact, bf16, wscale))
    a1 = d["a1"]
    if mask:
        d["mask"] = torch.randint(-1, 2, (m, k1), generator=g).double()           # signs, zeros among them
        a1 = a1 * (d["mask"] > 0)
    P, Q = a1, d["w1"].t()
    if k2:
        d["a2"], d["w2"] = _draw(g, (m, k2), exact, bf16), _draw(g, (n, k2), exact, bf16, wscale)
        P, Q = torch.cat([P, d["a2"]], dim=1), torch.cat([Q, d["w2"].t()], dim=0)
    P, Q = P.contiguous(), Q.contiguous()
    if "row_scale" in epi:
        d["row_scale"] = (torch.randint(1, 3, (m,), generator=g).double() * 0.5 if exact
                          else (torch.rand(m, generator=g) + 0.5).double())
    if "bias" in epi:
        d["bias"] = _draw(g, (n,), exact, False, lo=-3, hi=3)
    if "addend" in epi:
        d["addend"] = _draw(g, (m, n), exact, bf16, lo=-4, hi=4)
    if "gate" in epi:
        d["gate"] = torch.randint(-1, 2, (m, n), generator=g).double()
    relu = "relu" in epi

    def finish(z, absolute=False):
        z = z.clone()
        if "row_scale" in d:
            z *= d["row_scale"][:, None]
        if "bias" in d:
            z += d["bias"].abs() if absolute else d["bias"]
        if "addend" in d:
            z += d["addend"].abs() if absolute else d["addend"]
        if absolute:
            return z
        if relu:
            z.clamp_(min=0)
        if "gate" in d:
            z *= (d["gate"] > 0)
        return z

    return Problem(inputs=d, P=P, Q=Q, finish=finish, ref=finish(P @ Q), bound=finish(P.abs() @ Q.abs(), absolute=True), R=k1 + k2)


def exactness_holds(problem):
    """The condition of the exact leg: max(sum |a| |b| + |addend| + |bias|) < 2**24, so no partial sum in any order leaves the integers (or
    halves) that fp32 holds exactly."""
    return float(problem.bound.max()) < 2.0 ** 24 if problem.bound.numel() else True


# ---- comparators: True = accepted ---------------------------------------------------------------------------------------------------------
def as_stored(z, bf16_out):
    """A float64 result as the kernel would store it: rounded to bf16 (RNE) or to fp32."""
    return z.to(torch.bfloat16 if bf16_out else torch.float32)


def exact_ok(got, ref, bf16_out=False):
    return got.shape == ref.shape and torch.equal(got.double().cpu(), as_stored(ref, bf16_out).double())


def f32_random_bar(bound, R, S):
    return (R + S + 3) * U * bound


def f32_random_ok(got, ref, bound, R, S):
    return got.shape == ref.shape and bool(((got.double().cpu() - ref).abs() <= f32_random_bar(bound, R, S)).all())


def gradw_bf16_random_ok(got, ref):
    """The bar of tests/test_gradw_gpu.py."""
    if got.shape != ref.shape:
        return False
    if not ref.numel():
        return True
    return float((got.double().cpu() - ref).abs().max()) <= 2e-3 * float(ref.abs().max()) + 1e-3


def transform_random_ok(got, ref, f32_out):
    """The bars of test_mfma_transform_kernel / tests/test_dense_steady_gpu.py."""
    rtol, atol = (1e-4, 1e-3) if f32_out else (1e-2, 2e-2)
    return got.shape == ref.shape and bool(((got.double().cpu() - ref).abs() <= atol + rtol * ref.abs()).all())


def error_ratio(got, ref, bound):
    """Largest |err| / bound over the entries with a bound > 0 (bound = |A| @ |B|, plus |addend| + |bias| where there are any)."""
    err = (got.double().cpu() - ref).abs()
    ok = bound > 0
    return float((err[ok] / bound[ok]).max()) if bool(ok.any()) else 0.0


# ---- small errors a comparator has to reject ----------------------------------------------------------------------------------------------
def mutants(problem, visible):
    """name -> a float64 result that is wrong in one small way, built from the reference arrays alone: one reduction row dropped, one counted
    twice, two output columns swapped, the output transposed inside one 32 x 32 tile.  visible=False: the reduction row is the first from
    the middle on whose outer product is not zero (in the exact leg ANY such row has to show); True: the row whose outer product has the
    largest entry (the max-norm bars of the bf16 random legs cannot see every row -- the one they must see is the largest).  The columns
    swapped are column 0 and the one that differs most from it.  A shape too small for a mutation (one column: nothing to swap or
    transpose) leaves it out."""
    P, Q = problem.P, problem.Q
    z = P @ Q
    out = {}
    weight = P.abs().amax(dim=0) * Q.abs().amax(dim=1) if P.numel() and Q.numel() else torch.zeros(0)
    if weight.numel() and float(weight.max()) > 0:
        if visible:
            r = int(weight.argmax())
        else:
            order = list(range(problem.R // 2, problem.R)) + list(range(problem.R // 2))
            r = next(i for i in order if float(weight[i]) > 0)
        outer = P[:, r:r + 1] @ Q[r:r + 1]
        out["row dropped"] = problem.finish(z - outer)
        out["row doubled"] = problem.finish(z + outer)
    ref = problem.ref
    rows, cols = ref.shape
    if cols >= 2:
        j = int((ref - ref[:, :1]).abs().amax(dim=0).argmax())
        if j:
            swapped = ref.clone()
            swapped[:, 0], swapped[:, j] = ref[:, j], ref[:, 0]
            out["columns swapped"] = swapped
    s = min(32, rows, cols)
    if s >= 2:
        turned = ref.clone()
        turned[:s, :s] = ref[:s, :s].t()
        out["tile transposed"] = turned
    return out


# ---- bf16 split-K weight gradient (gradw.hip) ---------------------------------------------------------------------------------------------
GradwCase = collections.namedtuple("GradwCase", "name K1 K2 N M n_slabs")

GRADW_K1 = (47, 128, 130, 256)
GRADW_K2 = (0, 2, 100, 192, 250)
GRADW_SPLITS = tuple((k1, k2) for k2 in GRADW_K2 for k1 in GRADW_K1)                  # all 20 operand splits
GRADW_N = (1, 2, 47, 64, 65, 128, 129, 130, 200, 255, 256)
GRADW_ROWS = ((1, 1), (64, 1), (65, 1), (128, 1), (129, 1), (200, 1), (327, 6), (573, 9), (653, 5), (700, 9),
              # the ten above use 1, 4, 6 and 9 slabs; these three add the 2, 3 and 5 of the reduce kernel's four-wave interleave
              (128, 2), (129, 3), (300, 5))
GRADW_USED_SLABS = frozenset((1, 2, 3, 4, 5, 6, 9))


def gradw_geometry(case):
    """What grad_weight_bf16_impl (gradw.hip) makes of a case, by its own arithmetic: a.kslabs, grid.y, a.rows_per_slab, `used`, and the
    64-row step counts of the slabs."""
    ks0, ks1 = ceil_div(case.K1, 64), ceil_div(case.K2, 64)
    rows_per_slab = max(64, round_up(ceil_div(case.M, case.n_slabs), 64))
    used = ceil_div(case.M, rows_per_slab)
    steps = [ceil_div(min(case.M, (s + 1) * rows_per_slab) - s * rows_per_slab, 64) for s in range(used)]
    return dict(kslabs=(ks0, ks1), types=ceil_div(ks0 + ks1, 4), rows_per_slab=rows_per_slab, used=used, steps=steps)


def _gradw_cases():
    cases = []
    for i in range(5 * len(GRADW_ROWS)):
        (k1, k2), n, (m, sl) = GRADW_SPLITS[i % 20], GRADW_N[i % 11], GRADW_ROWS[i % 13]
        cases.append(GradwCase("%d+%d-n%d-m%d-s%d" % (k1, k2, n, m, sl), k1, k2, n, m, sl))
    return cases


GRADW_CASES = _gradw_cases()

# ---- fp32 product (gemm_f32.hip: launch_mm_f32 dispatches nt = ceil(N / 32) in 1..8 and a.vec: DGLL_MM(T), lines 349-359) ------------------
MmCase = collections.namedtuple("MmCase", "name N K1 K2 M mode epi ldc_vec entry")

MM_INSTANTIATIONS = frozenset((nt, vec) for nt in range(1, 9) for vec in (False, True))
F32_N = tuple(n for t in range(1, 9) for n in (32 * t - 5, 32 * t))
MM_K = ((5, 0), (31, 0), (32, 0), (33, 0), (100, 0), (256, 0), (33, 7), (47, 47), (3, 260))
MM_M = (1, 255, 256, 257, 511)
MM_EPI = ((), ("bias",), ("relu",), ("addend",), ("gate",), ("bias", "relu", "addend", "gate"))
MM_MODES = ("vec", "slice", "pitch")
MM_WIDE_N = 300               # through dense.mm_nt: two launches


def mm_instantiation(case):
    return (ceil_div(min(case.N, 256), 32), case.mode == "vec")


def _mm_cases():
    cases = []
    for ni, n in enumerate(F32_N):
        for vm, mode in enumerate(MM_MODES):
            k1, k2 = MM_K[(ni + 4 * vm) % 9]
            m = MM_M[(ni + vm) % 5]
            epi = MM_EPI[(ni + 2 * vm) % 6]
            entry = "mm" if k2 == 0 and "gate" not in epi and ni % 2 == 0 else "mm2"      # dgll_hip_mm_f32 / dgll_hip_mm2_f32
            cases.append(MmCase("n%d-%s-%d+%d-m%d-%s" % (n, mode, k1, k2, m, "+".join(epi) or "plain"), n, k1, k2, m, mode, epi,
                                (ni + vm) % 2 == 0, entry))
    return cases


MM_CASES = _mm_cases()

# ---- fp32 weight gradient (gemm_f32.hip: dgll_hip_grad_weight_f32 dispatches ktl = K > 128 ? 8 : 4, nt = ceil(min(N, 256) / 32) and vec:
# DGLL_GW(T), lines 416-441) ------------------------------------------------------------------------------------------------------------------
Gw32Case = collections.namedtuple("Gw32Case", "name K N M slabs mode")

GW32_INSTANTIATIONS = frozenset((ktl, nt, vec) for ktl in (4, 8) for nt in range(1, 9) for vec in (False, True))
GW32_K = {4: (3, 31, 32, 33, 100, 128), 8: (129, 200, 256, 257, 300, 520)}
GW32_M = (1, 31, 32, 33, 64, 95, 257)
GW32_SLABS = (1, 2, 3, 5)


def gw32_instantiation(case):
    return (8 if case.K > 128 else 4, ceil_div(min(case.N, 256), 32), case.mode == "vec")


def gw32_used_slabs(case):
    """dgll_hip_grad_weight_f32's own arithmetic: the slab count that is launched and summed."""
    slabs = min(max(1, min(case.slabs, ceil_div(case.M, 32))), 65535)
    per = round_up(ceil_div(case.M, slabs), 32)
    return ceil_div(case.M, per)


def _gw32_cases():
    cases, i = [], 0
    for ktl in (4, 8):
        for ni, n in enumerate(F32_N):
            for vb, mode in enumerate(("vec", ("slice", "pitch")[ni % 2])):
                k = GW32_K[ktl][(ni + 3 * vb) % 6]
                m, slabs = GW32_M[i % 7], GW32_SLABS[i % 4]
                cases.append(Gw32Case("k%d-n%d-m%d-s%d-%s" % (k, n, m, slabs, mode), k, n, m, slabs, mode))
                i += 1
    return cases


GW32_CASES = _gw32_cases()

# ---- 4-wave bf16 transform (dense.hip: transform_bf16_impl launches gemm_bf16_nt_kernel<c.nt> for c.kernel == 0) ----------------------------
FwCase = collections.namedtuple("FwCase", "name route N K1 K2 M out epi bits_out")

FW_NT = (2, 4, 8)
FW_N = (33, 64, 100, 128, 200, 256)
FW_M = (1, 77, 128, 129, 300)
FW_OUT = ("bf16", "bf16-odd", "f32", "f32-odd")      # bf16 on an aligned pitch / on one that is no multiple of 8, fp32 with ldo % 4 == 0 / != 0
FW_EPI = ((), ("bias",), ("relu",), ("row_scale",), ("addend",), ("gate",), ("bias", "relu", "row_scale", "addend", "gate"))
# what sends a launch to the 4-wave kernel (transform_choice.hpp), and its reductions: K1 no multiple of 8, odd and even chunk counts
FW_ROUTES = collections.OrderedDict([
    ("mask", ((100, 0), (47, 0), (190, 0))),                 # an input mask
    ("mask-pair", ((47, 47), (100, 60), (130, 64))),         # ... with a second operand, which the mask must not touch
    ("long", ((640, 0), (570, 0))),                          # K1 + K2 > 512: 10 and 9 chunks
    ("long-pair", ((300, 300), (300, 250))),
    ("pitch", ((100, 40), (47, 130), (250, 100))),           # two weight pitches: unequal chunk counts under the wrapper's own packing
])


def fw_nt(case):
    return 2 if case.N <= 64 else 4 if case.N <= 128 else 8


def fw_ldo(case):
    """The output pitch of a case: wider than N in every form."""
    n = case.N
    if case.out == "bf16":
        return round_up(n, 8) + 8
    if case.out == "bf16-odd":
        return n + 3 if (n + 3) % 8 else n + 5
    if case.out == "f32":
        return round_up(n, 4) + 4
    return n + 1 if (n + 1) % 4 else n + 2


def fw_choice_args(case):
    """The keyword arguments of dense_cases.choice that describe the launch the public wrapper makes for this case."""
    return dict(N=case.N, K1=case.K1, K2=case.K2, mask=case.route.startswith("mask"), out_f32=case.out.startswith("f32"),
                row_scale="row_scale" in case.epi, addend="addend" in case.epi, out_gate="gate" in case.epi,
                out_aligned=fw_ldo(case) % 8 == 0,
                ldw_equal=not case.K2 or ceil_div(case.K1, 64) == ceil_div(case.K2, 64), M=case.M)


def _fw_cases():
    cases, i = [], 0
    for route, shapes in FW_ROUTES.items():
        for ni, n in enumerate(FW_N):
            for rep in range(2):
                k1, k2 = shapes[(ni + rep) % len(shapes)]
                out, epi = FW_OUT[i % 4], FW_EPI[i % 7]
                # the sign bits come with a bf16 output without mask / row_scale / addend (dense.transform_bf16)
                bits = out.startswith("bf16") and not route.startswith("mask") and "row_scale" not in epi and "addend" not in epi
                cases.append(FwCase("%s-n%d-%d+%d-m%d-%s-%s" % (route, n, k1, k2, FW_M[i % 5], out, "+".join(epi) or "plain"), route, n, k1, k2,
                                    FW_M[i % 5], out, epi, bits))
                i += 1
    return cases


FW_CASES = _fw_cases()


def seed_of(case, exact):
    return (1000 if exact else 2000) + sum(ord(c) for c in case.name)


# the Problems of a case, built the same way on the host and for the device
def gradw_problems(case, exact):
    """[dW1's, dW2's or None]"""
    return make_gradient(case.M, (case.K1, case.K2), case.N, exact, seed_of(case, exact), bf16=True)


def mm_problem(case, exact):
    return make_product(case.M, case.N, case.K1, case.K2, case.epi, exact, seed_of(case, exact))


def gw32_problem(case, exact):
    return make_gradient(case.M, (case.K,), case.N, exact, seed_of(case, exact), bf16=False)[0]


def fw_problem(case, exact):
    return make_product(case.M, case.N, case.K1, case.K2, case.epi, exact, seed_of(case, exact), bf16=True,
                        mask=case.route.startswith("mask"), wscale=0.1)


def np32(t):
    return t.numpy().astype(np.float32)
