"""What the bf16 MFMA transform's choice rule can reach, and the cases that walk it (csrc/transform_choice.hpp: transform_choose,
read through dgll_hip_debug_transform_choice).  Shared by tests/test_dense_choice_host.py (no GPU: the rule itself, and that every
case below names the instantiation it is meant to hit) and tests/test_dense_steady_gpu.py (the cases run on the device).

An instantiation of the resident-weights kernel is (ntw, nc, cs, colsplit, epi, dual): gemm_bf16_res_kernel<NTW, 2, NC, CS, COLSPLIT,
1, EPI, 8, DUAL>."""
import collections
import ctypes as C

# (ntw, cs, colsplit) -> (output widths of the family: ragged and full, chunk counts it takes)
FAMILIES = collections.OrderedDict([
    ((2, 1, 1), ((47, 64), range(1, 9))),        # N <= 64
    ((4, 1, 1), ((100, 128), range(1, 9))),      # N <= 128
    ((4, 2, 1), ((200, 256), range(1, 5))),      # N <= 256, K <= 256: two waves per row group, 256 rows per block
    ((4, 1, 2), ((250, 256), range(5, 9))),      # N <= 256, K <= 512: two workgroups (column shares) per row block
])
DUAL_FAMILY = (4, 2, 2)

REACHABLE = frozenset([(ntw, nc, cs, colsplit, epi, 0) for (ntw, cs, colsplit), (_, ncs) in FAMILIES.items() for nc in ncs for epi in (0, 1, 2)] +
                      [(4, nc, 2, 2, 1, 1) for nc in range(1, 5)])
assert len(REACHABLE) == 24 * 3 + 4

GRID_CAP = 16            # dgll_hip_debug_tune(16, GRID_CAP) of the steady-state cases: the smallest grid the kernel takes
MAX_ROWS = 28237         # 55 blocks of 512 rows + 77: the tallest steady-state case


def choice(N, K1, K2=0, mask=False, out_f32=False, row_scale=False, addend=False, out_gate=False, gate_bits=False, out_aligned=True,
           ldw_equal=True, dual=False, M=1, n_cu=256, check=True):
    """The dgll_transform_choice of this launch description under the current knobs; check=False: (return code, struct)."""
    from dgll_amd import _lib

    out = _lib.TransformChoice()
    rc = _lib.lib.dgll_hip_debug_transform_choice(N, K1, K2, int(mask), int(out_f32), int(row_scale), int(addend), int(out_gate),
                                                  int(gate_bits), int(out_aligned), int(ldw_equal), int(dual), M, n_cu, C.byref(out))
    if check:
        _lib.check(rc, "dgll_hip_debug_transform_choice")
        return out
    return rc, out


def instantiation(c):
    return (c.ntw, c.nc, c.cs, c.colsplit, c.epi, c.dual)


Case = collections.namedtuple("Case", "name N K1 K2 fam nc epi dual f32 row_scale addend gate gate_bits unaligned bias relu bits_out "
                                      "addend_padded pad_check")


def _case(name, N, K1, K2, fam, epi, dual=False, **kw):
    opts = dict(f32=False, row_scale=False, addend=False, gate=False, gate_bits=False, unaligned=False, bias=False, relu=False,
                bits_out=False, addend_padded=True, pad_check=False)
    opts.update(kw)
    nc = -(-K1 // 64) + (-(-K2 // 64) if K2 else 0)
    return Case(name=name, N=N, K1=K1, K2=K2, fam=fam, nc=nc, epi=epi, dual=dual, **opts)


def case_instantiation(case):
    ntw, cs, colsplit = case.fam
    return (ntw, case.nc, cs, colsplit, case.epi, int(case.dual))


def case_choice_args(case):
    """The keyword arguments of `choice` that describe the launch the public wrapper makes for this case."""
    if case.dual:
        return dict(N=case.N, K1=case.K1, dual=True)
    bits_form = not (case.f32 or case.row_scale or case.addend)
    return dict(N=case.N, K1=case.K1, K2=case.K2, out_f32=case.f32, row_scale=case.row_scale, addend=case.addend, out_gate=case.gate,
                gate_bits=case.gate_bits and bits_form, out_aligned=not case.unaligned)


# the epilogue inputs of a case by kind; EPI 0 "all": everything the general epilogue takes at once (gate_bits is handed over too and,
# with the bf16 gate there, dropped by the wrapper: the general epilogue reads the gate as bf16)
_EPI1 = (dict(), dict(bias=True, relu=True, bits_out=True))
_EPI2 = (dict(gate_bits=True, bias=True, relu=True, bits_out=True), dict(gate_bits=True))
_ALL_F32 = dict(f32=True, row_scale=True, addend=True, gate=True, gate_bits=True, unaligned=True, bias=True, relu=True)
_ALL_BF16 = dict(row_scale=True, addend=True, gate=True, bias=True, relu=True)
_ALONE = collections.OrderedDict([
    ("f32", dict(f32=True)),
    ("rowscale", dict(row_scale=True, bias=True)),
    ("addend", dict(addend=True, addend_padded=False, relu=True)),
    ("gate", dict(gate=True, bits_out=True)),                                  # (sign bits: sign_bits_kernel's pass afterwards)
    ("gatebits-unaligned", dict(gate=True, gate_bits=True, unaligned=True)),
])


def _build_cases():
    cases = []
    for fam, (widths, ncs) in FAMILIES.items():
        tag = "%d%d%d" % fam
        for nc in ncs:
            # a single operand whose last chunk is ragged and whose K is no multiple of 8; the family's ragged / full width by turns
            k, n = 64 * nc - 17, widths[(nc + 1) % 2]
            first = nc == ncs[0]
            cases.append(_case("f%s-nc%d-plain" % (tag, nc), n, k, 0, fam, 1, pad_check=first, **_EPI1[(nc // 2) % 2]))
            cases.append(_case("f%s-nc%d-bits" % (tag, nc), n, k, 0, fam, 2, pad_check=first, **_EPI2[(nc // 2) % 2]))
            cases.append(_case("f%s-nc%d-all" % (tag, nc), n, k, 0, fam, 0, **_ALL_F32))
        # whole chunks (nothing for res_trim to do), the other width, and the general epilogue's bf16 paths all together
        nc = {(2, 1, 1): 4, (4, 1, 1): 8, (4, 2, 1): 2, (4, 1, 2): 6}[fam]
        cases.append(_case("f%s-nc%d-whole-plain" % (tag, nc), widths[nc % 2], 64 * nc, 0, fam, 1, bias=True))
        cases.append(_case("f%s-nc%d-whole-all" % (tag, nc), widths[nc % 2], 64 * nc, 0, fam, 0, pad_check=True, **_ALL_BF16))
        # every input of the general epilogue alone
        nc = {(2, 1, 1): 2, (4, 1, 1): 3, (4, 2, 1): 4, (4, 1, 2): 5}[fam]
        for i, (what, opts) in enumerate(_ALONE.items()):
            cases.append(_case("f%s-nc%d-%s" % (tag, nc, what), widths[i % 2], 64 * nc - 17, 0, fam, 0, **opts))
    # two operands: the boundary between them (chunks0) meets the rotation at another phase in every block.  The first four are the
    # flagship step's own shapes.
    for k1, k2, n, fam in ((100, 100, 256, (4, 2, 1)), (47, 47, 256, (4, 2, 1)), (256, 256, 256, (4, 1, 2)), (256, 256, 47, (2, 1, 1)),
                           (40, 24, 33, (2, 1, 1)), (130, 60, 128, (4, 1, 1)), (64, 448, 256, (4, 1, 2)), (448, 64, 200, (4, 1, 2))):
        name = "pair-%d+%d-%d" % (k1, k2, n)
        cases.append(_case(name + "-plain", n, k1, k2, fam, 1, **_EPI1[1]))
        cases.append(_case(name + "-bits", n, k1, k2, fam, 2, **_EPI2[0]))
        cases.append(_case(name + "-addend", n, k1, k2, fam, 0, addend=True, relu=True))
    for k in (47, 100, 175, 256):
        for n in (47, 256):
            cases.append(_case("dual-%d-%d" % (k, n), n, k, 0, DUAL_FAMILY, 1, dual=True, pad_check=(k, n) == (47, 47)))
    return cases


CASES = _build_cases()

# the real grid (key 16 = 0): one case per family at the smallest reduction it allows
REAL_GRID_CASES = [
    _case("real-64-64", 64, 64, 0, (2, 1, 1), 1, bias=True),
    _case("real-64-128", 128, 64, 0, (4, 1, 1), 1, bias=True),
    _case("real-64-256", 256, 64, 0, (4, 2, 1), 1, bias=True),
    _case("real-320-256", 256, 320, 0, (4, 1, 2), 1, bias=True),
    _case("real-dual-64-256", 256, 64, 0, DUAL_FAMILY, 1, dual=True),
]


def steady_rows(case):
    """(M, dgll_transform_choice at M) of a steady-state case under the current knobs (the caller holds key 16 at GRID_CAP):
    3.5 row blocks per row sequence, 77 rows in the last one."""
    c = choice(**case_choice_args(case))
    n_blocks = c.row_sequences * 7 // 2
    m = (n_blocks - 1) * c.rows_per_block + 77
    return m, choice(M=m, **case_choice_args(case))
