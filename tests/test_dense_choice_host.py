"""Which kernel a launch of the bf16 MFMA transform gets (transform_choice.hpp: transform_choose), read through
dgll_hip_debug_transform_choice -- no GPU.  The launch path (dense.hip: transform_bf16_impl, dgll_hip_transform_bf16_dual) calls
the same function, so what is pinned here is what runs: the boundaries of the rule as they are today, the set of resident-weights
instantiations it can reach (tests/dense_cases.py: 24 (family, NC) pairs x 3 epilogues + 4 dual), the diagnostic grid cap (key 16)
and the refusals."""
import contextlib
import ctypes as C
import itertools

import pytest

from dense_cases import (CASES, GRID_CAP, MAX_ROWS, REACHABLE, REAL_GRID_CASES, case_choice_args, case_instantiation, choice,
                         instantiation, steady_rows)

KS = (8, 47, 64, 65, 100, 128, 192, 256, 257, 320, 448, 512, 513, 640)
FOUR_WAVE, RESIDENT = 0, 1


@contextlib.contextmanager
def tuned(**keys):
    """dgll_hip_debug_tune(key, value) for the block (k4=.., k11=.., k16=..), zeros -- the shipped defaults -- restored in a finally."""
    from dgll_amd import _lib

    try:
        for k, v in keys.items():
            _lib.check(_lib.lib.dgll_hip_debug_tune(int(k[1:]), v), "dgll_hip_debug_tune")
        yield
    finally:
        for k in keys:
            _lib.check(_lib.lib.dgll_hip_debug_tune(int(k[1:]), 0), "dgll_hip_debug_tune")


def chunks(k):
    return -(-k // 64)


def model(N, K1, K2, mask=False, out_f32=False, row_scale=False, addend=False, out_gate=False, gate_bits=False, out_aligned=True,
          ldw_equal=True, four_wave=False):
    """The rule as DESIGN.md section 4.3 states it, written down a second time: (kernel, nt, ntw, nc, cs, colsplit, epi,
    rows_per_block, lds_bytes, per_cu, bits_in_epilogue), or "refused"."""
    nt32, nc = -(-N // 32), chunks(K1) + (chunks(K2) if K2 else 0)
    nt = 2 if N <= 64 else 4 if N <= 128 else 8
    simple = not (out_f32 or row_scale or addend)
    epi = 1 if simple and not out_gate and not gate_bits else 2 if simple and gate_bits and out_aligned else 0
    if nc > 8:
        fits = False
    elif nt32 > 4 and nc > 4:
        fits = True                                             # 256 columns x 512 k: two workgroups of 128 columns
    else:
        fits = nc * nt * 32 * 128 <= 128 * 1024                 # the 128 KiB weight budget
    res = fits and not mask and not four_wave and (not K2 or ldw_equal)
    if gate_bits and not out_gate and not (res and epi == 2):
        return "refused"
    if not res:
        return (FOUR_WAVE, nt, 0, 0, 0, 0, 0, 128, 2 * nt * 32 * 144, 0, 0)
    ntw, cs, colsplit = (2, 1, 1) if nt32 <= 2 else (4, 1, 1) if nt32 <= 4 else (4, 2, 1) if nc <= 4 else (4, 1, 2)
    lds = nc * ntw * cs * 32 * 128 + 8 * 32 * 80 + ntw * cs * 32 * 4
    return (RESIDENT, nt, ntw, nc, cs, colsplit, epi, 512 // cs, lds, 1 if lds > 80 * 1024 else 2, int(epi != 0))


def observed(c):
    return (c.kernel, c.nt, c.ntw, c.nc, c.cs, c.colsplit, c.epi, c.rows_per_block, c.lds_bytes, c.per_cu, c.bits_in_epilogue)


EPILOGUES = {1: dict(), 2: dict(gate_bits=True), 0: dict(out_f32=True)}


def test_rule_over_every_width_and_reduction():
    """N = 1 .. 256 x K1 x K2 under each epilogue kind: kernel, family, chunk count, epilogue, rows per block, LDS and workgroups per
    CU are the model's, and the grid follows from them."""
    reached = set()
    for kind, flags in EPILOGUES.items():
        for N, K1, K2 in itertools.product(range(1, 257), KS, (0,) + KS):
            want = model(N, K1, K2, **flags)
            rc, c = choice(N, K1, K2, M=100000, check=False, **flags)
            if want == "refused":
                assert rc == -1 and c.error == -1, (N, K1, K2, flags)
                continue
            assert rc == 0 and observed(c) == want, (N, K1, K2, flags, observed(c), want)
            if c.kernel == RESIDENT:
                assert c.epi == kind and c.dual == 0
                assert c.workgroups == 256 * c.per_cu and c.row_sequences == c.workgroups // c.colsplit
                assert c.n_blocks == -(-100000 // c.rows_per_block)
                reached.add(instantiation(c))
            else:
                assert c.workgroups == c.row_sequences == c.n_blocks == -(-100000 // 128)
    assert reached == {i for i in REACHABLE if not i[5]}


def test_reachable_set_is_72_plus_4_dual():
    reached = set()
    for flags in (dict(zip(("out_f32", "row_scale", "addend", "out_gate", "gate_bits", "out_aligned"), bits))
                  for bits in itertools.product((False, True), repeat=6)):
        for N, K1, K2 in itertools.product((1, 32, 33, 64, 65, 96, 97, 128, 129, 160, 255, 256), KS, (0,) + KS):
            want = model(N, K1, K2, **flags)
            rc, c = choice(N, K1, K2, check=False, **flags)
            if want == "refused":
                assert rc == -1
                continue
            assert rc == 0 and observed(c) == want, (N, K1, K2, flags)
            if c.kernel == RESIDENT:
                reached.add(instantiation(c))
    for N, K in itertools.product((1, 47, 64, 65, 128, 129, 256), (1, 8, 47, 64, 65, 100, 128, 129, 175, 192, 193, 256)):
        c = choice(N, K, dual=True)
        assert (c.kernel, c.nt, c.ntw, c.nc, c.cs, c.colsplit, c.epi, c.dual) == (RESIDENT, 8, 4, chunks(K), 2, 2, 1, 1)
        assert c.rows_per_block == 256 and c.bits_in_epilogue == 1
        assert c.lds_bytes == chunks(K) * 8 * 32 * 128 + 8 * 32 * 80 + 8 * 32 * 4 and c.per_cu == (1 if c.lds_bytes > 80 * 1024 else 2)
        assert c.workgroups == 256 * c.per_cu and c.row_sequences == c.workgroups // 2
        reached.add(instantiation(c))
    assert reached == REACHABLE and len(reached) == 72 + 4


def test_boundaries_of_res_applies_and_the_families():
    # eight chunks at the most, whichever way they are split over the operands
    assert choice(64, 512).kernel == RESIDENT and choice(64, 513).kernel == FOUR_WAVE
    assert choice(64, 256, 256).kernel == RESIDENT and choice(64, 257, 256).kernel == FOUR_WAVE and choice(64, 448, 65).kernel == FOUR_WAVE
    # the 128 KiB weight budget: 8 chunks x 128 columns fit exactly; 256 columns fit with 4 chunks, beyond that the columns are split
    assert instantiation(choice(128, 512)) == (4, 8, 1, 1, 1, 0)
    assert instantiation(choice(129, 256)) == (4, 4, 2, 1, 1, 0)
    assert instantiation(choice(129, 257)) == (4, 5, 1, 2, 1, 0)
    assert instantiation(choice(256, 512)) == (4, 8, 1, 2, 1, 0)
    # the widths
    assert [choice(n, 64).ntw for n in (1, 64, 65, 128, 129, 256)] == [2, 2, 4, 4, 4, 4]
    assert [choice(n, 64).cs for n in (64, 128, 129, 256)] == [1, 1, 2, 2]
    assert [choice(n, 64).rows_per_block for n in (64, 128, 129, 256)] == [512, 512, 256, 256]
    assert choice(256, 320).rows_per_block == 512


def test_four_wave_kernel_keeps_the_mask_two_pitches_and_key_4():
    for N, nt in ((1, 2), (64, 2), (65, 4), (128, 4), (129, 8), (256, 8)):
        for c in (choice(N, 128, mask=True), choice(N, 128, 128, ldw_equal=False), choice(N, 640)):
            assert (c.kernel, c.nt, c.rows_per_block, c.lds_bytes) == (FOUR_WAVE, nt, 128, 2 * nt * 32 * 144)
            assert c.bits_in_epilogue == 0
        assert choice(N, 128, ldw_equal=False).kernel == RESIDENT          # one operand pair: there is no second pitch
        with tuned(k4=1):
            assert choice(N, 128).kernel == FOUR_WAVE and choice(N, 128).nt == nt
        with tuned(k4=2):                                                 # no chunk rotation: the choice is the shipped one
            assert choice(N, 128).kernel == RESIDENT
    assert choice(64, 128).kernel == RESIDENT


def test_epilogue_kind():
    kind = lambda **kw: choice(256, 256, **kw).epi       # noqa: E731
    assert kind() == 1
    assert kind(gate_bits=True) == 2 and kind(gate_bits=True, out_gate=True) == 2
    assert kind(out_gate=True) == 0
    # gate bits on an output the bit epilogue cannot store to as whole vectors: the general epilogue, which reads the bf16 gate
    assert kind(gate_bits=True, out_gate=True, out_aligned=False) == 0
    assert kind(out_aligned=False) == 1
    for extra in ("out_f32", "row_scale", "addend"):
        assert kind(**{extra: True}) == 0 and kind(gate_bits=True, out_gate=True, **{extra: True}) == 0
    # who writes the sign bits
    assert [choice(256, 256, **kw).bits_in_epilogue for kw in (dict(), dict(gate_bits=True), dict(out_gate=True))] == [1, 1, 0]


def test_workgroups_per_cu_and_key_11():
    # two workgroups per CU up to 80 KiB of LDS each
    small, big = choice(128, 192), choice(128, 256)
    assert small.lds_bytes == 3 * 4 * 32 * 128 + 20480 + 512 <= 80 * 1024 < big.lds_bytes == 4 * 4 * 32 * 128 + 20480 + 512
    assert (small.per_cu, small.workgroups, big.per_cu, big.workgroups) == (2, 512, 1, 256)
    with tuned(k11=1):
        assert choice(128, 192).per_cu == 1 and choice(128, 192).workgroups == 256
    with tuned(k11=3):                                   # only while the CU's 160 KiB hold that many
        assert choice(64, 64).per_cu == 3 and choice(64, 64).workgroups == 768
        assert choice(128, 192).per_cu == 2 and choice(128, 256).per_cu == 1
    assert choice(128, 192).per_cu == 2
    # the CU count comes in as a plain integer: whole groups of 16, 256 when unknown
    assert [choice(128, 256, n_cu=n).workgroups for n in (256, 255, 304, 17, 15, 0, -1)] == [256, 240, 304, 16, 16, 256, 256]
    assert choice(256, 512, n_cu=64).row_sequences == 32


def test_grid_cap_key_16():
    default = choice(128, 192).workgroups
    try:
        for v, want in ((0, default), (1, 16), (15, 16), (16, 16), (17, 16), (31, 16), (32, 32), (100, 96), (512, 512), (513, 512), (10000, default)):
            with tuned(k16=v):
                c = choice(128, 192, M=28237)
                assert c.workgroups == want == c.row_sequences and c.workgroups % 16 == 0 and c.workgroups <= default, v
                assert c.n_blocks == 56
                split = choice(256, 512, M=13901)                              # column shares: half as many row sequences
                assert split.row_sequences * 2 == split.workgroups == min(want, 256) and split.n_blocks == 28
                dual = choice(256, 64, dual=True)
                assert dual.row_sequences * 2 == dual.workgroups == want
                assert choice(128, 640).workgroups == 1                        # the 4-wave kernel's grid is not the knob's
        assert choice(128, 192).workgroups == default                          # back at the default
    finally:
        from dgll_amd import _lib

        _lib.check(_lib.lib.dgll_hip_debug_tune(16, 0), "dgll_hip_debug_tune")


def test_unknown_keys_are_still_refused():
    from dgll_amd import _lib

    for key in (6, 8, 10, 17, 99, -1):
        assert _lib.lib.dgll_hip_debug_tune(key, 1) == -1 and "unknown tuning key" in _lib.last_error(), key


def test_refusals_carry_code_and_text():
    from dgll_amd import _lib

    for kw, text in ((dict(N=257, K1=64), "keeps all N <= 256 output columns"),
                     (dict(N=64, K1=257, dual=True), "dgll_hip_transform_bf16_dual: N, K <= 256"),
                     (dict(N=257, K1=64, dual=True), "dgll_hip_transform_bf16_dual: N, K <= 256"),
                     (dict(N=64, K1=640, gate_bits=True), "gate_bits alone"),                     # the 4-wave kernel
                     (dict(N=64, K1=64, gate_bits=True, mask=True), "gate_bits alone"),
                     (dict(N=64, K1=64, gate_bits=True, addend=True), "gate_bits alone"),         # the general epilogue
                     (dict(N=64, K1=64, gate_bits=True, out_aligned=False), "gate_bits alone")):
        rc, c = choice(check=False, **kw)
        assert rc == -1 == c.error and text in c.message.decode() and text in _lib.last_error(), kw
    assert choice(64, 640, gate_bits=True, out_gate=True).kernel == FOUR_WAVE
    # a description that is none
    out = _lib.TransformChoice()
    ok = [64, 64, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1000, 256]
    assert _lib.lib.dgll_hip_debug_transform_choice(*ok, C.byref(out)) == 0
    assert _lib.lib.dgll_hip_debug_transform_choice(*ok, None) == -1
    for index, value in ((0, 0), (1, 0), (2, -1), (12, 0)):
        bad = list(ok)
        bad[index] = value
        assert _lib.lib.dgll_hip_debug_transform_choice(*bad, C.byref(out)) == -1, (index, value)


def test_steady_state_cases_name_their_instantiations():
    """tests/dense_cases.py, as the GPU test runs it: under the grid cap every case reaches the instantiation it is meant for, with
    3.5 row blocks per row sequence; together the cases leave no reachable instantiation out."""
    with tuned(k16=GRID_CAP):
        for case in CASES:
            m, c = steady_rows(case)
            assert instantiation(c) == case_instantiation(case), case.name
            assert m <= MAX_ROWS and c.n_blocks >= 3 * c.row_sequences and c.n_blocks % c.row_sequences != 0, case.name
    assert len({case.name for case in CASES}) == len(CASES)
    assert {case_instantiation(case) for case in CASES} == REACHABLE
    for case in REAL_GRID_CASES:
        assert instantiation(choice(**case_choice_args(case))) == case_instantiation(case), case.name
    assert {case.fam for case in REAL_GRID_CASES} == {case.fam for case in CASES}
