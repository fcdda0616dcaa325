"""Which kernel a launch of the fused GAT passes gets (gat_choice.hpp: gat_choose), read through dgll_hip_debug_gat_choice -- no
device, no GPU.

Every expected value below is a literal worked out by hand from the rules as they stood before the choice became one function
(edge.hip's gat2_pick, gat2_inrow, gat1_pick, gat_schedule and gat_finalize, and the three launch ladders); none is computed by the
function under test."""
import ctypes as C
import importlib.util
import os

import pytest

from conftest import ROOT

F32, BF16 = 0, 1
FWD, ROWS, COLS = 0, 1, 2                      # pass: forward, rows of A, rows of A^T
INVALID, UNSUPPORTED = -1, -3                  # DGLL_ERR_*
NONE, WAVE, GROUP = 0, 1, 2                    # dgll_gat_choice.finalize

# (dtype, heads, fo) -> (lpr, nh, grid_y): second generation, compact 16-byte aligned scores
GEOMETRY = {
    (BF16, 8, 32): (32, 8, 1),
    (F32, 8, 32): (64, 8, 1),
    (BF16, 1, 48): (8, 1, 1),
    (BF16, 3, 24): (8, 2, 2),
    (BF16, 1, 8): (4, 1, 1),
    (BF16, 2, 16): (4, 2, 1),
    (BF16, 6, 8): (4, 2, 3),
}

NO_GAT2 = b"no second-generation GAT kernel for this head layout"
NO_DROP = b"no second-generation GAT kernel with dropout for this head layout"
NO_ROWSCORE = b"no row-score GAT kernel for this head layout"
ROWS_NEED_GAT2 = b"the row-score form and in-kernel dropout need the second-generation kernels [!attn2 && !drop]"
POW2 = (b"per-head width / vector must be a power of two <= 64 for the max-subtracted / dropout form (pad on the host) "
        b"[(*lph & (*lph - 1)) == 0 && *lph <= 64]")
STRIDED = b"strided score arrays need the second-generation kernels (mode 0, no attention dropout)"
EPILOGUE = b"the score-gradient epilogue needs the second-generation kernels [!attn1]"


def choose(pass_, dtype, heads, fo, mode=0, edge_scale=False, rowscore=False, drop=False, phase=3, t_stride=0, t_aligned=True,
           dd_aligned=True, sd_out=False, epilogue=False, behind=False, pitch=False, second=True, pad=0, plan=False, n_rows=10, nnz=505,
           n_chunks=0, n_long=0, y_aligned=True, code=0):
    from dgll_amd import _lib

    out = _lib.GatChoice()
    rc = _lib.lib.dgll_hip_debug_gat_choice(pass_, dtype, heads, fo, mode, int(edge_scale), int(rowscore), int(drop), phase, t_stride,
                                            int(t_aligned), int(dd_aligned), int(sd_out), int(epilogue), int(behind), int(pitch),
                                            int(second), pad, int(plan), n_rows, nnz, n_chunks, n_long, int(y_aligned), C.byref(out))
    assert rc == code == out.error, (rc, out.error, _lib.last_error())
    if code:
        assert _lib.last_error() == out.message.decode()
    return out


def form(c):
    return (c.generation, c.kind, c.trow, c.drop, c.inrow)


def geom(c):
    return (c.lpr, c.nh, c.grid_y)


def packed(n=8):
    """The gathered-side scores in the padding of the gathered rows: behind the last column, one row pitch apart, n bytes of padding."""
    return dict(behind=True, pitch=True, second=True, pad=n)


class knob9:
    """dgll_hip_debug_tune(9, value) for the block, the default restored in a finally."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from dgll_amd import _lib

        try:
            _lib.check(_lib.lib.dgll_hip_debug_tune(9, self.value), "dgll_hip_debug_tune")
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        from dgll_amd import _lib

        _lib.check(_lib.lib.dgll_hip_debug_tune(9, 0), "dgll_hip_debug_tune")      # GatTune's initialiser (gat_choice.hpp)


def test_geometry_row_by_row():
    for (dtype, heads, fo), expected in GEOMETRY.items():
        for pass_, phase in ((FWD, 0), (ROWS, 0), (ROWS, 3), (COLS, 0)):
            c = choose(pass_, dtype, heads, fo, phase=phase)
            assert c.generation == 2 and geom(c) == expected, (dtype, heads, fo, pass_, geom(c))
            assert c.epv == (8 if dtype == BF16 else 4) and c.unroll == 4 and c.lph == c.lpr // c.nh
    # blocks of four heads are read as float4s: whole blocks of 16-byte aligned, 4-float-strided scores -- or two heads at a time
    assert geom(choose(FWD, BF16, 4, 8)) == (4, 4, 1)
    assert geom(choose(FWD, BF16, 4, 8, t_stride=8)) == (4, 4, 1)
    assert geom(choose(FWD, BF16, 4, 8, t_stride=5)) == (4, 2, 2)
    assert geom(choose(FWD, BF16, 4, 8, t_aligned=False)) == (4, 2, 2)
    assert geom(choose(COLS, BF16, 4, 8, dd_aligned=False)) == (4, 2, 2)
    assert geom(choose(FWD, BF16, 8, 32, t_aligned=False)) == (8, 2, 4)
    # the row-score form reads no score row: neither its stride nor its alignment matters
    assert geom(choose(FWD, BF16, 4, 8, rowscore=True, t_aligned=False)) == (4, 4, 1)
    assert geom(choose(ROWS, BF16, 8, 32, rowscore=True, t_aligned=False)) == (32, 8, 1)
    # a head of 64 vectors fills the wavefront; 48 bf16 columns on 8 lanes, 48 fp32 ones on 16
    assert geom(choose(FWD, BF16, 2, 512)) == (64, 1, 2)
    assert geom(choose(FWD, F32, 1, 48)) == (16, 1, 1)


def test_forms_per_entry_point():
    for dtype, heads, fo in GEOMETRY:
        assert form(choose(FWD, dtype, heads, fo)) == (2, 0, 0, 0, 0)
        assert form(choose(FWD, dtype, heads, fo, rowscore=True)) == (2, 0, 1, 0, 0)
        assert form(choose(FWD, dtype, heads, fo, drop=True)) == (2, 0, 0, 1, 0)
        assert form(choose(FWD, dtype, heads, fo, rowscore=True, drop=True)) == (2, 0, 1, 1, 0)
        for phase in (0, 1, 2, 7):                 # 2, 7: not a phase, read as 0
            assert form(choose(ROWS, dtype, heads, fo, phase=phase)) == (2, 1, 0, 0, 0)
        for phase in (3, 4, 5, 6):
            assert form(choose(ROWS, dtype, heads, fo, phase=phase)) == (2, 3, 0, 0, 0)
        assert form(choose(ROWS, dtype, heads, fo, sd_out=True)) == (2, 3, 0, 0, 0)
        assert form(choose(ROWS, dtype, heads, fo, rowscore=True)) == (2, 3, 1, 0, 0)
        assert form(choose(ROWS, dtype, heads, fo, drop=True)) == (2, 3, 0, 1, 0)
        assert form(choose(ROWS, dtype, heads, fo, rowscore=True, drop=True)) == (2, 3, 1, 1, 0)
        assert form(choose(COLS, dtype, heads, fo)) == (2, 2, 0, 0, 0)
        assert form(choose(COLS, dtype, heads, fo, epilogue=True)) == (2, 2, 0, 0, 0)
        assert form(choose(COLS, dtype, heads, fo, drop=True, epilogue=True)) == (2, 2, 0, 1, 0)
        # what is not instantiated: the stored-output rows pass in the row-score form or with dropout, the transposed pass in the
        # row-score form (it gathers DN rows)
        for phase in (0, 1):
            for rowscore, drop in ((True, False), (False, True), (True, True)):
                assert choose(ROWS, dtype, heads, fo, phase=phase, rowscore=rowscore, drop=drop, code=UNSUPPORTED).message == NO_GAT2
        for drop in (False, True):
            assert choose(COLS, dtype, heads, fo, rowscore=True, drop=drop, code=UNSUPPORTED).message == NO_GAT2


def test_in_row_form():
    # one head, 6 of 8 lanes (bf16) / 12 of 16 (fp32) hold columns, the score slot right behind the row at the row's pitch
    for dtype in (BF16, F32):
        assert form(choose(FWD, dtype, 1, 48, **packed(4))) == (2, 0, 0, 0, 1)
        assert form(choose(ROWS, dtype, 1, 48, phase=0, **packed(4))) == (2, 1, 0, 0, 1)
        assert form(choose(ROWS, dtype, 1, 48, phase=3, **packed(4))) == (2, 3, 0, 0, 1)
        assert form(choose(ROWS, dtype, 1, 48, phase=5, **packed(4))) == (2, 3, 0, 0, 1)
        assert form(choose(COLS, dtype, 1, 48, **packed(8))) == (2, 2, 0, 0, 1)
    assert geom(choose(FWD, BF16, 1, 48, **packed())) == (8, 1, 1)
    assert form(choose(FWD, BF16, 1, 8, **packed())) == (2, 0, 0, 0, 1)                # 1 of 4 lanes
    # each condition on its own
    assert form(choose(FWD, BF16, 1, 48)) == (2, 0, 0, 0, 0)
    assert form(choose(FWD, BF16, 1, 48, behind=False, pitch=True, pad=8)) == (2, 0, 0, 0, 0)
    assert form(choose(FWD, BF16, 1, 48, behind=True, pitch=False, pad=8)) == (2, 0, 0, 0, 0)
    assert form(choose(FWD, BF16, 1, 48, behind=True, pitch=True, pad=3)) == (2, 0, 0, 0, 0)
    assert form(choose(FWD, BF16, 1, 64, **packed())) == (2, 0, 0, 0, 0)               # 8 vectors on 8 lanes: no idle lane
    assert form(choose(FWD, BF16, 2, 16, **packed())) == (2, 0, 0, 0, 0)               # two heads
    assert form(choose(FWD, BF16, 3, 24, **packed(12))) == (2, 0, 0, 0, 0)
    # the transposed pass fetches {s, dd}: dd one float after s, 8 bytes of padding
    assert form(choose(COLS, BF16, 1, 48, **packed(4))) == (2, 2, 0, 0, 0)
    assert form(choose(COLS, BF16, 1, 48, behind=True, pitch=True, second=False, pad=8)) == (2, 2, 0, 0, 0)
    # never in the row-score form or with dropout
    for pass_ in (FWD, ROWS):
        assert form(choose(pass_, BF16, 1, 48, rowscore=True, **packed())) == (2, 3 * pass_, 1, 0, 0)
        assert form(choose(pass_, BF16, 1, 48, drop=True, **packed())) == (2, 3 * pass_, 0, 1, 0)
        assert form(choose(pass_, BF16, 1, 48, rowscore=True, drop=True, **packed())) == (2, 3 * pass_, 1, 1, 0)
    assert form(choose(COLS, BF16, 1, 48, drop=True, **packed())) == (2, 2, 0, 1, 0)
    # key 9 = 2: the second generation without it
    with knob9(2):
        for pass_, kind in ((FWD, 0), (ROWS, 3), (COLS, 2)):
            c = choose(pass_, BF16, 1, 48, **packed())
            assert form(c) == (2, kind, 0, 0, 0) and geom(c) == (8, 1, 1)
        assert geom(choose(FWD, BF16, 8, 32)) == (32, 8, 1)
    assert form(choose(FWD, BF16, 1, 48, **packed())) == (2, 0, 0, 0, 1)


def first_generation(c):
    return (c.generation, c.lph, c.lpr, c.grid_y, c.unroll, c.inrow, c.nh)


def test_first_generation_fallback():
    def check(**how):
        for pass_, kind, unroll in ((FWD, 0, 4), (ROWS, 1, 2), (COLS, 2, 2)):
            c = choose(pass_, BF16, 8, 32, phase=0, **how)
            assert first_generation(c) == (1, 4, 32, 1, unroll, 0, 0) and c.kind == kind and c.epv == 8
            assert first_generation(choose(pass_, F32, 8, 64, phase=1, **how)) == (1, 16, 64, 2, unroll, 0, 0)
            assert first_generation(choose(pass_, BF16, 1, 8, phase=3, **how)) == (1, 1, 4, 1, unroll, 0, 0)
            assert first_generation(choose(pass_, BF16, 1, 512, phase=6, **how)) == (1, 64, 64, 1, unroll, 0, 0)
            assert first_generation(choose(pass_, BF16, 1, 64, **packed(), **how)) == (1, 8, 8, 1, unroll, 0, 0)
            # a per-head width that is not a power-of-two number of vectors; strided scores
            assert choose(pass_, BF16, 3, 24, code=INVALID, **how).message == POW2
            assert choose(pass_, BF16, 1, 48, code=INVALID, **how).message == POW2
            assert choose(pass_, BF16, 8, 32, t_stride=16, code=UNSUPPORTED, **how).message == STRIDED
            assert choose(pass_, BF16, 3, 24, t_stride=16, code=INVALID, **how).message == POW2          # the width is looked at first
        assert choose(ROWS, BF16, 8, 32, sd_out=True, code=UNSUPPORTED, **how).message == STRIDED
        # the forms only the second generation has
        assert choose(FWD, BF16, 8, 32, drop=True, code=UNSUPPORTED, **how).message == NO_DROP
        assert choose(FWD, BF16, 8, 32, rowscore=True, code=UNSUPPORTED, **how).message == NO_ROWSCORE
        assert choose(FWD, BF16, 8, 32, rowscore=True, drop=True, code=UNSUPPORTED, **how).message == NO_DROP
        for rowscore, drop in ((True, False), (False, True), (True, True)):
            assert choose(ROWS, BF16, 8, 32, rowscore=rowscore, drop=drop, code=INVALID, **how).message == ROWS_NEED_GAT2
        assert choose(COLS, BF16, 8, 32, drop=True, code=UNSUPPORTED, **how).message == NO_DROP
        assert choose(COLS, BF16, 8, 32, epilogue=True, code=INVALID, **how).message == EPILOGUE
        assert choose(COLS, BF16, 8, 32, epilogue=True, t_stride=16, code=UNSUPPORTED, **how).message == STRIDED

    check(mode=1)
    check(edge_scale=True)
    with knob9(1):
        check()
    assert choose(FWD, BF16, 8, 32).generation == 2


def test_heads_wider_than_a_wavefront():
    # more than 64 vectors per head: no second-generation kernel, and the first generation refuses the width
    for pass_ in (FWD, ROWS, COLS):
        assert choose(pass_, BF16, 1, 1024, code=INVALID).message == POW2
        assert choose(pass_, F32, 2, 260, code=INVALID).message == POW2
    assert choose(FWD, BF16, 1, 1024, drop=True, code=UNSUPPORTED).message == NO_DROP
    assert choose(FWD, BF16, 1, 1024, rowscore=True, code=UNSUPPORTED).message == NO_ROWSCORE
    assert choose(ROWS, BF16, 1, 1024, rowscore=True, code=INVALID).message == ROWS_NEED_GAT2
    assert choose(COLS, BF16, 1, 1024, drop=True, code=UNSUPPORTED).message == NO_DROP
    assert geom(choose(FWD, BF16, 1, 512)) == (64, 1, 1) and geom(choose(FWD, F32, 1, 256)) == (64, 1, 1)


def schedule(c):
    return (c.rows_per_wave, c.row_blocks, c.chunk_blocks)


def test_schedule():
    for pass_ in (FWD, ROWS, COLS):
        # no plan: one row per wavefront, four wavefronts per block, no chunk items (whatever the plan's numbers would be)
        assert schedule(choose(pass_, BF16, 8, 32, n_rows=10, nnz=505, n_chunks=5)) == (1, 3, 0)
        assert schedule(choose(pass_, BF16, 8, 32, n_rows=1000)) == (1, 250, 0)
        # a plan: 96 KiB of gathered bytes per wavefront, 1 .. 8 rows.  256 bf16 columns: 50.5 edges x 512 B -> 3 rows
        assert schedule(choose(pass_, BF16, 8, 32, plan=True, n_rows=10, nnz=505)) == (3, 1, 0)
        assert schedule(choose(pass_, BF16, 8, 32, plan=True, n_rows=1000, nnz=50500)) == (3, 84, 0)
        assert schedule(choose(pass_, BF16, 8, 32, plan=True, n_rows=10, nnz=960)) == (2, 2, 0)          # 96 x 512 B = 48 KiB exactly
        assert schedule(choose(pass_, BF16, 8, 32, plan=True, n_rows=10, nnz=961)) == (1, 3, 0)
        assert schedule(choose(pass_, BF16, 8, 32, plan=True, n_rows=10, nnz=10000)) == (1, 3, 0)        # 500 KiB: the lower end
        assert schedule(choose(pass_, BF16, 8, 32, plan=True, n_rows=10, nnz=240)) == (8, 1, 0)          # 24 x 512 B = 12 KiB exactly
        assert schedule(choose(pass_, BF16, 8, 32, plan=True, n_rows=10, nnz=241)) == (7, 1, 0)
        assert schedule(choose(pass_, BF16, 8, 32, plan=True, n_rows=1000, nnz=3200)) == (8, 32, 0)      # 1.6 KiB: the upper end
        assert schedule(choose(pass_, BF16, 8, 32, plan=True, n_rows=10, nnz=0)) == (8, 1, 0)
        assert schedule(choose(pass_, F32, 8, 32, plan=True, n_rows=1000, nnz=50500)) == (1, 250, 0)     # fp32: 50.5 x 1 KiB
        assert schedule(choose(pass_, BF16, 1, 48, plan=True, n_rows=1000, nnz=50500)) == (8, 32, 0)     # 50.5 x 96 B
        # the first-generation kernels walk the same schedule
        assert schedule(choose(pass_, BF16, 8, 32, mode=1, plan=True, n_rows=1000, nnz=50500, n_chunks=5)) == (3, 84, 2)
        # chunk items: four per block, in front of the row blocks
        for n_chunks, blocks in ((0, 0), (1, 1), (4, 1), (5, 2), (4001, 1001)):
            assert schedule(choose(pass_, BF16, 8, 32, plan=True, n_rows=1000, nnz=50500, n_chunks=n_chunks)) == (3, 84, blocks)


def test_finalize_variant():
    for pass_ in (FWD, ROWS, COLS):
        assert choose(pass_, BF16, 8, 32).finalize == NONE
        assert choose(pass_, BF16, 8, 32, plan=True, n_chunks=5).finalize == NONE                  # chunks of no long row: none
        assert choose(pass_, BF16, 8, 32, n_chunks=5, n_long=2).finalize == NONE                   # no plan
        assert choose(pass_, BF16, 8, 32, plan=True, n_chunks=5, n_long=2).finalize == WAVE
        assert choose(pass_, BF16, 64, 8, plan=True, n_chunks=5, n_long=2).finalize == WAVE
        assert choose(pass_, BF16, 65, 8, plan=True, n_chunks=5, n_long=2).finalize == GROUP
        assert choose(pass_, BF16, 8, 32, mode=1, plan=True, n_chunks=5, n_long=2).finalize == WAVE
    # output rows that do not admit the four-column stores: a workgroup per row -- but the rows pass's long rows end in fp32 scalars
    assert choose(FWD, BF16, 8, 32, plan=True, n_chunks=5, n_long=2, y_aligned=False).finalize == GROUP
    assert choose(COLS, F32, 8, 32, plan=True, n_chunks=5, n_long=2, y_aligned=False).finalize == GROUP
    assert choose(ROWS, BF16, 8, 32, plan=True, n_chunks=5, n_long=2, y_aligned=False).finalize == WAVE
    assert choose(ROWS, BF16, 65, 8, plan=True, n_chunks=5, n_long=2, y_aligned=False).finalize == GROUP


@pytest.fixture()
def bench():
    spec = importlib.util.spec_from_file_location("bench_for_gat_choice", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fragment(c, dtype):
    t = "unsigned short" if dtype == BF16 else "float"
    return "gat2_kernel<%s, %s, %d, %d, %d, %d, %d, %s, %s>" % (t, t, c.epv, c.lpr, c.nh, c.unroll, c.kind, "true" if c.inrow else "false",
                                                                 "true" if c.trow else "false")


def test_agrees_with_the_fragment_bench_names(bench):
    """bench.gat_kernel_fragment names the instantiation the launch runs wherever one exists.  It also names two that do not: the
    stored-output rows pass and the transposed pass with rowscore=True (the launch refuses those), and INROW together with TROW for one
    packed head (the launch runs the row-score form without INROW: it reads no score at all)."""
    compared = refused = inrow_named = 0
    for (dtype, heads, fo) in GEOMETRY:
        name = "torch.bfloat16" if dtype == BF16 else "torch.float32"
        for kind, pass_, phase in ((0, FWD, 0), (1, ROWS, 0), (2, COLS, 0), (3, ROWS, 3)):
            for pack in (False, True):
                for rowscore in (False, True):
                    named = bench.gat_kernel_fragment(heads, fo, name, kind, packed=pack, rowscore=rowscore)
                    how = packed() if pack else {}
                    if rowscore and kind in (1, 2):
                        assert choose(pass_, dtype, heads, fo, phase=phase, rowscore=True, code=UNSUPPORTED, **how).message == NO_GAT2
                        refused += 1
                        continue
                    c = choose(pass_, dtype, heads, fo, phase=phase, rowscore=rowscore, **how)
                    if rowscore and pack and heads == 1:
                        assert named.endswith("true, true>") and fragment(c, dtype) == named.replace("true, true>", "false, true>")
                        inrow_named += 1
                        continue
                    assert fragment(c, dtype) == named, (dtype, heads, fo, kind, pack, rowscore)
                    compared += 1
    assert (compared, refused, inrow_named) == (7 * 4 * 4 - 28 - 4, 7 * 2 * 2, 2 * 2)


def test_bad_descriptions_are_refused():
    from dgll_amd import _lib

    out = _lib.GatChoice()
    ok = [FWD, BF16, 8, 32, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 10, 0, 0, 0, 1]
    assert _lib.lib.dgll_hip_debug_gat_choice(*ok, C.byref(out)) == 0
    assert _lib.lib.dgll_hip_debug_gat_choice(*ok, None) == -1
    for index, value in ((0, 3), (1, 2), (2, 0), (3, 0), (3, 12), (4, 2), (19, 0)):      # pass, dtype, heads, fo, fo % 8, mode, n_rows
        bad = list(ok)
        bad[index] = value
        assert _lib.lib.dgll_hip_debug_gat_choice(*bad, C.byref(out)) == -1, (index, value)
