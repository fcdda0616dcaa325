"""Which SpMM kernel a launch gets (spmm.hip: spmm_choose), read through dgll_hip_debug_spmm_choice -- no device, no GPU.

Every expected value below is a literal taken from the kernel-choice table (spmm.hip's comment on spmm_choose, DESIGN.md
section 4.1) and from the `if` chain that stood in dgll_spmm_csr_impl before the choice became one function; none is computed
by the function under test.  Average row lengths are integer (n_rows, nnz) pairs: 10 rows and 241 edges are 24.1 edges per row."""
import ctypes as C
import importlib.util
import os

import pytest

from conftest import ROOT

W, S, G, F = 0, 1, 2, 3           # dgll_spmm_choice.kernel: wave-per-row, row-per-slot, row-group, flattened
F32, BF16 = 0, 1
# edges per row:  3.2  4.5  4.6  16.8  24   24.1  50.5  64   64.1  100   100.1
NNZ10 = (32, 45, 46, 168, 240, 241, 505, 640, 641, 1000, 1001)       # over 10 rows

# (dtype, feat) -> (lanes per row, kernels along NNZ10 for the plain launch, the same with accumulate / gate)
TABLE = {
    (BF16, 47): (8, (S, S, S, S, S, G, G, G, G, G, W), (S, S, S, S, S, W, W, W, W, W, W)),
    (BF16, 64): (8, (S, S, S, S, S, G, G, G, G, G, W), (S, S, S, S, S, W, W, W, W, W, W)),
    (BF16, 100): (16, (S, S, S, S, S, G, G, G, W, W, W), (S, S, S, S, S, W, W, W, W, W, W)),
    (BF16, 128): (16, (S, S, S, S, S, G, G, G, W, W, W), (S, S, S, S, S, W, W, W, W, W, W)),
    (BF16, 256): (32, (S, S, W, W, W, W, W, W, W, W, W), (S, S, W, W, W, W, W, W, W, W, W)),
    (F32, 100): (32, (S, S, W, F, F, F, F, F, F, F, F), (S, S, W, F, F, F, F, F, F, F, F)),
    (F32, 256): (64, (W,) * 11, (W,) * 11),
}


def choose(dtype, feat, n_rows=10, nnz=505, weighted=False, accumulate=0, gate=False, plan=True, aligned=True, only_long=False,
           y_dtype=None, n_chunks=0, n_flat=None):
    from dgll_amd import _lib

    if n_flat is None:
        n_flat = -(-(nnz + 4 * n_rows) // 256)       # what a plan of this graph holds
    out = _lib.SpmmChoice()
    _lib.check(_lib.lib.dgll_hip_debug_spmm_choice(dtype, dtype if y_dtype is None else y_dtype, feat, n_rows, int(plan), nnz, n_chunks,
                                                   n_flat, int(weighted), accumulate, int(gate), int(aligned), int(only_long),
                                                   C.byref(out)), "dgll_hip_debug_spmm_choice")
    return out


def what(c):
    return (c.kernel, c.lpr, c.spr, c.unroll, c.prefetch)


class knobs:
    """dgll_hip_debug_tune(key, value) for the block, the defaults restored in a finally."""
    DEFAULT = {0: 4, 1: 0, 2: 0, 3: 0, 5: 0, 13: 0, 14: 256, 15: 0}       # the initialisers of SpmmTune (spmm.hip): there is no getter; keep in step

    def __init__(self, **kv):
        self.kv = {int(k[1:]): v for k, v in kv.items()}

    def __enter__(self):
        from dgll_amd import _lib

        try:
            for k, v in self.kv.items():
                _lib.check(_lib.lib.dgll_hip_debug_tune(k, v), "dgll_hip_debug_tune")
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        from dgll_amd import _lib

        for k in self.kv:
            _lib.check(_lib.lib.dgll_hip_debug_tune(k, self.DEFAULT[k]), "dgll_hip_debug_tune")


def cases():
    for (dtype, feat), (lpr, plain, extra) in TABLE.items():
        for i, nnz in enumerate(NNZ10):
            for weighted in (False, True):
                for accumulate, gate in ((0, False), (1, False), (2, False), (0, True), (1, True)):
                    yield dtype, feat, lpr, nnz, weighted, accumulate, gate, (extra if accumulate or gate else plain)[i]


def test_the_table_row_by_row():
    for dtype, feat, lpr, nnz, weighted, accumulate, gate, kernel in cases():
        c = choose(dtype, feat, 10, nnz, weighted, accumulate, gate)
        spr = {W: 0, S: 1, G: 2, F: 0}[kernel]
        assert what(c) == (kernel, lpr, spr, 4, 0), (dtype, feat, nnz, weighted, accumulate, gate, what(c))
        assert c.epv == (8 if dtype == BF16 else 4)
        assert c.grid_y == 1
    # fp32 rows wider than 64 lanes x 4 take a second block column
    assert choose(F32, 300).grid_y == 2 and choose(F32, 300).lpr == 64
    # bf16 gathered, fp32 written: the same choice as bf16 / bf16
    assert what(choose(BF16, 47, 10, 505, y_dtype=F32)) == (G, 8, 2, 4, 0)
    assert what(choose(BF16, 256, 10, 505, y_dtype=F32)) == (W, 32, 0, 4, 0)


def test_no_plan_unaligned_and_only_long():
    for nnz in NNZ10:
        # no plan: "infinitely" long rows, one row per wavefront
        c = choose(BF16, 47, 10, nnz, plan=False)
        assert what(c) == (W, 8, 0, 4, 0) and c.rows_per_wave == 1 and c.row_blocks == 3 and c.chunk_blocks == 0
        assert what(choose(F32, 100, 10, nnz, plan=False)) == (W, 32, 0, 4, 0)
        assert what(choose(BF16, 256, 10, nnz, plan=False)) == (W, 32, 0, 4, 0)
        # operands that are not 16-byte aligned: one element per lane, 64 lanes per row, whatever the rows look like
        for dtype in (BF16, F32):
            for feat, gy in ((47, 1), (64, 1), (100, 2), (256, 4)):
                c = choose(dtype, feat, 10, nnz, aligned=False)
                assert what(c) == (W, 64, 0, 4, 0) and c.epv == 1 and c.grid_y == gy
        # only_long: the chunk items alone, on the wave-per-row kernel, no row blocks
        c = choose(BF16, 47, 10, nnz, only_long=True, n_chunks=5)
        assert what(c) == (W, 8, 0, 4, 0) and c.row_blocks == 0 and c.chunk_blocks == 8
        assert what(choose(F32, 100, 10, nnz, only_long=True)) == (W, 32, 0, 4, 0)
    # a plan without the flattened schedule
    assert what(choose(F32, 100, 10, 505, n_flat=0)) == (W, 32, 0, 4, 0)


def test_rows_per_wave_and_grid():
    # 96 KiB of gathered bytes per wavefront, 1 .. 8 rows: 50.5 edges x 512 B -> 3 rows, x 94 B -> 8 rows
    c = choose(BF16, 256, 1000, 50500)
    assert (c.kernel, c.rows_per_wave, c.row_blocks, c.chunk_blocks, c.grid_y) == (W, 3, 84, 0, 1)
    c = choose(BF16, 47, 1000, 50500, n_chunks=5)         # row-group, 4 rows at a time; 5 chunks = 2 blocks -> a multiple of 8
    assert (c.kernel, c.rows_per_wave, c.row_blocks, c.chunk_blocks, c.grid_y) == (G, 8, 32, 8, 1)
    c = choose(BF16, 47, 1000, 3200)                       # row-per-slot, 8 rows at a time
    assert (c.kernel, c.rows_per_wave, c.row_blocks) == (S, 8, 32)
    c = choose(F32, 100, 1000, 50500)                      # flattened: one wavefront per share of the plan's schedule
    assert (c.kernel, c.row_blocks, c.grid_y) == (F, 54, 1)      # (50500 + 4000) / 256 -> 213 shares -> 54 blocks
    with knobs(k1=3):
        assert choose(BF16, 256, 1000, 50500).rows_per_wave == 3 and choose(BF16, 256, 1000, 50500).row_blocks == 84
        c = choose(BF16, 47, 1000, 50500)                  # row-group at 8 lanes: 4 rows at a time
        assert (c.kernel, c.rows_per_wave, c.row_blocks) == (G, 4, 63)
        c = choose(BF16, 100, 1000, 50500)                 # row-group at 16 lanes: 2 rows at a time
        assert (c.kernel, c.rows_per_wave, c.row_blocks) == (G, 4, 63)
        c = choose(BF16, 47, 1000, 3200)                   # row-per-slot at 8 lanes: 8 rows at a time
        assert (c.kernel, c.rows_per_wave, c.row_blocks) == (S, 8, 32)
        c = choose(BF16, 128, 1000, 16800)                 # row-per-slot at 16 lanes: 4 rows at a time
        assert (c.kernel, c.rows_per_wave, c.row_blocks) == (S, 4, 63)
        assert choose(BF16, 47, 1000, 50500, plan=False).rows_per_wave == 1      # the knob needs a plan on the wave-per-row kernel
    with knobs(k1=5):
        assert choose(BF16, 256, 1000, 50500).rows_per_wave == 5 and choose(BF16, 256, 1000, 50500).row_blocks == 50
    # a multiple of the rows a wavefront handles at a time, whatever the shape; row_blocks follows
    for dtype, feat, lpr, nnz, weighted, accumulate, gate, kernel in cases():
        for n_rows in (10, 1000):
            c = choose(dtype, feat, n_rows, nnz * (n_rows // 10), weighted, accumulate, gate)
            at_a_time = {W: 1, F: 1, S: 64 // lpr, G: 64 // lpr // 2}[kernel]
            assert c.kernel == kernel and c.rows_per_wave % at_a_time == 0 and 1 <= c.rows_per_wave <= 8
            if kernel != F:
                assert c.row_blocks == -(-(-(-n_rows // c.rows_per_wave)) // 4)


def test_knob_unroll():
    for u in (2, 8):
        with knobs(k0=u):
            assert what(choose(BF16, 256, 10, 505)) == (W, 32, 0, u, 0)          # the wide rows exist at 2 / 4 / 8
            assert what(choose(F32, 256, 10, 505)) == (W, 64, 0, u, 0)
            assert what(choose(F32, 100, 10, 168)) == (W, 32, 0, u, 0)           # ... and the flattened kernel only at 4
            assert what(choose(BF16, 47, 10, 505)) == (W, 8, 0, 4, 0)            # so does the row-group kernel; narrow rows stay at 4
            assert what(choose(BF16, 100, 10, 505)) == (W, 16, 0, 4, 0)
            assert what(choose(BF16, 47, 10, 32)) == (S, 8, 1, 4, 0)             # the row-per-slot kernel does not care
            assert what(choose(BF16, 256, 10, 505, aligned=False)) == (W, 64, 0, 4, 0)
            with knobs(k15=2):
                assert what(choose(BF16, 47, 10, 505)) == (W, 8, 0, 4, 0)
            with knobs(k13=2):
                assert what(choose(BF16, 256, 10, 505)) == (W, 32, 0, u, 0)
    with knobs(k0=4):
        assert what(choose(BF16, 47, 10, 505)) == (G, 8, 2, 4, 0)
    with knobs(k0=3):                                                            # not a depth that exists: 4 is launched
        assert what(choose(BF16, 256, 10, 505)) == (W, 32, 0, 4, 0)


def test_knob_flags():
    with knobs(k2=1):                              # XCD remap: only the wave-per-row kernel has it
        assert what(choose(BF16, 47, 10, 505)) == (W, 8, 0, 4, 0)
        assert what(choose(BF16, 100, 10, 505)) == (W, 16, 0, 4, 0)
        assert what(choose(F32, 100, 10, 168)) == (W, 32, 0, 4, 0)
        assert what(choose(BF16, 47, 10, 32)) == (S, 8, 1, 4, 0)
        assert what(choose(BF16, 256, 10, 505)) == (W, 32, 0, 4, 0)
        with knobs(k15=2, k13=2):
            assert what(choose(BF16, 47, 10, 505)) == (W, 8, 0, 4, 0)
            assert what(choose(BF16, 256, 10, 505)) == (W, 32, 0, 4, 0)
    with knobs(k2=4):                              # next-row prefetch: bf16 / bf16 rows of 32 lanes at four gathers in flight
        assert what(choose(BF16, 256, 10, 505)) == (W, 32, 0, 4, 1)
        assert what(choose(BF16, 256, 10, 505, weighted=True, accumulate=1, gate=True)) == (W, 32, 0, 4, 1)
        assert what(choose(BF16, 256, 10, 505, y_dtype=F32)) == (W, 32, 0, 4, 0)
        assert what(choose(F32, 100, 10, 46)) == (W, 32, 0, 4, 0)
        assert what(choose(BF16, 512, 10, 505)) == (W, 64, 0, 4, 0)
        assert what(choose(BF16, 128, 10, 505)) == (G, 16, 2, 4, 0)
        assert what(choose(BF16, 128, 10, 1001)) == (W, 16, 0, 4, 0)
        assert what(choose(F32, 100, 10, 168)) == (F, 32, 0, 4, 0)
        assert what(choose(BF16, 256, 10, 32)) == (S, 32, 1, 4, 0)
        with knobs(k0=8):
            assert what(choose(BF16, 256, 10, 505)) == (W, 32, 0, 8, 0)
    with knobs(k2=5):
        assert what(choose(BF16, 256, 10, 505)) == (W, 32, 0, 4, 1)
        assert what(choose(BF16, 47, 10, 505)) == (W, 8, 0, 4, 0)


def test_knob_rowslot():
    with knobs(k5=1):                              # never: below 24 edges per row there is no row-group kernel either
        for nnz in NNZ10[:5]:
            assert what(choose(BF16, 47, 10, nnz)) == (W, 8, 0, 4, 0)
            assert what(choose(BF16, 128, 10, nnz)) == (W, 16, 0, 4, 0)
        assert what(choose(BF16, 256, 10, 32)) == (W, 32, 0, 4, 0)
        assert what(choose(F32, 100, 10, 32)) == (W, 32, 0, 4, 0)
        assert what(choose(F32, 100, 10, 168)) == (F, 32, 0, 4, 0)
        assert what(choose(BF16, 47, 10, 505)) == (G, 8, 2, 4, 0)
    with knobs(k5=2):                              # whenever it exists (rows of up to 32 lanes), ahead of the other two
        for nnz in NNZ10:
            assert what(choose(BF16, 47, 10, nnz)) == (S, 8, 1, 4, 0)
            assert what(choose(BF16, 256, 10, nnz)) == (S, 32, 1, 4, 0)
            assert what(choose(F32, 100, 10, nnz)) == (S, 32, 1, 4, 0)
            assert what(choose(F32, 256, 10, nnz)) == (W, 64, 0, 4, 0)
            assert what(choose(BF16, 47, 10, nnz, aligned=False)) == (W, 64, 0, 4, 0)
            assert what(choose(BF16, 47, 10, nnz, only_long=True)) == (W, 8, 0, 4, 0)
        c = choose(BF16, 47, 10, 505, plan=False)
        assert what(c) == (S, 8, 1, 4, 0) and c.rows_per_wave == 8
        with knobs(k1=3):                          # without a plan too
            assert choose(BF16, 128, 10, 505, plan=False).rows_per_wave == 4


def test_knob_flat():
    with knobs(k13=1):
        for nnz in NNZ10[2:]:
            assert what(choose(F32, 100, 10, nnz)) == (W, 32, 0, 4, 0)
    with knobs(k13=2):                             # whenever the plan has the schedule: rows of 16 / 32 lanes, bf16 included
        assert what(choose(BF16, 256, 10, 505)) == (F, 32, 0, 4, 0)
        assert what(choose(BF16, 256, 10, 505, weighted=True, accumulate=1, gate=True)) == (F, 32, 0, 4, 0)
        assert what(choose(BF16, 100, 10, 1000)) == (F, 16, 0, 4, 0)
        assert what(choose(BF16, 100, 10, 505)) == (G, 16, 2, 4, 0)              # the row-group band comes first
        assert what(choose(BF16, 100, 10, 505, accumulate=1)) == (F, 16, 0, 4, 0)
        assert what(choose(F32, 100, 10, 46)) == (F, 32, 0, 4, 0)
        assert what(choose(F32, 64, 10, 505)) == (F, 16, 0, 4, 0)
        assert what(choose(F32, 32, 10, 505)) == (W, 8, 0, 4, 0)                 # 8 lanes: not instantiated
        assert what(choose(BF16, 47, 10, 1001)) == (W, 8, 0, 4, 0)
        assert what(choose(F32, 256, 10, 505)) == (W, 64, 0, 4, 0)
        assert what(choose(BF16, 256, 10, 32)) == (S, 32, 1, 4, 0)
        assert what(choose(BF16, 256, 10, 505, n_flat=0)) == (W, 32, 0, 4, 0)
        assert what(choose(BF16, 256, 10, 505, plan=False)) == (W, 32, 0, 4, 0)
        assert what(choose(BF16, 256, 10, 505, only_long=True)) == (W, 32, 0, 4, 0)


def test_knob_rowgroup():
    with knobs(k15=1):                             # the choice before the kernel existed
        for nnz in NNZ10[5:]:
            assert what(choose(BF16, 47, 10, nnz)) == (W, 8, 0, 4, 0)
            assert what(choose(BF16, 100, 10, nnz)) == (W, 16, 0, 4, 0)
        assert what(choose(BF16, 47, 10, 240)) == (S, 8, 1, 4, 0)
    for v in (2, 4):                               # wherever it is instantiated: 8 lanes with v slots per row, 16 lanes with two
        with knobs(k15=v):
            for nnz in NNZ10[5:]:
                assert what(choose(BF16, 47, 10, nnz)) == (G, 8, v, 4, 0)
                assert what(choose(BF16, 64, 10, nnz, weighted=True)) == (G, 8, v, 4, 0)
                assert what(choose(BF16, 100, 10, nnz)) == (G, 16, 2, 4, 0)
                assert what(choose(BF16, 128, 10, nnz, y_dtype=F32)) == (G, 16, 2, 4, 0)
                assert what(choose(BF16, 7, 10, nnz)) == (W, 4, 0, 4, 0)         # one vector per row: never
                assert what(choose(BF16, 32, 10, nnz)) == (W, 4, 0, 4, 0)
                assert what(choose(BF16, 256, 10, nnz)) == (W, 32, 0, 4, 0)
                assert what(choose(BF16, 47, 10, nnz, accumulate=1)) == (W, 8, 0, 4, 0)
                assert what(choose(BF16, 47, 10, nnz, gate=True)) == (W, 8, 0, 4, 0)
                assert what(choose(BF16, 47, 10, nnz, only_long=True)) == (W, 8, 0, 4, 0)
                assert what(choose(BF16, 47, 10, nnz, aligned=False)) == (W, 64, 0, 4, 0)
                assert what(choose(F32, 32, 10, nnz)) == (W, 8, 0, 4, 0)         # fp32: never
            assert what(choose(F32, 100, 10, 505)) == (F, 32, 0, 4, 0)
            assert what(choose(BF16, 47, 10, 32)) == (S, 8, 1, 4, 0)             # the row-per-slot band comes first
            c = choose(BF16, 47, 10, 505, plan=False)
            assert what(c) == (G, 8, v, 4, 0) and c.rows_per_wave == 8 // v
            assert choose(BF16, 47, 1000, 50500).rows_per_wave == 8
            assert choose(BF16, 100, 10, 505, plan=False).rows_per_wave == 2


@pytest.fixture()
def bench():
    spec = importlib.util.spec_from_file_location("bench_for_choice", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fragment(c, dtype, weighted, extra, y_dtype=None):
    """The instantiation launch_rows() picks for the choice c, as bench.py names it; y_dtype: the output's, where it is not X's."""
    t = "unsigned short" if dtype == BF16 else "float"
    ty = t if y_dtype is None else ("unsigned short" if y_dtype == BF16 else "float")
    w, e = "true" if weighted else "false", "true" if extra else "false"
    if c.kernel == S:
        return "spmm_rowslot_kernel<%s, %s, %d, %d, %s, %s>" % (t, ty, c.epv, c.lpr, w, e)
    if c.kernel == F:
        return "spmm_csr_flat_kernel<%s, %s, %d, %d, %s, %d, %s>" % (t, ty, c.epv, c.lpr, w, c.unroll, e)
    if c.kernel == G:
        return "spmm_rowgroup_kernel<%s, %s, %d, %d, %d, %s>" % (t, ty, c.epv, c.lpr, c.spr, w)
    return "spmm_csr_kernel<%s, %s, %d, %d, %s, %d, %s, %s>" % (t, ty, c.epv, c.lpr, w, c.unroll, e, "true" if c.prefetch else "false")


def test_agrees_with_the_fragment_bench_names(bench):
    """bench.spmm_kernel_fragment names what the launch runs everywhere outside the row-group band (inside it bench.py still
    names the wave-per-row kernel: DESIGN.md section 10)."""
    compared = 0
    for dtype, feat, lpr, nnz, weighted, accumulate, gate, kernel in cases():
        extra = bool(accumulate or gate)
        c = choose(dtype, feat, 10, nnz, weighted, accumulate, gate)
        named = bench.spmm_kernel_fragment(feat, "torch.bfloat16" if dtype == BF16 else "torch.float32", weighted, extra, nnz / 10.0)
        if kernel == G:
            assert named.startswith("spmm_csr_kernel<") and fragment(c, dtype, weighted, extra).startswith("spmm_rowgroup_kernel<")
            continue
        assert fragment(c, dtype, weighted, extra) == named, (dtype, feat, nnz, weighted, accumulate, gate)
        compared += 1
    assert compared == 7 * 11 * 2 * 5 - 2 * 5 * 2 - 2 * 3 * 2
    # without an average row length bench names the wave-per-row kernel: the launch without a plan
    assert fragment(choose(BF16, 256, plan=False), BF16, True, True) == bench.spmm_kernel_fragment(256, "torch.bfloat16", True, True)
    assert fragment(choose(BF16, 47, plan=False), BF16, False, False) == bench.spmm_kernel_fragment(47, "torch.bfloat16", False, False)


def test_bad_descriptions_are_refused():
    from dgll_amd import _lib

    out = _lib.SpmmChoice()
    assert _lib.lib.dgll_hip_debug_spmm_choice(7, 0, 47, 10, 1, 505, 0, 3, 0, 0, 0, 1, 0, C.byref(out)) == -1
    assert _lib.lib.dgll_hip_debug_spmm_choice(1, 1, 0, 10, 1, 505, 0, 3, 0, 0, 0, 1, 0, C.byref(out)) == -1
    assert _lib.lib.dgll_hip_debug_spmm_choice(1, 1, 47, 10, 1, 505, 0, 3, 0, 0, 0, 1, 0, None) == -1
