"""The attention-dropout multiplier of the fused GAT passes (csrc/gat_dropout.hpp) on the host: dgll_host_gat_dropout_mask against a
numpy restatement of the generator written here, and the statistics of its draws.  No GPU: the device kernels evaluate the same
integer function (tests/test_gat_dropout_gpu.py checks that they agree bit for bit).

Seeds are fixed constants: the tests are deterministic statements about this generator, with 5-sigma bounds that a sound generator
misses about once in 1.7 million tries per comparison."""
import numpy as np
import pytest
import torch

SEEDS = [(0x1234ABCD, 0x0F1E2D3C), (0x9E3779B9, 0x7F4A7C15), (3, 0)]      # (seed word 0, seed word 1)
PS = [0.1, 0.5, 0.6]
U32 = np.uint32


# ---- the generator, restated ------------------------------------------------------------------------------------------------
def _mix(x):
    x = x.astype(U32)
    x = x ^ (x >> U32(16))
    x = x * U32(0x21F0AAAD)
    x = x ^ (x >> U32(15))
    x = x * U32(0x735A2D97)
    x = x ^ (x >> U32(15))
    return x


def _draws(seed, row, col, heads):
    """uint32 [E, heads]: draw of head k of edge (row, col) = mix((R + k G) ^ rotl(C, 5 k + 1)), R = mix(mix(row ^ s0) + s1),
    C = mix(~col ^ s1) + s0."""
    s0, s1 = U32(seed[0]), U32(seed[1])
    with np.errstate(over="ignore"):
        rk = _mix(_mix(row.astype(U32) ^ s0) + s1)
        ck = _mix(~col.astype(U32) ^ s1) + s0
        out = np.empty((len(row), heads), U32)
        for k in range(heads):
            rot = (5 * k + 1) & 31
            rotated = ck if rot == 0 else ((ck << U32(rot)) | (ck >> U32(32 - rot)))
            out[:, k] = _mix((rk + U32((k * 0x9E3779B9) & 0xFFFFFFFF)) ^ rotated)
    return out


def _mask_numpy(seed, p, row, col, heads):
    thresh = int(p * 4294967296.0)
    scale = np.float32(1.0 / (1.0 - p))
    return np.where(_draws(seed, row, col, heads) < thresh, np.float32(0.0), scale).astype(np.float32)


# ---- the library ---------------------------------------------------------------------------------------------------------------
def _mask_host(seed, p, rowptr, col, heads):
    from dgll_amd import _lib

    rowptr = np.ascontiguousarray(rowptr, np.int64)
    col = np.ascontiguousarray(col, np.int32)
    words = np.array([seed[0], seed[1]], np.uint32)
    out = np.full((len(col), heads), np.nan, np.float32)
    code = _lib.lib.dgll_host_gat_dropout_mask(rowptr.ctypes.data, col.ctypes.data, len(rowptr) - 1, heads, words.ctypes.data, float(p),
                                               out.ctypes.data)
    _lib.check(code, "dgll_host_gat_dropout_mask")
    return out


def _random_csr(n, deg, seed, n_cols=None):
    rng = np.random.default_rng(seed)
    n_cols = n if n_cols is None else n_cols
    rowptr = np.arange(n + 1, dtype=np.int64) * deg
    col = rng.integers(0, n_cols, n * deg).astype(np.int32)
    return rowptr, col


def _rows(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


# ---- tests -----------------------------------------------------------------------------------------------------------------
def test_host_mask_equals_the_numpy_restatement_bit_for_bit():
    """Row ids above 2^24 (the last rows of a 2^24 + 64-row structure whose other rows are mostly empty), column ids up to 2^31 - 1,
    ten heads (rotations past 32 bits wrap): every multiplier equals the restatement's."""
    n = (1 << 24) + 64
    deg = np.zeros(n, np.int64)
    deg[:200] = 5
    deg[-64:] = 7
    deg[[1 << 20, (1 << 24) - 1, 1 << 24]] = 3
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=rowptr[1:])
    rng = np.random.default_rng(11)
    col = rng.integers(0, (1 << 31) - 1, int(rowptr[-1])).astype(np.int32)
    col[:4] = [0, 1, (1 << 31) - 1, 1 << 24]
    row = _rows(rowptr)
    assert row.max() > (1 << 24) and col.max() > (1 << 24)
    for seed in SEEDS:
        for p in (0.6, 0.1):
            got = _mask_host(seed, p, rowptr, col, 10)
            want = _mask_numpy(seed, p, row, col, 10)
            assert got.tobytes() == want.tobytes(), (seed, p)


@pytest.mark.parametrize("p", PS)
def test_every_multiplier_is_exactly_zero_or_the_scale(p):
    rowptr, col = _random_csr(4000, 16, seed=2)
    for seed in SEEDS:
        m = _mask_host(seed, p, rowptr, col, 8)
        scale = np.float32(1.0 / (1.0 - p))
        assert np.all((m == np.float32(0.0)) | (m == scale))
        assert set(np.unique(m.view(np.uint32))) == {0, int(scale.view(np.uint32))}      # +0.0 and the scale, bit patterns


@pytest.mark.parametrize("p", PS)
def test_keep_rate(p):
    rowptr, col = _random_csr(20000, 16, seed=3)        # 320 000 edges x 4 heads = 1.28e6 draws
    for seed in SEEDS:
        m = _mask_host(seed, p, rowptr, col, 4)
        n_draws = m.size
        assert n_draws >= 10 ** 6
        kept = np.count_nonzero(m) / n_draws
        bound = 5.0 * np.sqrt(p * (1.0 - p) / n_draws)
        print("p %.1f seed %08x:%08x kept %.6f want %.6f bound %.6f" % (p, seed[0], seed[1], kept, 1.0 - p, bound))
        assert abs(kept - (1.0 - p)) <= bound, (p, seed, kept, bound)


def _agreement(a, b, p, what):
    n_draws = a.size
    q = p * p + (1.0 - p) * (1.0 - p)
    rate = np.count_nonzero((a != 0) == (b != 0)) / n_draws
    bound = 5.0 * np.sqrt(q * (1.0 - q) / n_draws)
    print("%s: p %.1f agreement %.6f want %.6f bound %.6f (%d draws)" % (what, p, rate, q, bound, n_draws))
    assert abs(rate - q) <= bound, (what, p, rate, q, bound)


@pytest.mark.parametrize("p", PS)
def test_independence_between_seeds_heads_and_edge_directions(p):
    n, deg, heads = 20000, 16, 4
    rowptr, col = _random_csr(n, deg, seed=4)
    row = _rows(rowptr)
    masks = [_mask_host(seed, p, rowptr, col, heads) for seed in SEEDS]
    # two seeds -- also seeds that differ in ONE word, and in one bit
    _agreement(masks[0], masks[1], p, "seeds")
    _agreement(masks[0], _mask_host((SEEDS[0][0], SEEDS[0][1] ^ 1), p, rowptr, col, heads), p, "seed word 1 differs in one bit")
    _agreement(masks[0], _mask_host((SEEDS[0][0] + 1, SEEDS[0][1]), p, rowptr, col, heads), p, "seed word 0 + 1")
    # two heads of the same edge: every pair of the four heads
    for seed, m in zip(SEEDS, masks):
        for k in range(heads):
            for k2 in range(k + 1, heads):
                _agreement(m[:, k], m[:, k2], p, "heads %d/%d" % (k, k2))
    # (i, j) against (j, i): the same edge list with the ends swapped, as a CSR of its own
    keep = row != col
    order = np.lexsort((row[keep], col[keep]))          # sorted by (col, row): rows of the swapped structure
    t_row, t_col = col[keep][order].astype(np.int64), row[keep][order].astype(np.int32)
    t_rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(t_row, minlength=n), out=t_rowptr[1:])
    for seed, m in zip(SEEDS, masks):
        swapped = _mask_host(seed, p, t_rowptr, t_col, heads)
        _agreement(m[keep][order], swapped, p, "(i, j) / (j, i)")


def test_neighbouring_ids_are_unrelated():
    """Edges (i, j) / (i, j + 1) and (i, j) / (i + 1, j): counters that differ in one low bit."""
    p, heads = 0.5, 4
    n = 300000
    row = np.arange(n, dtype=np.int64)
    col = np.random.default_rng(5).integers(0, 1 << 27, n).astype(np.int32) & ~np.int32(1)
    rowptr = np.arange(n + 1, dtype=np.int64)
    base = _mask_host(SEEDS[1], p, rowptr, col, heads)
    _agreement(base, _mask_host(SEEDS[1], p, rowptr, col + 1, heads), p, "j / j + 1")
    shifted = _mask_numpy(SEEDS[1], p, row + 1, col, heads)
    _agreement(base, shifted, p, "i / i + 1")


def test_duplicate_entries_share_a_draw_and_p_is_validated():
    from dgll_amd import _lib

    rowptr = np.array([0, 4], np.int64)
    col = np.array([7, 7, 9, 7], np.int32)
    m = _mask_host(SEEDS[0], 0.5, rowptr, col, 6)
    assert np.array_equal(m[0], m[1]) and np.array_equal(m[0], m[3])
    words = np.array(SEEDS[0], np.uint32)
    out = np.zeros((4, 6), np.float32)
    for bad in (1.0, -0.1, 1.5, float("nan")):
        code = _lib.lib.dgll_host_gat_dropout_mask(rowptr.ctypes.data, col.ctypes.data, 1, 6, words.ctypes.data, bad, out.ctypes.data)
        assert code == -1 and "[0, 1)" in _lib.last_error()
    # p = 0 keeps everything, multiplier exactly 1
    assert np.all(_mask_host(SEEDS[0], 0.0, rowptr, col, 6) == np.float32(1.0))


def test_python_wrapper_on_host_tensors():
    """ops.gat_dropout_mask on a host CSRGraph goes through the same entry point."""
    import dgll_amd
    from dgll_amd import ops

    rowptr, col = _random_csr(500, 6, seed=6)
    g = dgll_amd.CSRGraph(torch.from_numpy(rowptr), torch.from_numpy(col), None, 500, 500)
    seed = torch.from_numpy(np.array(SEEDS[0], np.uint32).view(np.int32).copy())
    got = ops.gat_dropout_mask(g, 3, 0.6, seed).numpy()
    assert got.tobytes() == _mask_numpy(SEEDS[0], 0.6, _rows(rowptr), col, 3).tobytes()
