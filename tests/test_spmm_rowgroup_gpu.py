"""The row-group SpMM kernel (spmm_rowgroup_kernel: several rows per wavefront, 2 or 4 slots each) vs the CPU oracle and vs the
kernels it replaces, on graphs whose average row length lies in its band.  GPU box only (-m gpu).

Tolerances are the ones tests/test_ops_gpu.py uses against the same oracle: bf16 output rtol = atol = 8e-3, fp32 output (bf16
gather, fp32 accumulation, no output rounding) rtol = atol = 1e-4.  dgll_hip_debug_tune(15, v): 0 = automatic choice, 1 = the
choice before the kernel existed, 2 / 4 = the kernel wherever it is instantiated with that many slots per row (F = 7 has no
instantiation and stays on the old kernel under every value)."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import cref

pytestmark = pytest.mark.gpu

U = 4                      # gathers in flight per lane: a round of the kernel is SPR x U edges per row
N_ROWS = 1003              # neither a multiple of the rows per wavefront (2, 4) nor of rows_per_wave: the last wave is partly filled
# row -> length.  Rows 4..7 are one lane-group set of a wavefront at 4 rows per wave: a short row, an empty one, a LONG one (above
# the plan's threshold: runs as chunk items) and a short one; 8 k + 1, exactly 8 / 16 and 0 edges elsewhere, the last row empty.
SPECIAL = {0: 0, 1: 8, 2: 16, 3: 9, 4: 5, 5: 0, 6: 650, 7: 3, 8: 17, 9: 25, 10: 33, 11: 1, 12: 7, 13: 15, 14: 24, 15: 32,
           500: 900, 501: 0, 502: 0, 503: 0, 1000: 41, 1001: 8, N_ROWS - 1: 0}


@contextlib.contextmanager
def rowgroup_choice(value):
    from dgll_amd import _lib

    _lib.check(_lib.lib.dgll_hip_debug_tune(15, value), "dgll_hip_debug_tune")
    try:
        yield
    finally:
        _lib.check(_lib.lib.dgll_hip_debug_tune(15, 0), "dgll_hip_debug_tune")


def band_graph(n_rows, n_cols, avg_len, seed, special=None, weighted=True):
    rng = np.random.default_rng(seed)
    deg = rng.poisson(avg_len, n_rows)
    for r, d in (special or {}).items():
        if r < n_rows:
            deg[r] = d
    deg = np.minimum(deg, n_cols)
    rowptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = np.concatenate([np.sort(rng.choice(n_cols, d, replace=False)) for d in deg] + [np.zeros(0, np.int64)]).astype(np.int32)
    val = rng.standard_normal(col.shape[0]).astype(np.float32) if weighted else None
    return rowptr, col, val


def to_dev(rowptr, col, val, n_cols, device):
    import dgll_amd

    return dgll_amd.CSRGraph(torch.from_numpy(rowptr).to(device), torch.from_numpy(col).to(device),
                             None if val is None else torch.from_numpy(val).to(device), len(rowptr) - 1, n_cols)


def bf16_features(n, feat, seed, device, pitch=None):
    """(fp32 numpy of the bf16-rounded values, device bf16 [n, feat] view of rows `pitch` elements apart)."""
    x = torch.from_numpy(np.random.default_rng(seed).standard_normal((n, feat)).astype(np.float32)).to(torch.bfloat16)
    pitch = (feat + 7) // 8 * 8 if pitch is None else pitch
    buf = torch.full((n, pitch), float("nan"), dtype=torch.bfloat16, device=device)     # the padding must never reach a result
    xd = buf[:, :feat]
    xd.copy_(x)
    return x.to(torch.float32).numpy(), xd


@pytest.mark.parametrize("spr", [2, 4])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("feat", [7, 33, 47, 64, 100])
def test_rowgroup_vs_oracle(cuda_device, feat, weighted, reduce, spr):
    from dgll_amd import ops

    rowptr, col, val = band_graph(N_ROWS, N_ROWS, 40, seed=feat + 7 * spr, special=SPECIAL, weighted=weighted)
    g = to_dev(rowptr, col, val, N_ROWS, cuda_device)
    assert g.num_long_rows() == 2
    # rows of one 128-byte line for the narrow widths (what the engine's backward pass gathers from): ldx != ldy
    x, xd = bf16_features(N_ROWS, feat, 3, cuda_device, pitch=64 if feat < 64 else None)
    ref = cref.spmm_csr(rowptr, col, val, x, reduce=reduce)
    with rowgroup_choice(spr):
        y = ops.spmm_raw(g, xd, reduce=reduce)
        y32 = ops.spmm_raw(g, xd, reduce=reduce, out_dtype=torch.float32)
        y_again = ops.spmm_raw(g, xd, reduce=reduce)
        y32_again = ops.spmm_raw(g, xd, reduce=reduce, out_dtype=torch.float32)
    assert y.dtype == torch.bfloat16 and (feat >= 64 or y.stride(0) != xd.stride(0))
    err16 = np.abs(y.float().cpu().numpy() - ref)
    err32 = np.abs(y32.cpu().numpy() - ref)
    print("feat %d weighted %s %s spr %d: max abs err bf16 %.3e fp32 %.3e" % (feat, weighted, reduce, spr, err16.max(), err32.max()))
    np.testing.assert_allclose(y.float().cpu().numpy(), ref, rtol=8e-3, atol=8e-3)
    np.testing.assert_allclose(y32.cpu().numpy(), ref, rtol=1e-4, atol=1e-4)
    assert torch.equal(y, y_again) and torch.equal(y32, y32_again), "two launches on the same inputs differ"


@pytest.mark.parametrize("spr", [2, 4])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("feat", [33, 47, 64, 100])
def test_rowgroup_vs_old_choice(cuda_device, feat, weighted, spr):
    """Same launch through the kernel chosen before the row-group kernel existed: equal within the oracle tolerance everywhere,
    and bit-equal in the rows of at most SPR x U edges (one round: the order of the sum is the wave-per-row kernel's)."""
    from dgll_amd import ops

    rowptr, col, val = band_graph(N_ROWS, N_ROWS, 40, seed=100 + feat + spr, special=SPECIAL, weighted=weighted)
    g = to_dev(rowptr, col, val, N_ROWS, cuda_device)
    _, xd = bf16_features(N_ROWS, feat, 4, cuda_device)
    bias = torch.from_numpy(np.random.default_rng(5).standard_normal(feat).astype(np.float32)).to(cuda_device)
    kw = dict(reduce="mean", bias=bias, relu=True)
    with rowgroup_choice(1):
        old = ops.spmm_raw(g, xd, **kw)
        old32 = ops.spmm_raw(g, xd, out_dtype=torch.float32, **kw)
    with rowgroup_choice(spr):
        new = ops.spmm_raw(g, xd, **kw)
        new32 = ops.spmm_raw(g, xd, out_dtype=torch.float32, **kw)
    np.testing.assert_allclose(new.float().cpu().numpy(), old.float().cpu().numpy(), rtol=8e-3, atol=8e-3)
    np.testing.assert_allclose(new32.cpu().numpy(), old32.cpu().numpy(), rtol=1e-4, atol=1e-4)
    spr_here = 2 if feat > 64 else spr                # rows of 16 lanes exist with two slots per row only
    short = torch.from_numpy(np.diff(rowptr) <= spr_here * U).to(cuda_device)
    assert int(short.sum()) >= 10
    assert torch.equal(new32[short], old32[short]) and torch.equal(new[short], old[short])
    # rows without edges: the epilogue of an empty sum
    empty = torch.from_numpy(np.diff(rowptr) == 0).to(cuda_device)
    assert torch.equal(new32[empty], torch.relu(bias).expand(int(empty.sum()), feat))


def test_rowgroup_is_the_automatic_choice_in_its_band(cuda_device):
    """F = 47 bf16 at 40 edges per row: the automatic choice gives the forced kernel's bits (fp32 output, so that a different
    order of the sum would show)."""
    from dgll_amd import ops

    rowptr, col, val = band_graph(N_ROWS, N_ROWS, 40, seed=9, special=SPECIAL)
    g = to_dev(rowptr, col, val, N_ROWS, cuda_device)
    _, xd = bf16_features(N_ROWS, 47, 6, cuda_device)
    auto = ops.spmm_raw(g, xd, out_dtype=torch.float32)
    with rowgroup_choice(2):
        forced = ops.spmm_raw(g, xd, out_dtype=torch.float32)
    assert torch.equal(auto, forced)


@pytest.mark.parametrize("n_rows", [1, 3, 5, 17])
def test_rowgroup_few_rows(cuda_device, n_rows):
    """Fewer rows than one wavefront's share: idle lane groups write nothing (the output buffer's other rows keep their fill)."""
    from dgll_amd import ops

    n_cols = 300
    rowptr, col, val = band_graph(n_rows, n_cols, 40, seed=n_rows)
    g = to_dev(rowptr, col, val, n_cols, cuda_device)
    x, xd = bf16_features(n_cols, 47, 8, cuda_device)
    buf = torch.full((n_rows + 8, 48), 7.0, dtype=torch.float32, device=cuda_device)
    with rowgroup_choice(2):
        ops.spmm_raw(g, xd, out=buf[:n_rows, :47])
    np.testing.assert_allclose(buf[:n_rows, :47].cpu().numpy(), cref.spmm_csr(rowptr, col, val, x), rtol=1e-4, atol=1e-4)
    assert bool((buf[n_rows:] == 7.0).all()) and bool((buf[:, 47] == 7.0).all())
