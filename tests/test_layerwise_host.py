"""Layer-wise samplers, host side: the numpy restatement (tests/layerwise_ref.py) reproduces every fixture the reference wrote
(tests/golden/gen_layerwise_goldens.py) -- normalisations, weights from a given draw order, block extraction -- and the arguments
are validated without a GPU."""
import glob
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import layerwise_ref as ref
from conftest import GOLDEN_DIR

FIXTURES = sorted(os.path.basename(p)[len("layerwise_"):-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "layerwise_*.npz")))


def load(name):
    d = np.load(os.path.join(GOLDEN_DIR, "layerwise_%s.npz" % name), allow_pickle=False)
    return {k: d[k] for k in d.files if k != "meta"}, json.loads(str(d["meta"]))


def lap_of(fx, meta):
    n = int(fx["n"])
    return sp.csr_matrix((fx["lap_data"], fx["lap_indices"], fx["lap_indptr"]), shape=(n, n))


def test_every_class_has_a_fixture():
    assert {"ladies", "ladies_flat", "ladies_wrs", "ladies_flat_wrs", "fastgcn", "fastgcn_flat", "fastgcn_flat_wrs",
            "fastgcn_flat_plain"} <= set(FIXTURES)


@pytest.mark.parametrize("name", FIXTURES)
def test_normalisation(name):
    fx, meta = load(name)
    n = int(fx["n"])
    A = ref.adjacency(fx["a_indptr"], fx["a_indices"], n)
    L = ref.row_normalized(A) if meta["class"].startswith("Ladies") else ref.sym_normalized_transpose(A)
    np.testing.assert_allclose(L.toarray(), lap_of(fx, meta).toarray(), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("name", FIXTURES)
def test_p_weights_and_blocks(name):
    fx, meta = load(name)
    L = lap_of(fx, meta)
    flat = bool(meta["kwargs"].get("flat", False))
    fastgcn = meta["class"].startswith("FastGCN")
    wrs = not fastgcn or bool(meta["kwargs"].get("wrs", False))
    for l in range(meta["layers"]):
        k = lambda s: fx["l%d_%s" % (l, s)]      # noqa: E731
        p = ref.column_p(L, None if fastgcn else k("rows"), flat)
        np.testing.assert_allclose(p, k("p"), rtol=1e-10, atol=1e-15)
        cols = k("cols")
        w = ref.wrs_weights(p[k("draw")], len(p)) if wrs else ref.inverse_weights(p[cols], int(k("s")))
        np.testing.assert_allclose(w, k("w"), rtol=1e-9)
        indptr, indices, values = ref.block(L, k("rows"), cols, w)
        assert np.array_equal(indptr, k("indptr"))
        ri, rv = ref.sorted_within_rows(k("indptr"), k("indices"), k("values"))
        assert np.array_equal(indices, ri)
        np.testing.assert_allclose(values, rv, rtol=1e-9)
    if meta["union"]:     # fix (b): the reference's layer-2 rows are LOCAL ids 0..|S'|-1, not the sampled nodes
        assert np.array_equal(fx["l1_rows"], np.arange(len(fx["l0_cols"])))
        assert not np.array_equal(fx["l1_rows"], fx["l0_cols"])


def test_prep_matches_the_restatement():
    from dgll_amd import prep

    fx, meta = load("fastgcn")
    n = int(fx["n"])
    A = ref.adjacency(fx["a_indptr"], fx["a_indices"], n).tocoo()
    row, col = torch.from_numpy(A.row.astype(np.int64)), torch.from_numpy(A.col.astype(np.int64))
    for g, want in ((prep.sym_normalized_transpose(row, col, n), lap_of(fx, meta)),
                    (prep.normalized_adjacency(row, col, n, symmetric=False), lap_of(*load("ladies")))):
        dense = np.zeros((n, n))
        dense[g.row_index().numpy(), g.col.numpy()] = g.val.numpy()
        np.testing.assert_allclose(dense, want.toarray(), rtol=1e-6, atol=1e-7)


def test_philox_known_answers():
    """Philox4x32-10, the samplers' generator: the published known-answer vectors."""
    from dgll_amd import _lib

    cases = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
             ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
             ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
              [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in cases:
        c, k, o = np.array(ctr, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
        assert _lib.lib.dgll_host_philox4x32_10(c.ctypes.data, k.ctypes.data, o.ctypes.data) == 0
        assert o.tolist() == want


def test_argument_validation_needs_no_gpu():
    from dgll_amd.graph import CSRGraph
    from dgll_amd.sampling import FastGCNSampler, Ladies, layerwise

    g = CSRGraph(torch.tensor([0, 1, 2], dtype=torch.int64), torch.tensor([1, 0], dtype=torch.int32), None, 2, 2)
    for bad in ([], [0], [5000], [16, -1]):
        with pytest.raises(ValueError):
            Ladies(bad, g)
        with pytest.raises(ValueError):
            FastGCNSampler(bad, g)
    with pytest.raises(ValueError):
        layerwise.LayerwiseSampler([4], g, norm="col")
    with pytest.raises(ValueError):
        layerwise.LayerwiseSampler([4], g, weights="wrs", union=True)
    assert layerwise._shift_for(1.0) == 60 and layerwise._shift_for(4096.0) == 49 and layerwise._shift_for(0.0) == 60


def test_reference_names_through_the_alias():
    import dgll  # noqa: F401
    from dgll.sampling import FastGCNSampler, FastGCNSamplerFlat, Ladies, LadiesFlatWrs, LadiesWrs  # noqa: F401

    assert issubclass(LadiesWrs, Ladies) and issubclass(LadiesFlatWrs, Ladies)


def test_c_abi_rejects_bad_arguments():
    from dgll_amd import _lib

    assert _lib.lib.dgll_hip_lw_weights(None, None, None, 4, None, 0, 10, 0, None) == -1
    assert _lib.lib.dgll_hip_lw_select(None, None, None, 10, None, 40, 0, 1, 0, 8, None, None, None, None, 8, None, None) == -1
    assert _lib.lib.dgll_hip_lw_block_fill(None, 16, 16, None, 16, 4, 10, 16, 16, 1, 16, 0, 5000, 16, 16, 16, 16, 16, 16, 16) == -1
