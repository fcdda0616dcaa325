"""kNN graphs and EdgeConv without a GPU: the float64 reference against hand-worked cases, what the wrapper and the C ABI refuse (on
the host, before any launch), and the layer's names, state-dict keys, exports and aliases."""
import numpy as np
import pytest
import torch

import knn_ref


# ---------------------------------------------------------------------------------------------------- the reference, by hand
def test_reference_on_a_line():
    """five points on a line, one segment: distances are squared, ties go to the smaller index, self comes first unless excluded"""
    x = np.array([[0.0], [1.0], [3.0], [3.0], [7.0]])
    ptr, col, dist = knn_ref.knn(x, [5], 2)
    assert list(ptr) == [0, 2, 4, 6, 8, 10]
    assert list(col) == [0, 1, 1, 0, 2, 3, 2, 3, 4, 2]          # rows 2 and 3 are duplicates: both list 2 before 3; 4 is 16 from both
    assert list(dist) == [0, 1, 0, 1, 0, 0, 0, 0, 0, 16]
    ptr, col, dist = knn_ref.knn(x, [5], 2, exclude_self=True)
    assert list(col) == [1, 2, 0, 2, 3, 1, 2, 1, 2, 3]          # row 1: 0 at 1, then 2 and 3 tie at 4 -> 2; row 2 keeps its duplicate 3
    assert list(dist) == [1, 9, 1, 4, 0, 4, 0, 4, 16, 16]


def test_reference_respects_segments_and_short_segments():
    x = np.array([[0.0, 0.0], [0.0, 1.0], [5.0, 5.0], [0.0, 0.5], [9.0, 9.0], [0.0, 0.1]])
    ptr, col, dist = knn_ref.knn(x, [2, 0, 1, 3], 2, exclude_self=True)
    assert list(ptr) == [0, 1, 2, 2, 4, 6, 8]                   # deg = min(k, size - 1): 1, 1 | (empty) | 0 | 2, 2, 2
    assert list(col) == [1, 0, 5, 4, 3, 5, 3, 4]
    assert np.allclose(dist, [1, 1, 0.16, 162 - 9 * 1 + 0.25, 153.25, 81 + 8.9 ** 2, 0.16, 81 + 8.9 ** 2])
    assert list(knn_ref.out_rowptr([2, 0, 1, 3], 2, True)) == list(ptr)
    assert list(knn_ref.out_rowptr([2, 0, 1, 3], 2, False)) == [0, 2, 4, 5, 7, 9, 11]


def test_reference_edgeconv_by_hand():
    """two destinations over three sources, F = 1 -> 1: max_j theta (h_j - h_i) + phi h_i + biases; the row without entries gets
    phi(h_i) plus the biases"""
    rowptr, col = torch.tensor([0, 2, 2, 3]), torch.tensor([1, 2, 0])
    h = torch.tensor([[1.0], [4.0], [-2.0]], dtype=torch.float64)
    wt, bt, wp, bp = (torch.tensor(v, dtype=torch.float64) for v in ([[2.0]], [0.5], [[-1.0]], [0.25]))
    out = knn_ref.edgeconv(rowptr, col, h, h, wt, bt, wp, bp)
    assert out.flatten().tolist() == [2 * 3 + 0.5 - 1 + 0.25, 0.5 - 4 + 0.25, 2 * 3 + 0.5 + 2 + 0.25]


def test_lattice_case_is_exact_in_both_dtypes():
    sizes, x, (b, e) = knn_ref.lattice_case(20, 256, 32, 256)
    assert x.shape == (sum(sizes), 256) and np.abs(x).max() <= 16 and (x == np.round(x)).all()
    assert torch.equal(torch.from_numpy(x).to(torch.bfloat16).double(), torch.from_numpy(x))
    assert 256 * 32 ** 2 < 2 ** 24                               # the largest possible distance is an exact fp32 integer
    assert e - b == 25 and (x[b:e] == x[b]).all()


# ---------------------------------------------------------------------------------------------------- refusals
def test_wrapper_refusals():
    from dgll_amd import knn as K

    x = torch.zeros(6, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        K.knn_graph(x, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        K.segmented_knn_graph(x, 2, [2, 4])
    for k in (0, -1, K.MAX_K + 1):
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            K.knn_graph(x, k)
    with pytest.raises(ValueError, match=r"D must be in \[1, 256\]"):
        K.knn_graph(torch.zeros(4, K.MAX_D + 1), 2)
    with pytest.raises(ValueError, match=r"D must be in \[1, 256\]"):
        K.knn_graph(torch.zeros(4, 0), 2)
    with pytest.raises(ValueError, match="sum to the number of points 6"):
        K.knn_graph(x, 2, [2, 3])
    with pytest.raises(ValueError, match="sum to the number of points 6"):
        K.knn_graph(x, 2, torch.tensor([7, -1]))
    with pytest.raises(ValueError, match="dist must be"):
        K.knn_graph(x, 2, dist="manhattan")
    with pytest.raises(ValueError, match="already segmented"):
        K.knn_graph(torch.zeros(2, 3, 3), 2, [3, 3])
    with pytest.raises(TypeError):
        K.knn_graph(x.double(), 2)
    with pytest.raises(RuntimeError):
        K.KNNGraph(2)(x)
    with pytest.raises(RuntimeError):
        K.SegmentedKNNGraph(2)(x, [3, 3])


def test_tile_constants_are_exported():
    from dgll_amd import _lib, knn as K

    assert (K.QUERY_TILE, K.CAND_TILE, K.MAX_K, K.MAX_D) == (_lib.KNN_QUERY_TILE, _lib.KNN_CAND_TILE, 64, 256)
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    for name, value in (("QUERY_TILE", K.QUERY_TILE), ("CAND_TILE", K.CAND_TILE), ("MAX_K", K.MAX_K), ("MAX_D", K.MAX_D)):
        assert int(re.search(r"#define DGLL_KNN_%s (\d+)" % name, text).group(1)) == value


def test_c_abi_refuses_on_the_host():
    """bad arguments are refused before any launch with code -1 and the limit in the text (no device is touched: this runs without one)"""
    from dgll_amd import _lib

    def call(ld=4, dtype=0, n=8, D=4, k=2, x=16, seg=16, rowptr=16, col=16, nnz=16, n_segs=1):
        return _lib.lib.dgll_hip_knn(None, x, ld, dtype, n, D, seg, n_segs, k, 0, rowptr, col, None, nnz)

    for k in (0, 65):
        assert call(k=k) == -1 and "[1, 64]" in _lib.last_error() and "k" in _lib.last_error()
    for D in (0, 257):
        assert call(D=D, ld=512) == -1 and "[1, 256]" in _lib.last_error()
    assert call(dtype=7) == -1 and "dtype" in _lib.last_error()
    assert call(ld=3) == -1 and "ld_x" in _lib.last_error()
    assert call(n=1 << 31) == -1 and "2^31" in _lib.last_error()
    assert call(x=None) == -1 and "NULL" in _lib.last_error()
    assert call(col=None) == -1 and "NULL" in _lib.last_error()
    assert call(n=0) == 0 and call(nnz=0) == 0                      # nothing to do: no launch, no error


# ---------------------------------------------------------------------------------------------------- the layer
def test_edgeconv_names_and_state_dict():
    from dgll_amd.nn.Convolution import EdgeConv

    conv = EdgeConv(5, 7)
    assert sorted(conv.state_dict()) == ["phi.bias", "phi.weight", "theta.bias", "theta.weight"]
    assert tuple(conv.theta.weight.shape) == (7, 5) and tuple(conv.phi.weight.shape) == (7, 5)
    assert tuple(conv.theta.bias.shape) == (7,) and tuple(conv.phi.bias.shape) == (7,)
    import inspect
    assert list(inspect.signature(EdgeConv.__init__).parameters)[1:] == ["in_feat", "out_feat", "batch_norm", "allow_zero_in_degree"]
    conv.set_allow_zero_in_degree(True)
    assert conv._allow_zero_in_degree is True


def test_edgeconv_batch_norm_raises_and_says_why():
    from dgll_amd.nn.Convolution import EdgeConv

    with pytest.raises(NotImplementedError, match="before the max"):
        EdgeConv(4, 4, batch_norm=True)


def test_edgeconv_refuses_wrong_widths_and_empty_rows():
    import dgll_amd
    from dgll_amd.nn.Convolution import EdgeConv

    g = dgll_amd.CSRGraph(torch.tensor([0, 1, 1]), torch.tensor([1], dtype=torch.int32), None, 2, 2)
    with pytest.raises(ValueError, match="features must be"):
        EdgeConv(4, 4)(g, torch.zeros(2, 3))
    with pytest.raises(ValueError, match="rows without entries"):
        EdgeConv(4, 4)(g, torch.zeros(2, 4))


def test_dgcnn_shape_of_the_model():
    from dgll_amd.nn.Convolution import DGCNN, EdgeConv

    m = DGCNN(3, hidden=(8, 8, 16), k=4, emb=32, n_classes=5)
    assert [type(c) for c in m.convs] == [EdgeConv] * 3 and [c._in_feat for c in m.convs] == [3, 8, 8]
    assert [n.num_features for n in m.norms] == [8, 8, 16]
    assert m.proj.in_features == 32 and m.proj.out_features == 32 and m.classifier[-1].out_features == 5
    with pytest.raises(RuntimeError):                               # the search has no CPU implementation
        m(torch.zeros(2, 6, 3))


def test_exports_and_aliases():
    import dgll
    import dgll.knn
    import dgll_amd
    import dgll_amd.knn
    from dgll.nn.Convolution.edgeconv import EdgeConv as alias
    from dgll_amd.nn import Convolution as conv

    names = {"EdgeConv", "DGCNN", "KNNGraph", "SegmentedKNNGraph"}
    assert names <= set(conv.__all__) and names <= set(dgll_amd.nn.__all__)
    assert alias is conv.EdgeConv and dgll.nn.Convolution.DGCNN is conv.DGCNN and dgll.nn.EdgeConv is conv.EdgeConv
    assert dgll.knn is dgll_amd.knn and dgll.knn.knn_graph is dgll_amd.knn.knn_graph
    assert conv.KNNGraph is dgll_amd.knn.KNNGraph and conv.SegmentedKNNGraph is dgll_amd.knn.SegmentedKNNGraph
    assert all(hasattr(dgll_amd.knn, n) for n in ("knn_graph", "segmented_knn_graph", "KNNGraph", "SegmentedKNNGraph"))
