"""segment_mm / gather_mm / TypedLinear without a GPU: the layer's state dict and errors, the host paths and their autograd against
the float64 reference (tests/segmm_ref.py), and the entry points' argument validation."""
import pytest
import torch

from segmm_ref import grouped_refs, segment_ids

SEGLEN = [0, 3, 0, 5, 1]


@pytest.mark.parametrize("regularizer, num_bases, shapes", [(None, None, {"W": (5, 6, 4)}), ("basis", 2, {"W": (2, 6, 4), "coeff": (5, 2)})])
def test_typed_linear_state_dict_and_host_forward(regularizer, num_bases, shapes):
    from dgll.nn import TypedLinear

    layer = TypedLinear(6, 4, 5, regularizer=regularizer, num_bases=num_bases)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == shapes
    x, t = torch.randn(9, 6), segment_ids(SEGLEN)
    w = layer.W if regularizer is None else (layer.coeff @ layer.W.view(2, -1)).view(5, 6, 4)
    want = torch.einsum("mk,mkn->mn", x, w[t])
    assert torch.allclose(layer(x, t, sorted_by_type=True), want, atol=1e-6)
    shuffle = torch.randperm(9, generator=torch.Generator().manual_seed(1))
    assert torch.allclose(layer(x[shuffle], t[shuffle]), want[shuffle], atol=1e-6)


def test_typed_linear_bdd_is_not_built():
    from dgll.nn import TypedLinear

    with pytest.raises(NotImplementedError, match="basis.*None"):
        TypedLinear(6, 4, 5, regularizer="bdd", num_bases=2)


def test_host_seglen_is_checked():
    from dgll_amd.ops_segmm import segment_mm

    a, b = torch.randn(9, 6), torch.randn(5, 6, 4)
    for bad in ([0, 3, 0, 5, 2], [0, 3, 0, 5, 0], [-1, 4, 0, 5, 1]):
        with pytest.raises(ValueError, match="seglen_a"):
            segment_mm(a, b, torch.tensor(bad))


@pytest.mark.parametrize("op", ["segment", "gather"])
def test_host_paths_and_gradients_equal_the_reference(op):
    from dgll_amd.ops_segmm import gather_mm, segment_mm

    gen = torch.Generator().manual_seed(3)
    a, b, g = (torch.randn(s, generator=gen, dtype=torch.float64) for s in ((9, 6), (5, 6, 4), (9, 4)))
    idx = segment_ids(SEGLEN)
    if op == "gather":
        idx = idx[torch.randperm(9, generator=gen)]
    a.requires_grad_(True)
    b.requires_grad_(True)
    c = gather_mm(a, b, idx_b=idx) if op == "gather" else segment_mm(a, b, torch.tensor(SEGLEN))
    c.backward(g)
    for got, want in zip((c, a.grad, b.grad), grouped_refs(a.detach(), b.detach(), g, idx)):
        assert torch.allclose(got.detach(), want, atol=1e-12)


def test_entry_points_validate_on_the_host():
    from dgll_amd import _lib

    lib = _lib.lib
    p = 4096                                      # a non-NULL, 16-byte aligned address that is never dereferenced
    assert lib.dgll_hip_segment_mm(None, None, 8, 1, p, p, 8, 2, None, 8, p, 8, 4, 8, 8, 0, 2, 1, p, 64) == -1 and "NULL" in _lib.last_error()
    assert lib.dgll_hip_segment_mm(None, p, 8, 1, p, p, 8, 2, None, 8, p, 300, 4, 8, 300, 0, 2, 1, p, 64) == -1 and "N <= 256" in _lib.last_error()
    assert lib.dgll_hip_segment_mm(None, p, 4, 1, p, p, 8, 2, None, 8, p, 8, 4, 8, 8, 0, 2, 1, p, 64) == -1 and "pitch" in _lib.last_error()
    assert lib.dgll_hip_segment_mm(None, p, 8, 7, p, p, 8, 2, None, 8, p, 8, 4, 8, 8, 0, 2, 1, p, 64) == -1 and "dtype" in _lib.last_error()
    assert lib.dgll_hip_segment_mm_pack(None, None, 0, 64, 8, 1, 2, 8, 8, 1, p) == -1 and "NULL" in _lib.last_error()
    assert lib.dgll_hip_segment_mm_pack(None, p, 0, 64, 8, 1, 2, 8, 300, 1, p) == -1 and "N = 256" in _lib.last_error()
    assert lib.dgll_hip_segment_mm_gradw(None, p, 8, None, 8, 1, p, 8, 2, None, 8, p, 64, 8, 4, 8, 8, p, 1 << 20) == -1 and "NULL" in _lib.last_error()
    assert lib.dgll_hip_segment_mm_gradw(None, p, 8, p, 8, 1, p, 8, 2, None, 8, p, 64, 8, 4, 8, 8, p, 16) == -1 and "workspace" in _lib.last_error()
