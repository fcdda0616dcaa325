"""The row-layout vocabulary of the wrappers (ops.rows16_ok / as_rows16 / alloc_features) and the nullable-argument helpers
(_lib.ptr / pitch) on host tensors: pointers and strides behave there as on the device."""
import pytest
import torch

CASES = [(torch.bfloat16, w) for w in (1, 7, 8, 9, 47, 48)] + [(torch.float32, w) for w in (1, 3, 4, 5)]
ROWS = 5


def _values(width, dtype):
    return (torch.arange(ROWS * width, dtype=torch.float32).reshape(ROWS, width) % 251 + 1).to(dtype)      # exact in bf16, never 0


def _layouts(width, dtype):
    """(name, [ROWS, width] tensor): contiguous, column slices of a wider buffer on an aligned and on a ragged pitch, and a slice whose
    storage offset leaves the base pointer off the 16-byte grid."""
    epv = 16 // torch.empty((), dtype=dtype).element_size()
    v = _values(width, dtype)
    yield "contiguous", v.clone()
    for name, ld, c0 in (("slice of an aligned pitch", -(-(width + 1) // epv) * epv + epv, 0), ("slice of a ragged pitch", width + epv + 1, 0),
                         ("misaligned storage offset", -(-(width + 1) // epv) * epv + epv, 1)):
        buf = torch.full((ROWS, ld), -7.0, dtype=dtype)
        x = buf[:, c0:c0 + width]
        x.copy_(v)
        yield name, x


def _expect_ok(x):
    esz = x.element_size()
    return x.stride(1) == 1 and x.stride(0) >= x.shape[1] and (x.stride(0) * esz) % 16 == 0 and x.data_ptr() % 16 == 0


@pytest.mark.parametrize("dtype,width", CASES)
def test_rows16_ok_and_as_rows16(dtype, width):
    from dgll_amd import dense, ops

    assert dense._as_rows16 is ops.as_rows16
    seen = set()
    for name, x in _layouts(width, dtype):
        ok = ops.rows16_ok(x)
        assert ok == _expect_ok(x), name
        seen.add(ok)
        for zero_pad in (False, True):
            y = ops.as_rows16(x, zero_pad=zero_pad)
            if ok:
                assert y is x, name
                continue
            assert y is not x and ops.rows16_ok(y), name
            assert y.shape == x.shape and y.dtype == x.dtype and torch.equal(y, x), name
            epv = 16 // x.element_size()
            assert y.stride(0) == -(-width // epv) * epv, name          # one copy into the narrowest 16-byte pitch
            if zero_pad:
                store = torch.empty(0, dtype=dtype).set_(y.untyped_storage(), y.storage_offset(), (ROWS, y.stride(0)), (y.stride(0), 1))
                assert torch.equal(store[:, :width], x) and bool((store[:, width:] == 0).all()), name
    assert seen == {True, False} or width == 1          # every case meets both answers
    assert not ops.rows16_ok(_values(width, dtype).t().contiguous().t()) or width == 1 or ROWS == 1      # column-major: not unit stride
    assert not ops.rows16_ok(torch.zeros(8, dtype=dtype))                                              # not a matrix


def test_misaligned_base_pointer_is_not_ok():
    buf = torch.zeros((4, 16), dtype=torch.bfloat16)
    assert ops_rows16(buf) and not ops_rows16(buf[:, 1:9]) and ops_rows16(buf[:, 8:16]) and ops_rows16(buf[1:, :8])
    overlapping = buf.as_strided((4, 16), (8, 1))
    assert not ops_rows16(overlapping)                       # rows on a 16-byte pitch that run into each other


def ops_rows16(x):
    from dgll_amd import ops

    return ops.rows16_ok(x)


@pytest.mark.parametrize("dtype,width", CASES)
def test_alloc_features_pitch(dtype, width):
    from dgll_amd import ops

    for pad_to in (1, 4, 8, 16, 64):
        y = ops.alloc_features(ROWS, width, dtype, "cpu", pad_to=pad_to)
        assert y.shape == (ROWS, width) and y.dtype == dtype and y.stride() == (-(-width // pad_to) * pad_to, 1)
        z = ops.alloc_features(ROWS, width, dtype, "cpu", pad_to=pad_to, zero_pad=True)
        assert z.stride() == y.stride()
        z.fill_(1)
        store = torch.empty(0, dtype=dtype).set_(z.untyped_storage(), 0, (ROWS, z.stride(0)), (z.stride(0), 1))
        assert bool((store[:, width:] == 0).all()) and bool((store[:, :width] == 1).all())
    assert ops.alloc_features(ROWS, width, dtype, "cpu").stride(0) == -(-width // 8) * 8          # the default: 8 elements


def test_edge_wrappers_keep_their_meaning():
    """ops_edge's names over the shared helpers: _ready zero-fills its copy, _empty_padded pads to one vector, _empty_like_rows
    takes another matrix's pitch."""
    from dgll_amd import ops_edge

    x = torch.full((3, 41), 5.0, dtype=torch.bfloat16)[:, :7]          # an 82-byte pitch
    y = ops_edge._ready(x)
    assert y.stride(0) == 8 and torch.equal(y, x) and bool((y.as_strided((3, 8), (8, 1))[:, 7:] == 0).all())
    assert ops_edge._empty_padded(3, 47, torch.bfloat16, "cpu").stride(0) == 48
    assert ops_edge._empty_padded(3, 5, torch.float32, "cpu").stride(0) == 8
    like = torch.zeros((2, 64), dtype=torch.bfloat16)[:, :16]
    e = ops_edge._empty_like_rows(9, like)
    assert e.shape == (9, 16) and e.stride() == (64, 1) and e.dtype == like.dtype
    assert ops_edge._empty_like_rows(9, torch.zeros(2, 16)).stride() == (16, 1)


def test_mfma_and_gradw_predicates_on_host_tensors():
    """dense._mfma_ok / _gradw_ok share the pitch test but keep their own clauses: device and dtype first, None allowed / refused."""
    from dgll_amd import dense

    x = torch.zeros((4, 8), dtype=torch.bfloat16)
    assert dense._mfma_ok(None) and dense._mfma_ok() and not dense._mfma_ok(x) and not dense._mfma_ok(None, x)      # host tensors never
    assert not dense._gradw_ok(None) and not dense._gradw_ok(x) and dense._gradw_ok()


def test_ptr_and_pitch():
    from dgll_amd import _lib

    assert _lib.ptr(None) is None and _lib.pitch(None) == 0
    buf = torch.zeros((6, 48), dtype=torch.bfloat16)
    view = buf[2:, 8:30]
    assert _lib.ptr(view) == buf.data_ptr() + (2 * 48 + 8) * 2 and _lib.pitch(view) == 48
    assert _lib.ptr(buf) == buf.data_ptr() and _lib.pitch(buf) == 48
    assert _lib.pitch(buf[::2]) == 96


def test_launch_timer_is_one_class():
    from dgll_amd import _lib, ops

    assert ops.LaunchTimer is _lib.LaunchTimer and ops.LaunchTimer.active is None
    with ops.LaunchTimer() as t:
        assert _lib.LaunchTimer.active is t
    assert _lib.LaunchTimer.active is None
