"""points.fps / points.radius without a GPU: what the wrapper and the C ABI refuse (on the host, before any launch), the sample-count
arithmetic, the table cache, the signatures against the header and the aliases."""
import os
import re

import pytest
import torch

from conftest import ROOT
from dgll_amd import _lib, points as P


def test_sample_counts_and_refusals():
    assert P.sample_counts([10, 3, 0, 1], ratio=0.25) == [3, 1, 0, 1] and P.sample_counts([10, 3], ratio=1.0) == [10, 3]
    assert P.sample_counts([10, 3], npoints=3) == [3, 3]
    x = torch.zeros(6, 3)
    for error, match, call in [
            (ValueError, r"npoints must be in \[0, 3\]", lambda: P.sample_counts([10, 3], npoints=4)),
            (ValueError, "exactly one of ratio and npoints", lambda: P.sample_counts([10], ratio=0.5, npoints=2)),
            (ValueError, r"ratio must be in \(0, 1\]", lambda: P.sample_counts([10], ratio=1.5)),
            (RuntimeError, "GPU only", lambda: P.fps(x, ratio=0.5)),
            (RuntimeError, "GPU only", lambda: P.radius(x, x.clone(), 1.0)),
            (RuntimeError, "GPU only", lambda: P.farthest_point_sampler(x.view(2, 3, 3), 2)),
            (ValueError, r"D must be in \[1, 32\]", lambda: P.fps(torch.zeros(4, 33), ratio=0.5)),
            (ValueError, "sum to the number of points 6", lambda: P.fps(x, [2, 3], ratio=0.5)),
            (ValueError, "already segmented", lambda: P.radius_graph(torch.zeros(2, 3, 3), 1.0, [3, 3])),
            (ValueError, r"max_num_neighbors must be in \[1, 64\]", lambda: P.radius(x, x, 1.0, max_num_neighbors=65)),
            (ValueError, "r must be >= 0", lambda: P.radius(x, x, -1.0)),
            (ValueError, "only when the queries are the candidates", lambda: P.radius(x, x.clone(), 1.0, _exclude_self=True)),
            (TypeError, "float32 or bfloat16", lambda: P.fps(x.double(), ratio=0.5))]:
        with pytest.raises(error, match=match):
            call()


def test_equal_segments_take_their_tables_from_the_cache():
    P._tables.clear()
    cpu = torch.device("cpu")
    seg, out = P._seg_ptr([5, 5, 5], [2, 2, 2], cpu)
    assert seg.tolist() == [0, 5, 10, 15] and out.tolist() == [0, 2, 4, 6]
    assert P._seg_ptr([5, 5, 5], [2, 2, 2], cpu)[0] is seg and len(P._tables) == 1
    seg, out = P._seg_ptr([5, 0, 7], [2, 0, 7], cpu)                                # unequal: built per call, not kept
    assert seg.tolist() == [0, 5, 5, 12] and out.tolist() == [0, 2, 2, 9] and len(P._tables) == 1


def test_c_abi_refuses_on_the_host_and_matches_the_header_and_the_aliases_resolve():
    import dgll
    import dgll_amd

    assert dgll.points is dgll_amd.points and dgll.nn.Convolution.PointNetConv is dgll_amd.nn.Convolution.PointNetConv

    def fps(ld=4, n=8, D=4, x=16, max_seg=8, n_out=4):
        return _lib.lib.dgll_hip_fps(None, x, ld, 0, n, D, 16, 1, max_seg, 16, None, 16, None, n_out, None)

    def radius(ld=4, m=8, D=4, K=2, col=16):
        return _lib.lib.dgll_hip_radius(None, 16, ld, m, 16, 16, ld, 8, 16, 1, 0, D, 1.0, K, 0, 16, col, None, 16, 16)

    for call, text in [(lambda: fps(D=33, ld=64), "[1, 32]"), (lambda: fps(ld=3), "ld_x"), (lambda: fps(n=1 << 31), "2^31"),
                       (lambda: fps(x=None), "NULL"), (lambda: fps(max_seg=8193), "scratch"), (lambda: radius(D=0), "[1, 32]"),
                       (lambda: radius(K=65), "[1, 64]"), (lambda: radius(m=1 << 31), "2^31"), (lambda: radius(col=None), "NULL")]:
        assert call() == -1 and text in _lib.last_error()
    assert fps(n=0) == 0 and fps(n_out=0) == 0                                      # nothing to do: no launch, no error
    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    for name, value in (("FPS_MAX_D", P.MAX_D), ("FPS_MAX_REG_SEG", P.MAX_REG_SEG), ("RADIUS_MAX_K", P.MAX_K), ("RADIUS_MAX_D", _lib.RADIUS_MAX_D)):
        assert int(re.search(r"#define DGLL_%s (\d+)" % name, text).group(1)) == value
    for fn in ("dgll_hip_fps", "dgll_hip_radius"):                                  # one ctypes argument per parameter of the header
        assert len(re.search(r"int %s\(([^;]*)\);" % fn, text).group(1).split(",")) == len(_lib.SIGNATURES[fn][1])
