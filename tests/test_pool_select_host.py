"""ops_pool and the selection-pooling layers without a GPU: what the C ABI and the wrappers refuse (on the host, before any launch),
the keep-count arithmetic, the signatures against the header and the aliases."""
import os
import re

import pytest
import torch

from conftest import ROOT
from dgll_amd import _lib, ops_pool


def test_c_abi_refuses_on_the_host_and_matches_the_header():
    def sort(n=8, score=16, idx=16, n_out=4, max_seg=8, n_segs=1):
        return _lib.lib.dgll_hip_segment_sort(None, score, 0, n, 16, n_segs, max_seg, 16, idx, None, n_out, None)

    def fwd(n=8, F=4, x=16, out=16, n_out=4, ld=4):
        return _lib.lib.dgll_hip_pool_select(None, x, ld, 0, n, F, 16, 0, 2, 16, n_out, out, ld)

    def bwd(n=8, F=4, inv=16, n_out=4, ld=4, gx=16):
        return _lib.lib.dgll_hip_pool_select_bwd(None, 16, ld, 0, n, F, 16, 0, 2, inv, 16, ld, n_out, gx, ld, 16)

    for call, text in [(lambda: sort(n=1 << 31), "2^31"), (lambda: sort(score=None), "NULL"), (lambda: sort(idx=None), "NULL"),
                       (lambda: sort(max_seg=_lib.SEGSORT_TILE + 1), "scratch"), (lambda: fwd(n=1 << 31), "2^31"),
                       (lambda: fwd(x=None), "NULL"), (lambda: fwd(out=None), "NULL"), (lambda: fwd(F=5), "ld_x"),
                       (lambda: fwd(F=_lib.POOL_MAX_F + 1, ld=1 << 20), "[1, 65536]"), (lambda: bwd(n=1 << 31), "2^31"),
                       (lambda: bwd(inv=None), "NULL"), (lambda: bwd(F=5), "ld_x")]:
        assert call() == -1 and text in _lib.last_error()
    assert sort(n=0) == 0 and sort(n_segs=0) == 0 and sort(n_out=0) == 0 and fwd(n_out=0) == 0 and bwd(n=0) == 0   # nothing to do: no launch
    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    assert int(re.search(r"#define DGLL_SEGSORT_TILE (\d+)", text).group(1)) == _lib.SEGSORT_TILE == ops_pool.TILE
    assert int(re.search(r"#define DGLL_POOL_MAX_F (\d+)", text).group(1)) == _lib.POOL_MAX_F
    for name, code in ops_pool.ACTS.items():
        assert int(re.search(r"#define DGLL_POOL_ACT_%s (\d+)" % name.upper(), text).group(1)) == code
    for fn in ("dgll_hip_segment_sort", "dgll_hip_pool_select", "dgll_hip_pool_select_bwd"):       # one ctypes argument per parameter
        assert len(re.search(r"int %s\(([^;]*)\);" % fn, text).group(1).split(",")) == len(_lib.SIGNATURES[fn][1])


def test_wrappers_refuse_bad_arguments_and_cpu_tensors_and_the_aliases_resolve():
    import dgll
    import dgll_amd

    assert dgll.nn.GlobalPooling.TopKPooling is dgll_amd.nn.GlobalPooling.TopKPooling
    assert dgll.nn.GlobalPooling.select.SortPooling is dgll_amd.nn.GlobalPooling.SortPooling
    assert {"TopKPooling", "SAGPooling", "SortPooling", "global_sort_pool"} <= set(dgll_amd.nn.GlobalPooling.__all__)
    assert ops_pool.keep_counts([10, 3, 0, 1], ratio=0.25) == [3, 1, 0, 1] and ops_pool.keep_counts([10, 3], ratio=1.0) == [10, 3]
    assert ops_pool.keep_counts([10, 3, 0], k=4) == [4, 3, 0]
    assert ops_pool.segment_sizes("t", 5, None, None) == [5] and ops_pool.segment_sizes("t", 5, torch.tensor([2, 0, 3])) == [2, 0, 3]
    s, x = torch.zeros(6), torch.zeros(6, 4)
    idx, inv = torch.zeros(3, dtype=torch.int64), torch.zeros(6, dtype=torch.int32)
    for error, match, call in [
            (ValueError, "exactly one of ratio and k", lambda: ops_pool.segment_topk(s, ratio=0.5, k=2)),
            (ValueError, "exactly one of ratio and k", lambda: ops_pool.segment_topk(s)),
            (ValueError, r"ratio must be in \(0, 1\]", lambda: ops_pool.segment_topk(s, ratio=1.5)),
            (ValueError, r"ratio must be in \(0, 1\]", lambda: ops_pool.segment_topk(s, ratio=0.0)),
            (ValueError, "k must be an integer >= 1", lambda: ops_pool.segment_topk(s, k=0)),
            (ValueError, r"\[N\] or \[N, 1\]", lambda: ops_pool.segment_topk(x, ratio=0.5)),
            (TypeError, "float32 or bfloat16", lambda: ops_pool.segment_topk(s.double(), ratio=0.5)),
            (ValueError, "sum to the number of rows 6", lambda: ops_pool.segment_sizes("t", 6, [2, 3])),
            (ValueError, "segs or batch, not both", lambda: ops_pool.segment_sizes("t", 6, [6], torch.zeros(6, dtype=torch.int64))),
            (ValueError, "act must be one of", lambda: ops_pool.select(x, s, idx, inv, act="relu")),
            (ValueError, "needs a score", lambda: ops_pool.select(x, None, idx, inv, act="tanh")),
            (ValueError, "nonlinearity must be one of", lambda: dgll_amd.nn.GlobalPooling.TopKPooling(4, nonlinearity="relu")),
            (ValueError, r"ratio must be in \(0, 1\]", lambda: dgll_amd.nn.GlobalPooling.SAGPooling(4, ratio=2.0)),
            (RuntimeError, "GPU only", lambda: ops_pool.segment_topk(s, ratio=0.5)),
            (RuntimeError, "GPU only", lambda: ops_pool.select(x, s, idx, inv)),
            (RuntimeError, "GPU only", lambda: ops_pool.sort_pool(x, k=2)),
            (RuntimeError, "GPU only", lambda: dgll_amd.nn.GlobalPooling.SortPooling(2)(x))]:
        with pytest.raises(error, match=match):
            call()
