"""ops_spgemm without a GPU: what the C ABI and the wrappers refuse on the host, before any launch; the constants and the signatures
against the header."""
import os
import re

import pytest
import torch

from conftest import ROOT
from dgll_amd import CSRGraph, _lib, ops_spgemm

BIG = 1 << 31


def test_c_abi_refuses_on_the_host_and_matches_the_header():
    room = _lib.lib.dgll_hip_spgemm_scratch_bytes(8, 8, 1)

    def sym(M=8, K=8, N=8, a=16, nnz_a=4, b=16, nnz_b=4, c=16, total=16, scratch=16, n_bytes=room):
        return _lib.lib.dgll_hip_spgemm_symbolic(None, M, K, N, a, a, nnz_a, b, b, nnz_b, c, total, scratch, n_bytes)

    def num(M=8, N=8, a=16, nnz_a=4, nnz_b=4, col=16, nnz_c=4, scratch=16, n_bytes=room):
        return _lib.lib.dgll_hip_spgemm_numeric(None, M, 8, N, a, a, None, nnz_a, 16, 16, None, nnz_b, 16, col, None, nnz_c, scratch, n_bytes)

    def bwd(mode=0, x_rows=8, x=16, nnz_x=4, y=16, nnz_c=4, grad=16):
        return _lib.lib.dgll_hip_spgemm_bwd(None, mode, x_rows, x, x, nnz_x, 8, y, y, None, 4, 8, 16, 16, 16, nnz_c, grad)

    for call, text in [(lambda: sym(M=BIG), "2^31"), (lambda: sym(K=BIG), "2^31"), (lambda: sym(N=BIG), "2^31"),
                       (lambda: sym(nnz_a=BIG), "2^31"), (lambda: sym(nnz_b=BIG), "2^31"), (lambda: sym(a=None), "NULL"),
                       (lambda: sym(b=None), "NULL"), (lambda: sym(c=None), "NULL"), (lambda: sym(total=None), "NULL"),
                       (lambda: sym(scratch=None), "NULL"), (lambda: sym(n_bytes=room - 1), "scratch too small"),
                       (lambda: sym(N=1 << 20), "scratch too small"), (lambda: num(M=BIG), "2^31"), (lambda: num(nnz_c=BIG), "2^31"),
                       (lambda: num(a=None), "NULL"), (lambda: num(col=None), "NULL"), (lambda: num(n_bytes=room - 1), "scratch too small"),
                       (lambda: num(nnz_c=-2), "column id of B"), (lambda: bwd(mode=2), "mode"), (lambda: bwd(x_rows=BIG), "2^31"),
                       (lambda: bwd(nnz_c=BIG), "2^31"), (lambda: bwd(x=None), "NULL"), (lambda: bwd(y=None), "NULL"),
                       (lambda: bwd(grad=None), "NULL")]:
        assert call() == -1 and text in _lib.last_error()
    assert sym(M=0) == 0 and sym(nnz_a=0) == 0 and sym(nnz_b=0) == 0 and num(M=0) == 0 and num(nnz_c=0) == 0 and bwd(nnz_x=0) == 0
    assert room == 128 + 32 + 48 and _lib.lib.dgll_hip_spgemm_scratch_bytes(-1, 8, 1) == 0
    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    assert int(re.search(r"#define DGLL_SPGEMM_WAVE_MAX (\d+)", text).group(1)) == _lib.SPGEMM_WAVE_MAX == ops_spgemm.WAVE_MAX
    assert int(re.search(r"#define DGLL_SPGEMM_LDS_MAX (\d+)", text).group(1)) == _lib.SPGEMM_LDS_MAX == ops_spgemm.LDS_MAX
    assert int(re.search(r"#define DGLL_SPGEMM_BWD_B (\d+)", text).group(1)) == _lib.SPGEMM_BWD_B
    for fn in ("dgll_hip_spgemm_scratch_bytes", "dgll_hip_spgemm_symbolic", "dgll_hip_spgemm_numeric", "dgll_hip_spgemm_bwd"):
        assert len(re.search(r"\w+ %s\(([^;]*)\);" % fn, text).group(1).split(",")) == len(_lib.SIGNATURES[fn][1])
    assert _lib.lib.dgll_hip_abi_version() == 2


def test_wrappers_refuse_bad_operands_and_cpu_graphs():
    a = CSRGraph.from_coo(torch.tensor([0, 1, 1]), torch.tensor([1, 0, 2]), None, (2, 3))
    b = CSRGraph.from_coo(torch.tensor([0, 2]), torch.tensor([1, 0]), None, (3, 4))
    twice = CSRGraph(torch.tensor([0, 1, 3, 3]), torch.tensor([0, 2, 2], dtype=torch.int32), None, 3, 4)     # row 1 holds column 2 twice
    down = CSRGraph(torch.tensor([0, 2, 3]), torch.tensor([2, 1, 0], dtype=torch.int32), None, 2, 3)         # row 0 runs downwards
    square = CSRGraph.from_coo(torch.tensor([0]), torch.tensor([1]), None, (2, 2))
    for error, match, call in [
            (ValueError, "inner dimensions differ", lambda: ops_spgemm.spgemm(b, a)),
            (ValueError, "operand b must be strictly increasing", lambda: ops_spgemm.spgemm(a, twice)),
            (ValueError, "operand a must be strictly increasing", lambda: ops_spgemm.spgemm(down, b)),
            (TypeError, "must be CSRGraphs", lambda: ops_spgemm.spgemm(a, torch.zeros(3, 4))),
            (RuntimeError, "GPU only", lambda: ops_spgemm.spgemm(a, b)),
            (RuntimeError, "GPU only", lambda: ops_spgemm.spgemm(down, twice, check=False)),
            (RuntimeError, "GPU only", lambda: a @ b),
            (ValueError, "k must be an integer >= 1", lambda: ops_spgemm.khop_graph(a, 0)),
            (ValueError, "square adjacency", lambda: ops_spgemm.khop_graph(a, 2)),
            (ValueError, "square adjacency", lambda: ops_spgemm.coarsen(a, torch.zeros(2, dtype=torch.int64))),
            (ValueError, "one cluster id per node", lambda: ops_spgemm.coarsen(square, torch.zeros(3, dtype=torch.int64))),
            (RuntimeError, "GPU only", lambda: ops_spgemm.coarsen(square, torch.zeros(2, dtype=torch.int64)))]:
        with pytest.raises(error, match=match):
            call()
    assert CSRGraph.__matmul__(a, torch.zeros(3, 4)) is NotImplemented
    with pytest.raises(TypeError):
        a @ torch.zeros(3, 4)
