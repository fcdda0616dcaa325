"""dgll_hip_gat_pass without a GPU: the descriptor binding against the C struct, the pass and phase constants against the header, and
the host-side argument checks of the three passes.  Every refused descriptor holds dummy host addresses that are only inspected, never
followed: nothing is launched before every check has passed."""
import ctypes
import math
import os
import re
import subprocess

import pytest

from conftest import ROOT

_BUF = (ctypes.c_float * 64)()
P = (ctypes.addressof(_BUF) + 15) & ~15        # a 16-byte aligned address


def _desc(kind, **fields):
    """A descriptor of pass `kind` (2 heads of 4 fp32 columns, 4 x 4 nodes) that passes every check, then `fields` on top."""
    from dgll_amd import _lib

    d = _lib.GatDesc()
    d.pass_, d.dtype, d.mode, d.apply_elu = kind, _lib.F32, 0, 1
    d.rowptr = d.col = d.h = d.row_score = d.col_score = P
    d.n_rows, d.n_cols, d.heads, d.fo, d.alpha, d.ld_h = 4, 4, 2, 4, 0.2, 8
    if kind == _lib.GAT_FORWARD:
        d.out, d.ld_out, d.rowsum = P, 8, P
    elif kind == _lib.GAT_ROWS:
        d.out = d.grad_out = d.dn = d.rowsum = d.dd = d.grad_score = P
        d.ld_out = d.ld_grad_out = d.ld_dn = 8
        d.phase = _lib.GAT_ROWS_EXACT_ONLY
    else:
        d.dn = d.grad_h = d.col_dd = d.grad_score = P
        d.ld_dn = d.ld_grad_h = 8
    for name, v in fields.items():
        setattr(d, name, v)
    return d


F, R, T = 0, 1, 2       # _lib.GAT_FORWARD / GAT_ROWS / GAT_TRANSPOSED (test_constants_match_the_header holds them to the header)
_ROWSCORE = dict(col_score=None, attn2=P)
_DROP = dict(drop_seed=P, drop_p=0.5)

# (pass, fields on top of a descriptor that would pass, error code, a word of the message)
REFUSED = [
    (7, {}, -1, "pass"),
    (F, dict(dtype=7), -1, "dtype"),
    (R, dict(mode=2), -1, "mode"),
    (T, dict(heads=0), -1, "positive"),
    (F, dict(fo=6), -1, "multiple"),
    (F, dict(rowptr=None), -1, "CSR"),
    (F, dict(ld_h=10), -1, "aligned"),
    (R, dict(ld_grad_out=10), -1, "aligned"),
    (T, dict(dn=P + 4), -1, "aligned"),
    (F, dict(rowsum=None), -1, "NULL"),
    (R, dict(grad_out=None), -1, "NULL"),
    (T, dict(col_dd=None), -1, "NULL"),
    (F, dict(mode=1), -1, "rowmax"),
    (R, dict(mode=1), -1, "rowmax"),
    (T, dict(mode=1), -1, "rowmax"),
    (F, dict(raw=1, mode=1, rowmax=P), -1, "split"),
    (T, dict(edge_scale=P), -1, "permutation"),
    (T, dict(attn1=P), -1, "epilogue"),
    (T, dict(attn1=P, attn2=P), -1, "epilogue"),
    # the gathered-side scores: a stride below heads, in every pass
    (F, dict(col_score_stride=1), -1, "col_score_stride"),
    (R, dict(col_score_stride=1), -1, "col_score_stride"),
    (T, dict(col_score_stride=1), -1, "col_score_stride"),
    (F, dict(col_score_stride=-8), -1, "col_score_stride"),
    # the rows pass's dd outputs
    (R, dict(dd=None), -1, "dd"),
    (R, dict(dd=None, sd=P, sd_stride=3), -1, "sd_stride"),
    (R, dict(sd=P, sd_stride=0), -1, "sd_stride"),
    (R, dict(phase=4), -1, "partial3"),
    (R, dict(phase=5, partial3=P, dd=None, sd=P, sd_stride=4), -1, "partial3"),
    (R, dict(phase=6), -1, "partial3"),
    # the row-score form: attn2 INSTEAD of col_score, one launch, addressable by 32-bit offsets
    (F, dict(attn2=P), -1, "INSTEAD"),
    (R, dict(attn2=P), -1, "INSTEAD"),
    (F, dict(_ROWSCORE, mode=1, rowmax=P), -1, "INSTEAD"),
    (F, dict(_ROWSCORE, edge_scale=P), -1, "INSTEAD"),
    (R, dict(_ROWSCORE, phase=0), -1, "INSTEAD"),
    (F, dict(col_score=None), -1, "NULL"),
    (F, dict(_ROWSCORE, n_cols=(1 << 24) + 1), -3, "col_score"),
    (R, dict(_ROWSCORE, n_cols=(1 << 24) + 1), -3, "col_score"),
    (F, dict(_ROWSCORE, n_cols=1 << 21, ld_h=1024), -3, "col_score"),      # 2 M rows x 4 KB
    (R, dict(_ROWSCORE, n_cols=1 << 21, ld_h=1024), -3, "col_score"),
    (F, dict(_ROWSCORE, n_cols=0), -3, "col_score"),
    # dropout drawn in the kernels
    (F, dict(_DROP, attn2=P), -1, "not both"),
    (R, dict(_DROP, attn2=P), -1, "not both"),
    (F, dict(_DROP, col_score=None), -1, "not both"),
    (F, dict(_DROP, n_cols=1 << 31), -1, "32-bit"),
    (R, dict(_DROP, n_cols=1 << 31), -1, "32-bit"),
    (R, dict(_DROP, n_cols=0), -1, "32-bit"),
    (T, dict(_DROP, n_rows=1 << 31), -1, "32-bit"),
    (F, dict(_DROP, raw=1), -1, "one launch"),
    (F, dict(_DROP, accumulate=1), -1, "one launch"),
    (R, dict(_DROP, phase=1), -1, "one launch"),
    (F, dict(_DROP, edge_scale=P), -1, "in-kernel dropout"),
    (T, dict(_DROP, edge_scale=P, perm=P), -1, "in-kernel dropout"),
] + [(kind, dict(_DROP, drop_p=p), -1, "[0, 1)") for kind in (F, R, T) for p in (1.0, -0.25, math.nan)]


@pytest.mark.parametrize("kind,fields,code,word", REFUSED)
def test_refused_descriptors(kind, fields, code, word):
    from dgll_amd import _lib

    d = _desc(kind, **fields)
    assert _lib.lib.dgll_hip_gat_pass(None, ctypes.byref(d)) == code
    assert word in _lib.last_error(), _lib.last_error()


def test_null_descriptor():
    from dgll_amd import _lib

    assert _lib.lib.dgll_hip_gat_pass(None, None) == -1 and "NULL" in _lib.last_error()


@pytest.mark.parametrize("kind", [F, R, T])
def test_an_empty_pass_is_ok(kind):
    """n_rows <= 0 returns before any other field is looked at."""
    from dgll_amd import _lib

    d = _lib.GatDesc()
    d.pass_ = kind
    assert _lib.lib.dgll_hip_gat_pass(None, ctypes.byref(d)) == 0
    d.n_rows = -3
    assert _lib.lib.dgll_hip_gat_pass(None, ctypes.byref(d)) == 0


def test_constants_match_the_header():
    from dgll_amd import _lib

    text = open(os.path.join(ROOT, "include", "dgll_hip.h")).read()
    names = ["FORWARD", "ROWS", "TRANSPOSED", "ROWS_STORED_FIRST", "ROWS_STORED_FURTHER", "ROWS_EXACT_ONLY", "ROWS_EXACT_FIRST",
             "ROWS_EXACT_MIDDLE", "ROWS_EXACT_LAST"]
    for name in names:
        assert int(re.search(r"\bDGLL_GAT_%s\s*=\s*(\d+)" % name, text).group(1)) == getattr(_lib, "GAT_" + name), name
    assert (F, R, T) == (_lib.GAT_FORWARD, _lib.GAT_ROWS, _lib.GAT_TRANSPOSED)


def test_descriptor_binding_matches_the_c_struct(tmp_path):
    """_lib.GatDesc field by field against offsetof / sizeof of dgll_gat_desc as a C compiler lays it out."""
    from dgll_amd import _lib

    fields = [name for name, _ in _lib.GatDesc._fields_]
    c_names = ["pass" if f == "pass_" else f for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dgll_hip.h"\nint main(void) {\n'
                   + "".join('    printf("%%zu\\n", offsetof(dgll_gat_desc, %s));\n' % n for n in c_names)
                   + '    printf("%zu\\n", sizeof(dgll_gat_desc));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [getattr(_lib.GatDesc, f).offset for f in fields] + [ctypes.sizeof(_lib.GatDesc)]
