"""The small-shape dense sweeps without a GPU: that the case tables of tests/dense_small_cases.py reach every instantiation and every slab
geometry they are meant to, that the exact leg's condition holds for every case, that the comparators of both legs reject one dropped or
doubled reduction row, two swapped columns and a tile transposed in place, and that the fp32 random-leg bar holds for a plain float32
product.  Everything here works on the reference arrays; no project kernel runs."""
import collections

import pytest
import torch

import dense_small_cases as sc
from dense_cases import choice


def ids(cases):
    return [c.name for c in cases]


# ---- coverage tables ------------------------------------------------------------------------------------------------------------------------
def test_mm_f32_cases_reach_every_instantiation():
    """mm_f32_mfma_kernel<NT, VEC>: all 16, each at a ragged (32 t - 5) and a full (32 t) width; VEC off by a sliced pointer and by a pitch."""
    hit = collections.defaultdict(set)
    for c in sc.MM_CASES:
        hit[sc.mm_instantiation(c)].add(c.N % 32 == 0)
    assert set(hit) == sc.MM_INSTANTIATIONS and len(sc.MM_INSTANTIATIONS) == 16
    assert all(v == {False, True} for v in hit.values())
    for nt in range(1, 9):
        assert {c.mode for c in sc.MM_CASES if sc.mm_instantiation(c)[0] == nt} == set(sc.MM_MODES)
        assert {c.ldc_vec for c in sc.MM_CASES if sc.mm_instantiation(c)[0] == nt} == {False, True}
    for vec in (False, True):       # every reduction split, row count and epilogue input with and without the float4 loads
        mine = [c for c in sc.MM_CASES if (c.mode == "vec") == vec]
        assert {(c.K1, c.K2) for c in mine} == set(sc.MM_K)
        assert {c.M for c in mine} == set(sc.MM_M)
        assert {c.epi for c in mine} == set(sc.MM_EPI)
    assert {c.entry for c in sc.MM_CASES} == {"mm", "mm2"}


def test_gradw_f32_cases_reach_every_instantiation():
    """gradw_f32_mfma_kernel<KTL, NT, VEC>: all 32, each at a ragged and a full width; every K, every (M, slabs)."""
    hit = collections.defaultdict(set)
    for c in sc.GW32_CASES:
        hit[sc.gw32_instantiation(c)].add(c.N % 32 == 0)
    assert set(hit) == sc.GW32_INSTANTIATIONS and len(sc.GW32_INSTANTIATIONS) == 32
    assert all(v == {False, True} for v in hit.values())
    assert {c.K for c in sc.GW32_CASES} == set(sc.GW32_K[4] + sc.GW32_K[8])
    assert {(c.M, c.slabs) for c in sc.GW32_CASES} == {(m, s) for m in sc.GW32_M for s in sc.GW32_SLABS}
    assert {c.mode for c in sc.GW32_CASES} == {"vec", "slice", "pitch"}
    assert any(c.slabs > sc.ceil_div(c.M, 32) for c in sc.GW32_CASES)             # more slabs than 32-row chunks
    assert {sc.gw32_used_slabs(c) for c in sc.GW32_CASES} >= {1, 2, 3, 5}


def test_fourwave_cases_reach_the_kernel_at_every_nt():
    """dense_cases.choice: every case runs gemm_bf16_nt_kernel (kernel 0) at the NT it is meant for; per route every width, an odd and an
    even chunk count, a K1 that is no multiple of 8 and every row count; overall every output form and epilogue input."""
    for c in sc.FW_CASES:
        got = choice(**sc.fw_choice_args(c))
        assert got.kernel == 0 and got.nt == sc.fw_nt(c), c.name
    assert {sc.fw_nt(c) for c in sc.FW_CASES} == set(sc.FW_NT)
    for route in sc.FW_ROUTES:
        mine = [c for c in sc.FW_CASES if c.route == route]
        assert {c.N for c in mine} == set(sc.FW_N)
        assert {c.M for c in mine} == set(sc.FW_M)
        assert {(sc.ceil_div(c.K1, 64) + sc.ceil_div(c.K2, 64)) % 2 for c in mine} == {0, 1}
        assert any(c.K1 % 8 for c in mine)
        assert {c.out for c in mine} == set(sc.FW_OUT)
        assert {c.epi for c in mine} == set(sc.FW_EPI)
    assert any(c.bits_out for c in sc.FW_CASES if c.route in ("long", "long-pair", "pitch"))
    # the routes are what they say: without the mask / with one pitch / at a shorter reduction the same launch is the resident kernel's
    assert choice(N=256, K1=100, mask=False).kernel == 1 and choice(N=256, K1=100, mask=True).kernel == 0
    assert choice(N=256, K1=100, K2=40, ldw_equal=True).kernel == 1 and choice(N=256, K1=100, K2=40, ldw_equal=False).kernel == 0
    assert choice(N=256, K1=512).kernel == 1 and choice(N=256, K1=513).kernel == 0


def test_gradw_cases_reach_every_slab_geometry():
    """gradw_splitk_kernel / gradw_reduce_kernel, from the entry point's own arithmetic (sc.gradw_geometry)."""
    geo = {c.name: sc.gradw_geometry(c) for c in sc.GRADW_CASES}
    assert {g["kslabs"] for g in geo.values()} == {(a, b) for a in range(1, 5) for b in range(0, 5)}
    assert {(c.K1, c.K2) for c in sc.GRADW_CASES} == set(sc.GRADW_SPLITS) and len(sc.GRADW_SPLITS) == 20
    assert {g["types"] for g in geo.values()} == {1, 2}
    assert {s % 2 for g in geo.values() for s in g["steps"]} == {0, 1}            # an odd count: the second half of the loop multiplies zeros
    assert {g["used"] for g in geo.values()} == sc.GRADW_USED_SLABS
    assert any(g["used"] < c.n_slabs for c, g in zip(sc.GRADW_CASES, geo.values()))
    assert any(c.M % 64 for c in sc.GRADW_CASES)                                  # a ragged last step
    assert any(sum(g["kslabs"]) % 4 for g in geo.values())                        # ks_total no multiple of 4: idle waves in the last type
    # every value of every factor meets both workgroup-type counts (K2 = 0 cannot: at most four 64-column slabs; K2 = 250 cannot: at least five)
    for key, values in (("N", sc.GRADW_N), ("K1", sc.GRADW_K1), ("K2", sc.GRADW_K2[1:-1])):
        for v in values:
            assert {geo[c.name]["types"] for c in sc.GRADW_CASES if getattr(c, key) == v} == {1, 2}, (key, v)
    for rows in sc.GRADW_ROWS:
        assert {geo[c.name]["types"] for c in sc.GRADW_CASES if (c.M, c.n_slabs) == rows} == {1, 2}, rows
    assert {c.N for c in sc.GRADW_CASES if c.N <= 128} and {c.N for c in sc.GRADW_CASES if c.N > 128}   # G's upper half idle / active


# ---- the legs, per case, on the reference arrays --------------------------------------------------------------------------------------------
def _problems(kind, case, exact):
    if kind == "gradw":
        return [p for p in sc.gradw_problems(case, exact) if p is not None]
    if kind == "mm":
        return [sc.mm_problem(case, exact)]
    if kind == "gw32":
        return [sc.gw32_problem(case, exact)]
    return [sc.fw_problem(case, exact)]


def _slabs(kind, case):
    return sc.gw32_used_slabs(case) if kind == "gw32" else 0


def _bf16_out(kind, case):
    return kind == "fw" and case.out.startswith("bf16")


def _random_ok(kind, case, got, p):
    if kind == "gradw":
        return sc.gradw_bf16_random_ok(got, p.ref)
    if kind == "fw":
        return sc.transform_random_ok(got, p.ref, not _bf16_out(kind, case))
    return sc.f32_random_ok(got, p.ref, p.bound, p.R, _slabs(kind, case))


ALL = ([("gradw", c) for c in sc.GRADW_CASES] + [("mm", c) for c in sc.MM_CASES] + [("gw32", c) for c in sc.GW32_CASES] +
       [("fw", c) for c in sc.FW_CASES])
ALL_IDS = ["%s:%s" % (k, c.name) for k, c in ALL]


@pytest.mark.parametrize("kind,case", ALL, ids=ALL_IDS)
def test_exact_leg_condition_and_comparator(kind, case):
    """max(sum |a| |b| + |addend| + |bias|) < 2**24; the reference passes its own comparator as the kernel would store it, and every small
    error is rejected -- whichever reduction row it is."""
    bf16_out = _bf16_out(kind, case)
    for p in _problems(kind, case, True):
        assert sc.exactness_holds(p)
        assert sc.exact_ok(sc.as_stored(p.ref, bf16_out), p.ref, bf16_out)
        wrong = sc.mutants(p, visible=False)
        assert set(wrong) >= ({"row dropped", "row doubled"} if min(p.ref.shape) < 2 else
                              {"row dropped", "row doubled", "columns swapped", "tile transposed"}), (case.name, sorted(wrong))
        for what, z in wrong.items():
            assert not sc.exact_ok(sc.as_stored(z, bf16_out), p.ref, bf16_out), (case.name, what)


@pytest.mark.parametrize("kind,case", ALL, ids=ALL_IDS)
def test_random_leg_comparator(kind, case):
    """The reference as stored passes; each small error is rejected (the reduction row with the largest outer product: the max-norm bars of
    the bf16 legs are the project's own and cannot see every row -- the exact leg does)."""
    bf16_out = _bf16_out(kind, case)
    for p in _problems(kind, case, False):
        assert _random_ok(kind, case, sc.as_stored(p.ref, bf16_out), p)
        wrong = sc.mutants(p, visible=True)
        assert len(wrong) >= (2 if min(p.ref.shape) < 2 else 4), (case.name, sorted(wrong))
        for what, z in wrong.items():
            assert not _random_ok(kind, case, sc.as_stored(z, bf16_out), p), (case.name, what)


F32 = [(k, c) for k, c in ALL if k in ("mm", "gw32")]


@pytest.mark.parametrize("kind,case", F32, ids=["%s:%s" % (k, c.name) for k, c in F32])
def test_f32_random_bar_holds_for_a_float32_product(kind, case):
    """(R + S + 3) * 2**-24 * (|A| @ |B| + |addend| + |bias|) is a bound for ANY order of rounded fp32 additions: numpy's float32 product
    passes it, and so does the same product summed in reversed row order."""
    p = _problems(kind, case, False)[0]
    d = p.inputs
    for P, Q in ((p.P, p.Q), (p.P.flip(1), p.Q.flip(0))):
        z = torch.from_numpy(sc.np32(P) @ sc.np32(Q))
        if kind == "mm":
            for key in ("addend", "bias"):
                if key in d:
                    z = z + d[key].float()
            if "relu" in case.epi:
                z = z.clamp(min=0)
            if "gate" in d:
                z = z * (d["gate"] > 0)
        assert z.dtype == torch.float32
        assert sc.f32_random_ok(z, p.ref, p.bound, p.R, _slabs(kind, case)), case.name
